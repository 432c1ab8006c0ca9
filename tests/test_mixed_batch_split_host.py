"""CPU-side checks of the depth split of a mixed step's attention tiles (csrc/gl3_batch_plan.h: batch_plan_split, through
gl3_debug_batch_plan_split — plain arrays in and out, no plan, no device): the shallow 8-row tiles of the one-launch table form, the deep
records of at most 16 rows of the long-context trio's table form, and the list of deep step rows the softmax launch covers."""
import ctypes

import numpy as np

from test_mixed_batch_host import RUNS, _hip, _p, batch_plan, rows_of

DEEP_ROWS = 16                               # PA_TB = SCM_TB = PVM_TB: rows of a deep record


def split(hip, seq_ids, positions, fused_max_pos, n_seqs=8, ctx=64, capacity=64):
    """-> (code, shallow [s][4], deep [d][4], deep rows); records are (first row, rows, sequence, position of the first row)"""
    s, p = np.ascontiguousarray(seq_ids, np.int32), np.ascontiguousarray(positions, np.int32)
    n = s.size
    sh, dp, rows = np.full((max(n, 1), 4), -7, np.int32), np.full((max(n, 1), 4), -7, np.int32), np.full(max(n, 1), -7, np.int32)
    ns, nd, nr = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    code = hip.lib().gl3_debug_batch_plan_split(_p(s), _p(p), n, n_seqs, ctx, capacity, fused_max_pos, _p(sh), ctypes.byref(ns), _p(dp), ctypes.byref(nd),
                                                _p(rows), ctypes.byref(nr))
    if code != 0:
        return code, None, None, None
    return code, sh[:ns.value].tolist(), dp[:nd.value].tolist(), rows[:nr.value].tolist()


def last(rec):
    return rec[3] + rec[1] - 1


def covered(recs):
    return sorted(r for t in recs for r in range(t[0], t[0] + t[1]))


def test_the_library_exports_the_split_and_the_dispatch_tap(pkg):
    hip = _hip()
    names = hip.check_exports()                   # header == ctypes table == exported symbols
    for name in ("gl3_debug_batch_plan_split", "gl3_get_attn_rows"):
        assert name in names and name in hip._SIGS
    assert hip.lib().gl3_get_attn_rows(None, None) == hip.E_ARG
    from importlib import import_module
    import __graft_entry__ as ge
    assert callable(import_module(ge.PKG_NAME + ".plan").HipMasterPlan.attn_rows)


def test_a_limit_at_or_past_ctx_is_todays_table(pkg):
    hip = _hip()
    seqs, poss = rows_of(RUNS)
    _, _, tiles, _ = batch_plan(hip, seqs, poss)
    for fmp in (64, 63, 1 << 30, 0x7FFFFFFF):
        code, sh, dp, rows = split(hip, seqs, poss, fmp)
        assert code == 0 and sh == tiles and dp == [] and rows == []
    code, sh, dp, rows = split(hip, seqs, poss, 56)      # the deepest row of the step
    assert code == 0 and sh == tiles and dp == [] and rows == []


def test_no_limit_makes_every_row_deep(pkg):
    hip = _hip()
    seqs, poss = rows_of(RUNS)                    # 1, 8, 9 and 17 rows
    code, sh, dp, rows = split(hip, seqs, poss, -1)
    assert code == 0 and sh == [] and rows == list(range(len(seqs))) and covered(dp) == rows
    assert sorted(d[1] for d in dp) == [1, 1, 8, 9, 16]
    for row0, n, seq, pos0 in dp:
        assert 1 <= n <= DEEP_ROWS and len(set(seqs[row0:row0 + n])) == 1 and seqs[row0] == seq and poss[row0] == pos0


def test_a_run_that_straddles_the_limit(pkg):
    """37 rows from position 30, limit 47: tiles 30..37 and 38..45 are shallow, tile 46..53 is deep (its last position is past 47, although its
    first two rows are not), so the deep suffix starts at row 16: 16 + 5 rows."""
    hip = _hip()
    runs = [(2, 3, 1), (0, 30, 37), (1, 0, 4)]    # a decode row in front (rows shift by one) and a short run behind
    seqs, poss = rows_of(runs)
    code, sh, dp, rows = split(hip, seqs, poss, 47, ctx=128)
    assert code == 0
    assert sh == [[9, 8, 0, 38], [1, 8, 0, 30], [0, 1, 2, 3], [38, 4, 1, 0]]       # deepest last position first: 45, 37, 3, 3 (stable)
    assert dp == [[33, 5, 0, 62], [17, 16, 0, 46]]                                  # last positions 66, 61
    assert rows == list(range(17, 38))
    # the same run alone: row numbers as in the issue
    seqs, poss = rows_of([(0, 30, 37)])
    code, sh, dp, rows = split(hip, seqs, poss, 47, ctx=128)
    assert code == 0 and sorted(sh) == [[0, 8, 0, 30], [8, 8, 0, 38]] and sorted(dp) == [[16, 16, 0, 46], [32, 5, 0, 62]] and rows == list(range(16, 37))
    # one position more and the third tile's last position is still past the limit; at 53 it is shallow
    assert len(split(hip, seqs, poss, 52, ctx=128)[1]) == 2
    code, sh, dp, rows = split(hip, seqs, poss, 53, ctx=128)
    assert len(sh) == 3 and dp == [[24, 13, 0, 54]] and rows == list(range(24, 37))


def test_deep_records_never_cross_a_run_boundary(pkg):
    hip = _hip()
    runs = [(0, 50, 20), (1, 50, 20), (2, 100, 3)]      # two deep suffixes of 20 rows side by side: 16 + 4 each, not 16 + 16 + 8
    seqs, poss = rows_of(runs)
    code, sh, dp, rows = split(hip, seqs, poss, 49, ctx=128)
    assert code == 0 and sh == [] and rows == list(range(43))
    assert sorted(dp) == [[0, 16, 0, 50], [16, 4, 0, 66], [20, 16, 1, 50], [36, 4, 1, 66], [40, 3, 2, 100]]
    for row0, n, seq, pos0 in dp:
        assert len(set(seqs[row0:row0 + n])) == 1 and seqs[row0] == seq and poss[row0] == pos0


def test_both_tables_are_ordered_deepest_first_and_stable(pkg):
    hip = _hip()
    runs = [(0, 50, 20), (1, 50, 20), (3, 0, 9), (2, 100, 3), (4, 0, 9)]
    seqs, poss = rows_of(runs)
    code, sh, dp, rows = split(hip, seqs, poss, 49, ctx=128)
    assert code == 0
    assert [last(t) for t in sh] == sorted((last(t) for t in sh), reverse=True)
    assert [last(t) for t in dp] == sorted((last(t) for t in dp), reverse=True)
    # ties keep row order (a stable sort over records made in row order)
    assert sh == [[48, 1, 3, 8], [60, 1, 4, 8], [40, 8, 3, 0], [52, 8, 4, 0]]
    assert dp == [[49, 3, 2, 100], [16, 4, 0, 66], [36, 4, 1, 66], [0, 16, 0, 50], [20, 16, 1, 50]]
    assert rows == sorted(rows) == covered(dp) and sorted(covered(sh) + rows) == list(range(len(seqs)))


def test_a_deep_decode_row_is_a_one_row_record(pkg):
    hip = _hip()
    seqs, poss = rows_of([(0, 0, 12), (1, 560, 1), (2, 3, 1)])
    code, sh, dp, rows = split(hip, seqs, poss, 511, ctx=600)
    assert code == 0 and dp == [[12, 1, 1, 560]] and rows == [12]
    assert sh == [[8, 4, 0, 8], [0, 8, 0, 0], [13, 1, 2, 3]]
    code, sh, dp, rows = split(hip, seqs, poss, 560, ctx=600)      # the limit is inclusive
    assert code == 0 and dp == [] and rows == [] and len(sh) == 4


def test_the_deep_rows_are_the_union_of_the_deep_records(pkg):
    hip = _hip()
    rng = np.random.default_rng(5)
    for _ in range(40):
        order = rng.permutation(8)[:rng.integers(1, 6)]
        runs = [(int(s), int(rng.integers(0, 90)), int(rng.integers(1, 30))) for s in order]
        seqs, poss = rows_of(runs)
        fmp = int(rng.integers(-1, 130))
        code, sh, dp, rows = split(hip, seqs, poss, fmp, ctx=128, capacity=256)
        assert code == 0
        assert rows == sorted(set(rows)) == covered(dp)
        assert sorted(covered(sh) + rows) == list(range(len(seqs)))
        assert all(last(t) <= fmp and t[1] <= 8 for t in sh) and all(d[1] <= DEEP_ROWS for d in dp)
        _, plan_runs, tiles, _ = batch_plan(hip, seqs, poss, ctx=128, capacity=256)
        assert sh == [t for t in tiles if last(t) <= fmp]
        for row0, n, seq, pos0 in plan_runs:      # shallow rows are a prefix of their run, deep records start at its first deep row
            deep_here = [r for r in rows if row0 <= r < row0 + n]
            assert deep_here == list(range(row0 + n - len(deep_here), row0 + n))
            recs = sorted(d for d in dp if row0 <= d[0] < row0 + n)
            assert [d[0] for d in recs] == list(range(row0 + n - len(deep_here), row0 + n, DEEP_ROWS))
            assert all(d[2] == seq and d[3] == pos0 + d[0] - row0 for d in recs)
            if deep_here:                         # the tile the first deep row starts ends past the limit
                o = deep_here[0] - row0
                assert o % 8 == 0 and pos0 + min(o + 8, n) - 1 > fmp


def test_what_the_plan_refuses_the_split_refuses(pkg):
    hip = _hip()
    E = hip.E_ARG
    for fmp in (-1, 10, 1 << 20):
        assert split(hip, [0, 0, 1], [3, 4, 0], fmp)[0] == 0
        assert split(hip, [0, 0, 1, 0], [3, 4, 0, 5], fmp)[0] == E           # a sequence split into two runs
        assert split(hip, [0, 0, 1], [3, 5, 0], fmp)[0] == E                 # a gap
        assert split(hip, [0, 0, 1], [4, 3, 0], fmp)[0] == E                 # a descending pair
        seqs, poss = rows_of([(2, 60, 5)])
        assert split(hip, seqs, poss, fmp, ctx=64)[0] == E                   # a run ending at ctx + 1
        seqs, poss = rows_of([(0, 0, 9)])
        assert split(hip, seqs, poss, fmp, capacity=9)[0] == 0 and split(hip, seqs, poss, fmp, capacity=8)[0] == E
        assert split(hip, [8], [0], fmp, n_seqs=8)[0] == E and split(hip, [-1], [0], fmp)[0] == E and split(hip, [0], [-1], fmp)[0] == E
    L = hip.lib()
    one = ctypes.c_int32()
    buf = np.zeros(8, np.int32)
    assert L.gl3_debug_batch_plan_split(None, None, 1, 8, 64, 64, 10, _p(buf), ctypes.byref(one), _p(buf), ctypes.byref(one), _p(buf), ctypes.byref(one)) == E
    assert L.gl3_debug_batch_plan_split(_p(buf), _p(buf), 0, 8, 64, 64, 10, _p(buf), ctypes.byref(one), _p(buf), ctypes.byref(one), _p(buf), ctypes.byref(one)) == E
    assert L.gl3_debug_batch_plan_split(_p(buf), _p(buf), 1, 8, 64, 64, 10, None, ctypes.byref(one), _p(buf), ctypes.byref(one), _p(buf), ctypes.byref(one)) == E
