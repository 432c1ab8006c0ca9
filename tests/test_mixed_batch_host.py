"""CPU-side checks of the mixed batched step's C-ABI (gl3_forward_batch, gl3_forward_batch_sample) and of its host-side step plan
(csrc/gl3_batch_plan.h through gl3_debug_batch_plan: plain arrays in and out, no plan, no device): runs, attention tiles, output rows
and every refusal the run structure can earn."""
import ctypes
import os

import numpy as np

import __graft_entry__ as ge

NEW = ["gl3_forward_batch", "gl3_forward_batch_sample", "gl3_debug_batch_plan"]
TILE_ROWS = 8                                # FA_TB: rows of an attention tile


def _hip():
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgpullama_hip.so")):
        ge.build()
    ge.load_package()
    from importlib import import_module
    return import_module(ge.PKG_NAME + ".hip")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def batch_plan(hip, seq_ids, positions, want=None, n_seqs=8, ctx=64, capacity=64):
    """-> (code, runs [r][4], tiles [t][4], output rows); records are (first row, rows, sequence, position of the first row)"""
    s, p = np.ascontiguousarray(seq_ids, np.int32), np.ascontiguousarray(positions, np.int32)
    w = np.ascontiguousarray(want, np.int8) if want is not None else None
    n = s.size
    runs, tiles, outs = np.full((n, 4), -7, np.int32), np.full((n, 4), -7, np.int32), np.full(n, -7, np.int32)
    nr, nt, no = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    code = hip.lib().gl3_debug_batch_plan(_p(s), _p(p), _p(w), n, n_seqs, ctx, capacity, _p(runs), ctypes.byref(nr), _p(tiles), ctypes.byref(nt),
                                          _p(outs), ctypes.byref(no))
    if code != 0:
        return code, None, None, None
    return code, runs[:nr.value].tolist(), tiles[:nt.value].tolist(), outs[:no.value].tolist()


def rows_of(runs):
    """runs [(sequence, first position, rows)] -> (seq_ids, positions)"""
    seqs, poss = [], []
    for seq, pos0, rows in runs:
        seqs += [seq] * rows
        poss += list(range(pos0, pos0 + rows))
    return seqs, poss


def test_the_library_exports_the_mixed_step(pkg):
    hip = _hip()
    names = hip.check_exports()                   # header == ctypes table == exported symbols
    raw = ctypes.CDLL(hip.SO_PATH)
    for name in NEW:
        assert name in names and name in hip._SIGS
        getattr(raw, name)
    L = hip.lib()
    assert L.gl3_forward_batch(None, None, None, None, None, 1, None, None) == hip.E_ARG
    assert L.gl3_forward_batch_sample(None, None, None, None, None, 1, None, None, None, None) == hip.E_ARG
    from importlib import import_module
    plan_mod = import_module(ge.PKG_NAME + ".plan")
    for name in ("forward_batch", "forward_batch_sample"):
        assert callable(getattr(plan_mod.HipMasterPlan, name))


RUNS = [(3, 0, 1), (0, 5, 8), (5, 0, 9), (1, 40, 17)]      # (sequence, first position, rows): 1, 8, 9 and 17 rows at 0, 5, 0 and 40


def test_runs_tiles_and_default_output_rows(pkg):
    hip = _hip()
    seqs, poss = rows_of(RUNS)
    code, runs, tiles, outs = batch_plan(hip, seqs, poss)
    assert code == 0
    first = [0, 1, 9, 18]
    assert runs == [[first[i], r[2], r[0], r[1]] for i, r in enumerate(RUNS)]
    # tiles: 1 / 8 / 8 + 1 / 8 + 8 + 1 rows, none across a run boundary, first position and sequence of each
    want = []
    for (row0, rows, seq, pos0) in runs:
        for o in range(0, rows, TILE_ROWS):
            want.append([row0 + o, min(TILE_ROWS, rows - o), seq, pos0 + o])
    assert sorted(tiles) == sorted(want)
    assert sorted(t[1] for t in tiles) == sorted([1, 8, 8, 1, 8, 8, 1])
    for row0, rows, seq, pos0 in tiles:
        assert 1 <= rows <= TILE_ROWS
        assert len(set(seqs[row0:row0 + rows])) == 1 and seqs[row0] == seq and poss[row0] == pos0
    covered = sorted(r for t in tiles for r in range(t[0], t[0] + t[1]))
    assert covered == list(range(len(seqs)))
    # deepest last position first
    last = [t[3] + t[1] - 1 for t in tiles]
    assert last == sorted(last, reverse=True) and last[0] == 56 and last[-1] == 0
    assert outs == [0, 8, 17, 34]                 # the four run ends


def test_an_explicit_want_logits_is_honoured_in_row_order(pkg):
    hip = _hip()
    seqs, poss = rows_of(RUNS)
    want = np.zeros(len(seqs), np.int8)
    flagged = [33, 2, 9, 10, 0]
    want[flagged] = [1, 5, -1, 1, 1]              # any non-zero value flags a row
    code, runs, tiles, outs = batch_plan(hip, seqs, poss, want)
    assert code == 0 and outs == sorted(flagged) and len(runs) == 4 and len(tiles) == 7
    code, _, _, outs = batch_plan(hip, seqs, poss, np.zeros(len(seqs), np.int8))
    assert code == 0 and outs == []               # no output rows: a pure multi-sequence prefill
    code, _, _, outs = batch_plan(hip, seqs, poss, np.ones(len(seqs), np.int8))
    assert code == 0 and outs == list(range(len(seqs)))


def test_single_rows_are_one_tile_each(pkg):
    hip = _hip()
    code, runs, tiles, outs = batch_plan(hip, [4, 1, 0], [7, 30, 2])
    assert code == 0 and runs == [[0, 1, 4, 7], [1, 1, 1, 30], [2, 1, 0, 2]] and outs == [0, 1, 2]
    assert tiles == [[1, 1, 1, 30], [0, 1, 4, 7], [2, 1, 0, 2]]


def test_what_the_run_structure_refuses(pkg):
    hip = _hip()
    E = hip.E_ARG
    ok = batch_plan(hip, [0, 0, 1], [3, 4, 0])[0]
    assert ok == 0
    assert batch_plan(hip, [0, 0, 1, 0], [3, 4, 0, 5])[0] == E           # a sequence split into two runs
    assert batch_plan(hip, [0, 0, 1], [3, 5, 0])[0] == E                 # a gap
    assert batch_plan(hip, [0, 0, 1], [4, 3, 0])[0] == E                 # a descending pair
    assert batch_plan(hip, [0, 0, 1], [3, 3, 0])[0] == E                 # a repeated position
    seqs, poss = rows_of([(2, 60, 4)])
    assert batch_plan(hip, seqs, poss, ctx=64)[0] == 0                   # ends at the last position of the context
    seqs, poss = rows_of([(2, 60, 5)])
    assert batch_plan(hip, seqs, poss, ctx=64)[0] == E                   # a run ending at ctx + 1
    seqs, poss = rows_of([(0, 0, 9)])
    assert batch_plan(hip, seqs, poss, capacity=9)[0] == 0
    assert batch_plan(hip, seqs, poss, capacity=8)[0] == E               # n above the capacity
    assert batch_plan(hip, [8], [0], n_seqs=8)[0] == E and batch_plan(hip, [-1], [0])[0] == E      # sequence out of range
    assert batch_plan(hip, [0], [-1])[0] == E
    L = hip.lib()
    one = ctypes.c_int32()
    buf = np.zeros(8, np.int32)
    assert L.gl3_debug_batch_plan(None, None, None, 1, 8, 64, 64, _p(buf), ctypes.byref(one), _p(buf), ctypes.byref(one), _p(buf), ctypes.byref(one)) == E
    assert L.gl3_debug_batch_plan(_p(buf), _p(buf), None, 0, 8, 64, 64, _p(buf), ctypes.byref(one), _p(buf), ctypes.byref(one), _p(buf), ctypes.byref(one)) == E
