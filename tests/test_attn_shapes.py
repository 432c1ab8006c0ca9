"""What the attention shape grid (tests/attn_shapes.py) covers, and the dispatch rule it states, checked without a GPU: against fixed
expectations, and against the library's own decode attention plan (csrc/gl3_decode_attn.h through gl3_debug_decode_attn_plan: plain
integers in, plain arrays out, no plan, no device)."""
import ctypes
from importlib import import_module

import numpy as np

import __graft_entry__ as ge
import attn_shapes as sh

# launch records of gl3_debug_decode_attn_plan: kernel ids in the order of include/gpullama3_hip.h
HEAD, SCORES, SCORES_LOOP, SOFTMAX_PV, EXP, SUM, PV = range(7)
REGIME_OF = {(HEAD,): "head", (SCORES, SOFTMAX_PV): "pair", (SCORES_LOOP, EXP, SUM, PV): "long-loop", (SCORES, EXP, SUM, PV): "long-tile"}
REGIME_CODE = {"head": 1, "pair": 2, "long-loop": 0, "long-tile": 0}      # AttnRegime: ATT_LONG 0, ATT_SHORT 1, ATT_MID 2


def library_plan(hs, kvmul, pos, head_kernel=True, attn_mid=sh.ATTN_MID, ctx=sh.CTX, window=None, group=1, kv_heads=2):
    """-> (regime code, launches [(kernel, grid x, grid y, block, LDS bytes, LDS cap)], (attn_head_smem(hs, group), admitted, admitted with group))"""
    ge.load_package()
    lib = import_module(ge.PKG_NAME + ".hip").lib()
    regime, n = ctypes.c_int32(-1), ctypes.c_int32(-1)
    launches, head = np.full((4, 6), -7, np.int64), np.full(3, -7, np.int64)
    code = lib.gl3_debug_decode_attn_plan(hs, kvmul, kvmul * kv_heads, kv_heads, ctx, window if window is not None else min((ctx + 3) & ~3, 16384), attn_mid,
                                          int(head_kernel), pos, group, ctypes.byref(regime), launches.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n),
                                          head.ctypes.data_as(ctypes.c_void_p))
    assert code == 0, (code, hs, kvmul, pos)
    return regime.value, [tuple(r) for r in launches[:n.value].tolist()], tuple(head.tolist())


def test_the_grid_covers_every_head_size_kvmul_and_family():
    """Computed from the grid: the head sizes, the kvMul set of each kernel class (looping scores kernel, one-tile scores kernel, 1024-thread
    workgroups, the attn_head_kernel group forms) and the families at the new head sizes.  Dropping a row must fail: every row is the only
    one that meets some requirement."""
    names = sorted(sh.SHAPES)
    assert sh.missing(names) == []
    for drop in names:
        assert sh.missing([n for n in names if n != drop]), "the grid covers the same without %s" % drop
    assert {sh.head_size_of(n) for n in names} >= {32, 64, 128, 160, 192, 224, 256}
    assert {sh.kvmul_of(n) for n in names} >= {1, 2, 3, 5, 7, 8, 16}
    assert all(sh.SHAPES[n][3] >= 2 for n in names if n != "llama-hs256-kv16")


def test_every_shape_is_a_tiny_config_the_library_accepts(pkg):
    for name in sh.SHAPES:
        c = sh.shape_config(pkg.synth, name, 1100)
        assert (c.dim, c.hidden, c.n_layers, c.vocab, c.ctx) == (256, 512, 2, 512, 1100)
        assert c.head_size % 32 == 0 and 32 <= c.head_size <= 256 and c.n_heads % c.n_kv_heads == 0 and c.n_heads // c.n_kv_heads <= 16      # gl3_create
        assert sh.scores_kernel_lds(c.head_size, c.n_heads // c.n_kv_heads) <= 128 * 1024      # what gl3_create allows attn_scores_kernel
    assert sh.scores_kernel_lds(256, 16) > 64 * 1024                                                 # ... and more than a launch gets unasked


def test_the_dispatch_rule():
    """attn_head_kernel exists up to head size 128; the group form of a static-batched step up to kvMul 8; the decode regimes change at 128 and 768"""
    assert [hs for hs in range(32, 257, 32) if sh.has_head_kernel(hs)] == [32, 64, 96, 128]
    assert sh.attn_head_smem(128) == 134720 and sh.attn_head_smem(160) > sh.LDS_MAX
    assert [sh.bd_group(128, m) for m in (4, 5, 7, 8, 16)] == [4, 5, 7, 8, 1] and sh.bd_group(64, 16) == 1
    assert [sh.decode_regime(64, 5, p) for p in (0, 127, 128, 767, 768)] == ["head", "head", "pair", "pair", "long-tile"]
    assert [sh.decode_regime(64, 5, p, head_kernel=False) for p in (0, 127, 128)] == ["pair"] * 3
    assert [sh.decode_regime(160, 2, p) for p in (0, 127, 767, 768)] == ["pair", "pair", "pair", "long-tile"]
    assert sh.decode_regime(128, 3, 768) == sh.decode_regime(64, 2, 1030) == "long-loop" and sh.decode_regime(32, 4, 768) == "long-tile"
    assert sh.batched_rows(64, [3, 127]) == [2, 0, 0, 0] and sh.batched_rows(64, [3, 128]) == [0, 0, 0, 2] and sh.batched_rows(160, [3]) == [0, 0, 0, 1]
    assert not any(sh.has_tiled_prefill(hs, 1) for hs in (160, 192, 224, 256)) and sh.has_tiled_prefill(32, 16)


def test_the_decode_walk_meets_every_regime_of_every_shape():
    """The positions at which tests/test_gpu_attn_shapes.py decodes: every shape runs each regime it has, the looping scores kernel sees 2 and 3
    chain wavefronts at both of its head sizes, the one-tile scores kernel every kvMul on the four-launch path."""
    names = sorted(sh.SHAPES)
    for name in names:
        hs, kvmul = sh.head_size_of(name), sh.kvmul_of(name)
        seen = {sh.decode_regime(hs, kvmul, p) for p in sh.DECODE_AT}
        assert seen == ({"head"} if sh.has_head_kernel(hs) else set()) | {"pair", "long-loop" if kvmul <= 4 and hs in (64, 128) else "long-tile"}, name
    at_768 = lambda n: sh.decode_regime(sh.head_size_of(n), sh.kvmul_of(n), 768)
    assert {(sh.kvmul_of(n), sh.head_size_of(n)) for n in names if at_768(n) == "long-loop"} == {(2, 64), (3, 64), (2, 128), (3, 128)}
    assert {sh.kvmul_of(n) for n in names if at_768(n) == "long-tile"} >= {1, 2, 3, 5, 7, 8, 16}
    assert {127, 128, 767, 768} <= set(sh.DECODE_AT) and max(sh.DECODE_AT) >= sh.PV_ROWS + 6 and max(sh.DECODE_AT) // 64 + 1 > 16
    assert sh.CTX % 4 == 0 and not set(sh.PREFILL_KV_AT) & set(sh.DECODE_AT)
    for edge in (64, 128, 768, 1024):
        assert max(p for p in sh.PREFILL_KV_AT if p < edge) >= edge - 3 and min(p for p in sh.PREFILL_KV_AT if p >= edge) <= edge + 3


def test_the_dispatch_rule_is_the_librarys_plan():
    """decode_regime, has_head_kernel, attn_head_smem, the size condition of bd_group and scores_kernel_lds equal csrc/gl3_decode_attn.h on every
    head size and kvMul gl3_create accepts, either side of each regime boundary at context 1100, with and without the head kernel, with the
    two-launch pair at its default depth and switched off; and no launch of any of these plans asks for more LDS than its kernel's cap."""
    for hs in range(32, 257, 32):
        for kvmul in range(1, 17):
            for group in (1, kvmul):
                smem, admitted, admitted_group = library_plan(hs, kvmul, 0, group=group)[2]
                assert smem == sh.attn_head_smem(hs, group) and bool(admitted) == sh.has_head_kernel(hs), (hs, kvmul, group)
                assert bool(admitted_group) == (sh.attn_head_smem(hs, group) <= sh.LDS_MAX), (hs, kvmul, group)
            assert sh.bd_group(hs, kvmul) == (kvmul if kvmul <= 8 and admitted_group else 1), (hs, kvmul)
            for head_kernel in (True, False):
                for attn_mid in (768, 0):
                    for pos in (0, 127, 128, 767, 768, 1030):
                        case = (hs, kvmul, pos, head_kernel, attn_mid)
                        code, launches, _ = library_plan(hs, kvmul, pos, head_kernel, attn_mid)
                        want = sh.decode_regime(hs, kvmul, pos, head_kernel, attn_mid)
                        assert REGIME_OF[tuple(k[0] for k in launches)] == want and code == REGIME_CODE[want], case
                        for kernel, gx, gy, block, lds, cap in launches:
                            assert 0 <= lds <= cap and gx >= 1 and gy >= 1 and 64 <= block <= 1024, (case, kernel)
                            if kernel == SCORES:
                                assert lds == sh.scores_kernel_lds(hs, kvmul), case
                            if kernel == HEAD:
                                assert lds == sh.attn_head_smem(hs) and cap == sh.LDS_MAX, case
    # the largest softmax window (16384 positions of a longer context) stays within attn_softmax_pv_kernel's cap
    _, launches, _ = library_plan(128, 4, 200, ctx=20000, window=16384)
    (pv,) = [k for k in launches if k[0] == SOFTMAX_PV]
    assert pv[4] == (16384 + sh.PV_ROWS * 16) * 4 == 131072 and pv[4] <= pv[5]


def test_the_tensor_parallel_depth_schedules_hit_what_they_claim(pkg):
    """tests/tp_depth.py: every position a row-split rank decodes in tests/test_gpu_tp.py falls in the regime its case intends, on the rank's own
    heads_l / kv_heads_l and under the case's switches, by the library's plan and by the dispatch rule of tests/attn_shapes.py alike; the plan's last
    launch there is the kernel meant to hand xb to the peers (attn_head_kernel 0, attn_softmax_pv_kernel 3, attn_pv_kernel 6), and each of the three
    is that kernel at some position of at least three cases.  The main schedule crosses 128, 768 and PV_ROWS with steps on both sides."""
    import tp_depth as td
    producer_cases = {HEAD: set(), SOFTMAX_PV: set(), PV: set()}
    for name, case in td.CASES.items():
        c = pkg.synth.CONFIGS[case.cfg]
        assert c.n_heads % case.tp == 0 and c.n_kv_heads % case.tp == 0, name
        hs, kvmul, kv_heads_l = c.head_size, c.n_heads // c.n_kv_heads, c.n_kv_heads // case.tp
        head_kernel, attn_mid, window = td.plan_switches(case)
        pos = td.positions(case.schedule)
        assert pos == sorted(set(pos)) and case.schedule.prefill <= min(pos) and max(pos) < case.schedule.ctx, name
        assert sorted(p for lo, hi, _ in case.intent for p in range(lo, hi + 1)) == pos, name       # the intent names every position once
        for p in pos:
            want = td.intended(case, p)
            code, launches, _ = library_plan(hs, kvmul, p, head_kernel, attn_mid, ctx=case.schedule.ctx, window=window, kv_heads=kv_heads_l)
            kernels = tuple(k[0] for k in launches)
            assert REGIME_OF[kernels] == want and code == REGIME_CODE[want], (name, p, kernels)
            assert sh.decode_regime(hs, kvmul, p, head_kernel, attn_mid) == want, (name, p)
            assert kernels[-1] == td.PRODUCER[want], (name, p, kernels)
            kernel, gx, gy = launches[-1][:3]
            heads_l = kvmul * kv_heads_l
            assert (gx, gy) == {HEAD: (heads_l, 1), SOFTMAX_PV: (heads_l * (hs // 16), 1), PV: (kv_heads_l * ((kvmul + sh.PV_G - 1) // sh.PV_G) * (hs // 16), 1)}[kernel], (name, p)
            producer_cases[kernel].add(name)
        if window is not None:                                      # the windowed form: rows longer than the window
            assert min(pos) + 1 < window < max(pos) + 1 and {td.intended(case, p) for p in pos} == {"pair"}, name
    assert all(len(v) >= 3 for v in producer_cases.values()), producer_cases
    m = td.MAIN
    at = set(td.positions(m))
    assert {127, 128, 767, 768, sh.PV_ROWS - 1, sh.PV_ROWS} <= at and set(range(m.prefill, 132)) <= at and td.chunks(m) == [64, 56]
    assert set(td.BOUNDARY_ROWS) <= set(td.kv_rows(m))
    # kvMul 6: the second head quad of attn_pv_kernel holds two heads of four; one kv head per rank in two cases; four ranks once, as a child process
    q2 = pkg.synth.CONFIGS["mid-qwen2"]
    assert q2.n_heads // q2.n_kv_heads == 6 and q2.n_kv_heads // 2 == 1 and pkg.synth.CONFIGS["tiny-llama"].n_kv_heads // 2 == 1
    assert [n for n, cs in td.CASES.items() if cs.tp > 2] == [n for n, cs in td.CASES.items() if cs.child] == ["mid-llama-q8-tp4"]
    assert {(cs.cfg, cs.wtype) for cs in td.CASES.values()} >= {("tiny-llama", 8), ("mid-llama", 8), ("mid-qwen3", 8), ("mid-qwen2", 8), ("mid-llama", 2), ("mid-llama", 1)}
    assert [n for n, cs in td.CASES.items() if cs.fold[0] == 0] == ["tiny-llama-gather"] and td.CASES["tiny-llama-gather"].schedule == td.CASES["tiny-llama-q8"].schedule
