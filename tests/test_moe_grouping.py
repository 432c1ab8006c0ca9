"""CPU mirror of moe_group_kernel (gl3_moe_kernels.h): the (token, choice) assignments of a batched Qwen2-MoE step sorted by expert, and
the tile table the grouped expert GEMMs (bdw_gemm_kernel<.., GRP>) walk on a grid sized from the token count alone.

The mirror keeps the kernel's structure: a wavefront owns one expert at a time and walks the assignments 64 per trip; the ballot of the
matches counts them in the first pass and ranks them in the second; one thread scans the counts in between.

This file proves the algorithm and the grid bound on a restatement; it cannot see the HIP code diverge from it.  What binds the mirror to
the kernel are the GPU tests of tests/test_gpu_moe_batched.py: a slot in the wrong entry, a missing slot or a wrong scatter row there
changes x of some row, which they compare bit for bit with the oracle.
"""
import random

import pytest

import moe_shapes as ms

WAVE = 64
# every case of the configuration grid (tests/moe_shapes.py) at one token, past the 16-token tile and on the > 64-token path
GRID_SHAPES = sorted({(n, topk, experts) for experts, topk, _, _, _ in ms.GRID.values() for n in (1, 17, 65)})


def max_entries(n, topk, n_experts):
    """moe_group_max_entries: the grid bound."""
    s = n * topk
    return min(n_experts, s) + s // 16


def group(sel, n, topk, n_experts):
    """sel: [n * topk] expert ids, token-major.  Returns (slot_tok, slot_dst, entries) as the kernel writes them."""
    S = n * topk
    cnt = [0] * n_experts
    for e in range(n_experts):                                      # pass 1
        for i0 in range(0, S, WAVE):
            ballot = [i0 + lane < S and sel[i0 + lane] == e for lane in range(WAVE)]
            cnt[e] += sum(ballot)
    start, tstart, s, u = [], [], 0, 0
    for e in range(n_experts):                                      # the scan of thread 0
        start.append(s)
        tstart.append(u)
        s += cnt[e]
        u += (cnt[e] + 15) >> 4
    slot_tok, slot_dst, entries = [None] * S, [None] * S, [None] * u
    for e in range(n_experts):                                      # pass 2
        at = start[e]
        for i0 in range(0, S, WAVE):
            ballot = [i0 + lane < S and sel[i0 + lane] == e for lane in range(WAVE)]
            for lane in range(WAVE):
                if ballot[lane]:
                    i = i0 + lane
                    pos = at + sum(ballot[:lane])
                    tok = i // topk
                    assert slot_tok[pos] is None
                    slot_tok[pos] = tok
                    slot_dst[pos] = tok * (topk + 1) + (i - tok * topk)
            at += sum(ballot)
        j = 0
        while 16 * j < cnt[e]:
            assert entries[tstart[e] + j] is None
            entries[tstart[e] + j] = (e, start[e] + 16 * j, min(16, cnt[e] - 16 * j))
            j += 1
    return slot_tok, slot_dst, entries


def check(sel, n, topk, n_experts):
    slot_tok, slot_dst, entries = group(sel, n, topk, n_experts)
    S = n * topk
    assert len(entries) <= max_entries(n, topk, n_experts)          # the launch's grid covers the table
    assert all(en is not None for en in entries)
    seen = []
    prev_expert = -1
    for e, first, valid in entries:
        assert 1 <= valid <= 16 and 0 <= first and first + valid <= S
        assert e >= prev_expert                                     # an expert's entries are consecutive
        prev_expert = e
        for slot in range(first, first + valid):
            tok, dst = slot_tok[slot], slot_dst[slot]
            choice = dst - tok * (topk + 1)
            assert 0 <= tok < n and 0 <= choice < topk
            assert sel[tok * topk + choice] == e                    # entries never mix experts
            seen.append((tok, choice))
    assert sorted(seen) == [(t, c) for t in range(n) for c in range(topk)]      # every assignment in exactly one entry
    assert len(seen) == S
    # stable: inside an expert the slots ascend in (token, choice), so a run is reproducible
    for e in range(n_experts):
        mine = [(slot_tok[s], slot_dst[s]) for s in range(S) if sel[slot_tok[s] * topk + slot_dst[s] - slot_tok[s] * (topk + 1)] == e]
        assert mine == sorted(mine)
    return entries


def random_routing(rng, n, topk, n_experts):
    sel = []
    for _ in range(n):
        sel.extend(rng.sample(range(n_experts), topk))              # a token's choices are distinct experts
    return sel


RANDOM_SHAPES = [(1, 2, 8), (1, 4, 60), (3, 2, 8), (17, 2, 8), (96, 2, 8), (5, 4, 60), (32, 4, 60), (80, 4, 60), (512, 4, 60), (64, 1, 3), (33, 8, 8),
                 (20, 6, 4096)]
RANDOM_SHAPES += [s for s in GRID_SHAPES if s not in RANDOM_SHAPES]      # (1, 2, 8) and (17, 2, 8) are grid shapes already


@pytest.mark.parametrize("n,topk,n_experts", RANDOM_SHAPES)
def test_random_routings(n, topk, n_experts):
    rng = random.Random(1000 * n + topk)
    for _ in range(3):
        check(random_routing(rng, n, topk, n_experts), n, topk, n_experts)


@pytest.mark.parametrize("n,topk,n_experts", [(1, 1, 8), (40, 1, 8), (16, 1, 60), (512, 1, 60), (23, 2, 8)] + GRID_SHAPES)
def test_all_tokens_on_one_expert(n, topk, n_experts):
    """Every token's first choice is one expert — 5, or the last one where there are fewer (the grid's 1-expert case) — and the other choices,
    if any, spread: that expert owns ceil(n / 16) entries."""
    rng = random.Random(n)
    hot = min(5, n_experts - 1)
    sel = []
    for _ in range(n):
        sel.extend([hot] + rng.sample([e for e in range(n_experts) if e != hot], topk - 1))
    entries = check(sel, n, topk, n_experts)
    assert sum(1 for e, _, _ in entries if e == hot) == (n + 15) // 16


def test_the_grid_shapes_are_in_the_lists():
    assert set(GRID_SHAPES) <= set(RANDOM_SHAPES) and len(set(RANDOM_SHAPES)) == len(RANDOM_SHAPES)
    assert len(GRID_SHAPES) == 3 * 8 and (65, 64, 64) in GRID_SHAPES and (17, 6, 130) in GRID_SHAPES and (1, 1, 1) in GRID_SHAPES      # 8 / 2 twice in the grid


def test_fewer_assignments_than_experts():
    n, topk, E = 3, 2, 60
    entries = check([7, 59, 0, 7, 58, 59], n, topk, E)
    assert len(entries) == 4 <= max_entries(n, topk, E) == 6       # min(E, n topk) is the binding term
    assert [e for e, _, _ in entries] == [0, 7, 58, 59]


@pytest.mark.parametrize("per_expert", [16, 32, 48])
def test_counts_that_are_exact_multiples_of_16(per_expert):
    """Every expert holds a whole number of full entries: no ragged entry, and the bound's n topk / 16 term is reached exactly."""
    E, topk = 8, 2
    n = per_expert * E // topk
    sel = []
    for t in range(n):
        sel.extend([(2 * t) % E, (2 * t + 1) % E])
    entries = check(sel, n, topk, E)
    assert all(valid == 16 for _, _, valid in entries) and len(entries) == n * topk // 16


def test_worst_case_reaches_the_bound():
    """One assignment over a multiple of 16 on as many experts as possible: a ragged entry per expert + the full ones."""
    E, topk, n = 4, 1, 68                                           # 17 per expert: 4 ragged + 4 full = min(E, S) + S / 16
    sel = [t % E for t in range(n)]
    entries = check(sel, n, topk, E)
    assert len(entries) == max_entries(n, topk, E) == 8
