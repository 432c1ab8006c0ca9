"""The schedules at which tests/test_gpu_tp.py takes row-split ranks to depth, and what every schedule is meant to run: the decode attention
regime of each position and the kernel that hands xb to the peers there.  Under folded gathers (plan.tp_fold_mode() == (1, 0)) that kernel stores
xb into every peer's arena and publishes the flag itself; gl3_decode_attn.h has that epilogue three times (attn_head_kernel,
attn_softmax_pv_kernel, attn_pv_kernel).  tests/test_attn_shapes.py holds the intent below equal to the library's own plan and to the dispatch
rule of tests/attn_shapes.py without a GPU; tests/test_gpu_tp.py runs the schedules.

A schedule: batched prefill of `prefill` tokens from position 0 in chunks of `batch`, then stretches (first, last) of single-token decode steps.
Between the stretches the KV cache holds rows that neither side wrote: zeros in the plan and in the oracle alike.  The token at position p is
javarand.bench_tokens(vocab, ctx)[p] on both sides."""
from collections import namedtuple

CTX = 1300
BOUNDARY_ROWS = (127, 128, 767, 768, 1024)      # K / V rows compared where a schedule decodes them: both sides of every hand-over, the first row of the second V slab

Schedule = namedtuple("Schedule", "ctx batch prefill stretches")
# across AF_MAXN = 128 on a fully real cache, across ATTN_MID_DEFAULT = 768, across PV_ROWS = 1024 (a second V slab and tile)
MAIN = Schedule(CTX, 64, 120, ((120, 131), (764, 771), (1022, 1026)))


def main_intent(long_form):
    return ((120, 127, "head"), (128, 131, "pair"), (764, 767, "pair"), (768, 771, long_form), (1022, 1026, long_form))


# cfg: synth config; wtype: ggml type (8 Q8_0, 2 Q4_0, 1 F16); no_graph: GL3_FLAG_NO_GRAPH; env: set around plan creation (in the child's environment
# for child = True: tp ranks as threads of a fresh process, scripts/debug_tp_fold.py); fold: the tp_fold_mode() every rank must report;
# intent: (first, last, regime in the names of attn_shapes.decode_regime) over every scheduled position
Case = namedtuple("Case", "cfg wtype tp no_graph env child fold schedule intent")
CASES = {
    # head size 32: the one-tile scores kernel in the long regime; one kv head per rank
    "tiny-llama-q8":      Case("tiny-llama", 8, 2, False, {}, False, (1, 0), MAIN, main_intent("long-tile")),
    # head size 64: looping scores kernel, four kv heads per rank
    "mid-llama-q8":       Case("mid-llama", 8, 2, False, {}, False, (1, 0), MAIN, main_intent("long-loop")),
    # head size 128, q / k norm
    "mid-qwen3-q8":       Case("mid-qwen3", 8, 2, False, {}, False, (1, 0), MAIN, main_intent("long-loop")),
    # kvMul 6: two head quads in attn_pv_kernel, whose second quad stores for two of its four heads and publishes all the same; bias; one kv head per rank
    "mid-qwen2-q8":       Case("mid-qwen2", 8, 2, False, {}, False, (1, 0), MAIN, main_intent("long-tile")),
    # vector-order producers
    "mid-llama-q4":       Case("mid-llama", 2, 2, False, {}, False, (1, 0), MAIN, main_intent("long-loop")),
    "mid-llama-f16":      Case("mid-llama", 1, 2, False, {}, False, (1, 0), MAIN, main_intent("long-loop")),
    # the same regimes launched eagerly
    "mid-llama-q8-eager": Case("mid-llama", 8, 2, True, {}, False, (1, 0), MAIN, main_intent("long-loop")),
    # four ranks share the GPU: consumers wait in their own prologue, every matvec capped at 16 workgroups
    "mid-llama-q8-tp4":   Case("mid-llama", 8, 4, False, {"GL3_TP_FOLD": "2", "GL3_WGS": "16"}, True, (1, 31), MAIN, main_intent("long-loop")),
    # attn_softmax_pv_kernel pushes from position 0
    "tiny-llama-nofused": Case("tiny-llama", 8, 2, False, {"GL3_NO_FUSED_ATTN": "1"}, False, (1, 0),
                               Schedule(CTX, 64, 0, ((0, 5), (126, 130))), ((0, 5, "pair"), (126, 130, "pair"))),
    # softmax rows longer than the LDS window run in windows, under the fold
    "tiny-llama-window":  Case("tiny-llama", 8, 2, False, {"GL3_ATTN_MID": "4096", "GL3_ATTN_WINDOW": "1024"}, False, (1, 0),
                               Schedule(CTX, 64, 120, ((1022, 1026), (1100, 1102))), ((1022, 1026, "pair"), (1100, 1102, "pair"))),
    # the long path right behind 128
    "tiny-llama-mid0":    Case("tiny-llama", 8, 2, False, {"GL3_ATTN_MID": "0"}, False, (1, 0),
                               Schedule(CTX, 64, 120, ((126, 131),)), ((126, 127, "head"), (128, 131, "long-tile"))),
    # the control: gather launches, same schedule and answers as tiny-llama-q8
    "tiny-llama-gather":  Case("tiny-llama", 8, 2, False, {"GL3_TP_FOLD": "0"}, False, (0, 0), MAIN, main_intent("long-tile")),
}

PRODUCER = {"head": 0, "pair": 3, "long-loop": 6, "long-tile": 6}      # the last launch of the regime, in gl3_debug_decode_attn_plan's numbering


def positions(schedule):
    return [p for lo, hi in schedule.stretches for p in range(lo, hi + 1)]


def chunks(schedule):
    return [min(schedule.batch, schedule.prefill - p) for p in range(0, schedule.prefill, schedule.batch)]


def kv_rows(schedule):
    """rows compared after the walk: the boundary rows the schedule decodes, the ends of every stretch, the ends of the prompt"""
    pos = positions(schedule)
    rows = {p for p in BOUNDARY_ROWS if p in pos} | {p for s in schedule.stretches for p in s}
    if schedule.prefill:
        rows |= {0, schedule.prefill - 1}
    return sorted(rows)


def intended(case, pos):
    (regime,) = [name for lo, hi, name in case.intent if lo <= pos <= hi]
    return regime


def plan_switches(case):
    """(attn_head_kernel allowed, attn_mid, softmax window or None) as gl3_create reads them from the case's environment"""
    env = case.env
    return env.get("GL3_NO_FUSED_ATTN") != "1", int(env.get("GL3_ATTN_MID", 768)), int(env["GL3_ATTN_WINDOW"]) if "GL3_ATTN_WINDOW" in env else None


def schedule_arg(schedule):
    """the schedule argument of scripts/debug_tp_fold.py"""
    return "ctx=%d;batch=%d;prefill=%d;decode=%s;kv=%s" % (schedule.ctx, schedule.batch, schedule.prefill, ",".join("%d-%d" % s for s in schedule.stretches),
                                                         ",".join(map(str, kv_rows(schedule))))
