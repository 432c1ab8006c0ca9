"""The mixed batched step against today's two calls, on a Qwen3-4B-shaped random-weight Q8_0 model on one MI355X (max_batch 128).

    (a)  31 decode rows at depth 64 + one 96-token prompt run as ONE gl3_forward_batch (127 rows; output rows: the 31 decode rows)
    (b)  the same work as the two existing calls: gl3_forward_decode_batch of 31 + gl3_forward_prefill_seq of 96
    (c)  (a) with the decode rows at depth 600: the deepest row's score rows do not fit LDS, the step takes the per-row attention pair
    (d)  (b) at depth 600, the yardstick of (c)

The variants of a depth alternate in one process after a warm-up of each; a sample is `--inner` calls in a row, each ending in the
library's own stream synchronise (host clock).  Every call forwards the same tokens at the same positions, so the KV rows it writes
are rewritten with the same values and the cases do not disturb each other.  Prints one JSON line (min / median / max per case in ms
per step) and, with --out, writes it to a file.

    python scripts/mixed_step.py [--layers 36] [--reps 7] [--inner 5] [--out profiles/mixed_step.json]

--only a|b|c|d with --reps 1 --inner 1 runs one variant alone behind its warm-up: the target of a rocprofv3 --kernel-trace --stats
run (launch counts)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--decode-rows", type=int, default=31)
    ap.add_argument("--prompt", type=int, default=96)
    ap.add_argument("--only", choices=["a", "b", "c", "d"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    from importlib import import_module
    pkg = ge.load_package()
    synth = pkg.synth
    plan_mod = import_module(ge.PKG_NAME + ".plan")
    cfg = synth.CONFIGS["qwen3-4b"]
    cfg = synth.ModelConfig(**{**cfg.__dict__, "n_layers": args.layers})
    D, P = args.decode_rows, args.prompt
    shallow, deep = 64, 600
    assert deep + 1 <= cfg.ctx and D + P <= 128
    toks = pkg.javarand.bench_tokens(cfg.vocab, deep + P + D)
    plan = plan_mod.HipMasterPlan(synth.StreamModel(cfg, synth.GGML_Q8_0, synth.iter_torch(cfg, wtype=synth.GGML_Q8_0, seed=42, device="cuda")),
                                  prefill_batch_size=128, n_seqs=D + 1)
    dec_tok = [toks[(7 * s) % len(toks)] for s in range(D)]
    prompt = toks[deep:deep + P]
    seqs = list(range(D))

    def variants(depth):
        rows_t, rows_s, rows_p = dec_tok + prompt, seqs + [D] * P, [depth] * D + list(range(P))
        want = [1] * D + [0] * P

        def mixed():
            plan.forward_batch(rows_t, rows_s, rows_p, want_logits=want, logits=False)

        def two_calls():
            plan.forward_decode_batch(dec_tok, seqs, [depth] * D, want_logits=False)
            plan.prefill_seq(D, prompt, 0)
        return mixed, two_calls

    def measure(cases):
        """cases: {name: callable}; alternating samples after one warm-up call of each"""
        for f in cases.values():
            f()
        samples = {k: [] for k in cases}
        for _ in range(args.reps):
            for k, f in cases.items():
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(args.inner):
                    f()
                samples[k].append(1e3 * (time.perf_counter() - t1) / args.inner)
        return {k: dict(min_ms=round(min(v), 3), median_ms=round(statistics.median(v), 3), max_ms=round(max(v), 3), samples_ms=[round(x, 3) for x in v])
                for k, v in samples.items()}

    res = {}
    for s in seqs:
        plan.prefill_seq(s, toks[s:s + shallow], 0)
    a, b = variants(shallow)
    pick = {k: f for k, f in (("a", a), ("b", b)) if args.only in (None, k)}
    if pick:
        res.update(measure(pick))
    if args.only in (None, "c", "d"):
        for s in seqs:
            plan.prefill_seq(s, toks[s + shallow:s + deep], shallow)
        c, d = variants(deep)
        res.update(measure({k: f for k, f in (("c", c), ("d", d)) if args.only in (None, k)}))
    plan.freeTornadoExecutionPlan()
    ratio = lambda x, y: round(res[x]["median_ms"] / res[y]["median_ms"], 3) if x in res and y in res else None
    line = json.dumps(dict(metric="mixed step, ms per step (median)", value=(res.get("a") or next(iter(res.values())))["median_ms"], unit="ms", n_gpus=1,
                           reps=args.reps, inner=args.inner, dtype="q8_0", data="synthetic",
                           config=dict(workload="Qwen3-4B shape, Q8_0, %d layers, random weights; %d decode rows + a %d-token prompt run, max_batch 128"
                                       % (cfg.n_layers, D, P), depth_a_b=shallow, depth_c_d=deep),
                           a_over_b=ratio("a", "b"), c_over_d=ratio("c", "d"), **res))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
