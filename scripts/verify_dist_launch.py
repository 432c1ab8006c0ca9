"""The decision launch with and without draft distributions on the same rows (profiles/spec_draft.md), for a kernel trace of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/verify_dist_launch.py [--vocab 128256] [--rows 8] [--iters 10]

A tiny model with the 1B / 8B vocabulary, one run of --rows rows on random logits (the taps gl3_verify_rows / gl3_verify_rows_dist: no forward
pass).  Two shapes of a run, each --iters times through both kernels: every draft accepted (every row examined once: maximum + numerators,
the last row emits) and a rejection at row 0 (one row examined, then its residual: all chunks and the hit chunk once more).  The trace
lists verify_runs_kernel<false> and verify_runs_kernel<true>; the q read is the difference."""
import argparse
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    pkg = ge.load_package()
    from importlib import import_module
    plan_mod = import_module(ge.PKG_NAME + ".plan")
    V, m, F32 = args.vocab, args.rows, np.float32
    model = pkg.synth.make_numpy(dataclasses.replace(pkg.synth.CONFIGS["tiny-llama"], vocab=V), seed=5)
    plan = plan_mod.HipMasterPlan(model, prefill_batch_size=max(16, m))
    rng = np.random.default_rng(1)
    lg = (rng.standard_normal((m, V)) * 3).astype(F32)
    tokens = [3] + [int(np.argmax(r)) for r in lg[:-1]]                  # the likeliest token of every row: accepted by the coin 0
    for s in range(m - 1):
        e = np.exp(rng.standard_normal(V) * 3)
        plan.draft_probs_put_host(s, (e / e.sum()).astype(F32))
    slots = list(range(m - 1)) + [-1]
    top = float(F32(1.0) - F32(2.0) ** -24)
    accept_all = np.tile(np.asarray([[0.0, 0.5]], F32), (m, 1))
    reject_0 = accept_all.copy()
    reject_0[0, 0] = top
    worst = [3, int(np.argmin(lg[0]))] + tokens[2:]                     # p[d] tiny: rejected by the largest coin under both rules
    for what, toks, coins in (("all accepted", tokens, accept_all), ("rejection at row 0", worst, reject_0)):
        for _ in range(args.iters):
            a = plan.verify_rows(lg, toks, [m], [0.8], coins)
            b = plan.verify_rows_dist(lg, toks, [m], [0.8], coins, slots)
        print(what, "one-hot", a.tolist(), "dist", b.tolist(), flush=True)
    plan.freeTornadoExecutionPlan()


if __name__ == "__main__":
    main()
