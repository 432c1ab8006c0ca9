"""Batched steps of a Llama-3-8B-shaped random model in the Q4_K_M mix (scripts/kquant_tg.py's model): converted to Q8_0 at load (the
default plan) against native K-quant storage with the batched entry points (GL3_FLAG_KQUANT_NATIVE_BATCH).

Three workloads, the two plans alternated inside one invocation (1 warm-up and --reps timed repetitions each), outputs compared for
equality in every repetition: a static-batched decode step at 32 sequences (16 steps per repetition, logits of every row to the host),
pp512 with 512-token chunks (kq_expand_q8t_kernel + the Q8_0 GEMMs) and pp512 with 64-token chunks (kq_gemm_kernel).  Prints one JSON line.

    python scripts/kquant_batched.py [--layers 32] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from kquant_tg import KqModel  # noqa: E402

NSEQ, PP, STEPS = 32, 512, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import __graft_entry__ as ge
    from importlib import import_module
    pkg = ge.load_package()
    synth = pkg.synth
    plan_mod, hip = import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")
    cfg = synth.CONFIGS["llama-3-8b"]
    cfg = synth.ModelConfig(**{**cfg.__dict__, "ctx": PP + STEPS + 8, "n_layers": args.layers})
    kw = dict(prefill_batch_size=PP, n_seqs=NSEQ)
    plans = {"converted": plan_mod.HipMasterPlan(KqModel(cfg, synth, hip.lib(), 42, True), **kw),
             "native": plan_mod.HipMasterPlan(KqModel(cfg, synth, hip.lib(), 42, False), flags=hip.FLAG_KQUANT_NATIVE_BATCH, **kw)}
    toks = pkg.javarand.bench_tokens(cfg.vocab, PP + STEPS)

    def decode32(plan):                                   # every sequence 8 positions deep, then STEPS timed steps
        for s in range(NSEQ):
            plan.prefill_seq(s, toks[s:s + 8])
        t1 = time.perf_counter()
        for j in range(STEPS):
            lg, ids = plan.forward_decode_batch([toks[8 + j + s] for s in range(NSEQ)], range(NSEQ), [8 + j] * NSEQ)
        return NSEQ * STEPS / (time.perf_counter() - t1), lg

    def pp(batch):
        def run(plan):
            t1 = time.perf_counter()
            plan.prefill(toks[:PP], 0, batch=batch)
            dt = time.perf_counter() - t1
            return PP / dt, np.concatenate(plan.kv(cfg.n_layers - 1, PP - 1))
        return run

    out = dict(unit="tokens/s", n_gpus=1, data="synthetic", config=dict(workload="Llama-3-8B shape, Q4_K_M mix, %d layers, random weights" % cfg.n_layers, reps=args.reps),
               weight_bytes_in_hbm={k: p.weight_bytes() for k, p in plans.items()})
    for name, fn in (("decode_b32", decode32), ("pp512_b512", pp(512)), ("pp512_b64", pp(64))):
        samples, equal = {k: [] for k in plans}, True
        for r in range(args.reps + 1):                    # repetition 0 is the warm-up
            last = {}
            for k, plan in plans.items():
                s, last[k] = fn(plan)
                if r:
                    samples[k].append(round(s, 1))
            equal = equal and bool(np.array_equal(last["converted"], last["native"]))
        out[name] = dict(outputs_equal=equal, **{k: dict(tok_s=round(float(np.mean(v)), 1), samples_tok_s=v, spread_tok_s=round(max(v) - min(v), 1))
                                                  for k, v in samples.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
