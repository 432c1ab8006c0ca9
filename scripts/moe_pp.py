"""pp512 and static-batched decode of a Qwen1.5-MoE-A2.7B-shaped random-weight model (GL3_ARCH_QWEN2MOE, Q8_0) on one MI355X.

The reference's LlamaBench protocol for pp (512 prompt tokens into an empty cache, no logits) at -b 512 and -b 64, and the tokens/s of
a static-batched decode step of 32 sequences (greedy ids only, positions 16 ..).  A library without the batched MoE block accepts
max_batch = 512 and prefills token by token, so the same command measures it (the batched-decode leg is then reported as null).
Prints one JSON line.

    python scripts/moe_pp.py [--layers 24] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-prompt", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32, help="sequences of the static-batched decode step")
    ap.add_argument("--decode-steps", type=int, default=32)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    from importlib import import_module
    pkg = ge.load_package()
    synth = pkg.synth
    plan_mod, hip = import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")
    cfg = synth.CONFIGS["qwen1.5-moe-a2.7b"]
    cfg = synth.ModelConfig(**{**cfg.__dict__, "ctx": args.n_prompt + 8, "n_layers": args.layers})
    toks = pkg.javarand.bench_tokens(cfg.vocab, args.n_prompt)

    def model():
        return synth.StreamModel(cfg, synth.GGML_Q8_0, synth.iter_torch(cfg, wtype=synth.GGML_Q8_0, seed=42, device="cuda"))

    t0 = time.time()
    plan = plan_mod.HipMasterPlan(model(), prefill_batch_size=args.n_prompt)
    setup_s = time.time() - t0
    pp = {}
    for b in (512, 64):
        plan.prefill(toks, 0, batch=b)                               # warm-up (and graph / buffer set-up)
        samples = []
        for _ in range(args.reps):
            plan.reset_kv()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            plan.prefill(toks, 0, batch=b)
            samples.append(time.perf_counter() - t1)
        pp[b] = dict(tok_s=round(args.reps * args.n_prompt / sum(samples), 1), samples_tok_s=[round(args.n_prompt / s, 1) for s in samples])
    plan.freeTornadoExecutionPlan()

    bd = None
    try:
        plan = plan_mod.HipMasterPlan(model(), prefill_batch_size=args.batch, n_seqs=args.batch)
    except hip.Gl3Error as e:
        if e.code != hip.E_UNSUPPORTED:
            raise
        plan = None
    if plan is not None:
        B, start = args.batch, 16
        for s in range(B):
            plan.prefill_seq(s, toks[s:s + start], 0)
        order = list(range(B))
        cur = [toks[(7 * s) % len(toks)] for s in range(B)]

        def steps(pos0):
            c = list(cur)
            for i in range(args.decode_steps):
                _, ids = plan.forward_decode_batch(c, order, [pos0 + i] * B, want_logits=False)
                c = [int(v) for v in ids]
        steps(start)
        samples = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            steps(start)
            samples.append(time.perf_counter() - t1)
        n_tok = B * args.decode_steps
        bd = dict(sequences=B, tok_s=round(args.reps * n_tok / sum(samples), 1), samples_tok_s=[round(n_tok / s, 1) for s in samples],
                  ms_per_step=round(1e3 * sum(samples) / (args.reps * args.decode_steps), 3))
        plan.freeTornadoExecutionPlan()
    print(json.dumps(dict(metric="pp%d tokens/s" % args.n_prompt, value=pp[512]["tok_s"], unit="tokens/s", n_gpus=1, reps=args.reps, dtype="i8",
                          data="synthetic",
                          config=dict(workload="Qwen1.5-MoE-A2.7B shape, Q8_0, %d layers, 60 experts top-4, random weights" % cfg.n_layers),
                          pp_b512=pp[512], pp_b64=pp[64], batched_decode=bd, setup_s=round(setup_s, 1))))


if __name__ == "__main__":
    main()
