"""pp512 and static-batched decode of a Qwen1.5-MoE-A2.7B-shaped random-weight model (GL3_ARCH_QWEN2MOE, Q8_0) on one MI355X.

The reference's LlamaBench protocol for pp (512 prompt tokens into an empty cache, no logits) at -b 512 and -b 64, and the tokens/s of
a static-batched decode step of 32 sequences (greedy ids only, positions 16 ..).  A library without the batched MoE block accepts
max_batch = 512 and prefills token by token, so the same command measures it (the batched-decode leg is then reported as null).
Prints one JSON line.

    python scripts/moe_pp.py [--layers 24] [--reps 5]
    python scripts/moe_pp.py --kquant-mix [--layers 24] [--reps 5]

--kquant-mix: the K-quant mix of scripts/moe_tg.py --kquant-mix, the plan converted to Q8_0 at load and the native plan
(GL3_FLAG_KQUANT_NATIVE_MOE) alternated inside every leg; the batched-decode leg also compares the ids both plans end on.
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
    ap.add_argument("--kquant-mix", action="store_true")
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

    def make(**kw):        # {name: plan}: the Q8_0 model, or with --kquant-mix the converted and the native plan of the K-quant mix
        if args.kquant_mix:
            import kquant_tg
            return kquant_tg.moe_plans(cfg, synth, hip, plan_mod, **kw)
        return {"q8_0": plan_mod.HipMasterPlan(synth.StreamModel(cfg, synth.GGML_Q8_0, synth.iter_torch(cfg, wtype=synth.GGML_Q8_0, seed=42, device="cuda")), **kw)}

    def timed(plans, run, n_tok, before=lambda plan: None):
        """1 warm-up and --reps timed runs per plan, the plans alternated -> {name: (tokens/s, samples)}"""
        samples = {k: [] for k in plans}
        for r in range(args.reps + 1):
            for k, plan in plans.items():
                before(plan)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                run(plan)
                if r:
                    samples[k].append(time.perf_counter() - t1)
        return {k: dict(tok_s=round(args.reps * n_tok / sum(v), 1), samples_tok_s=[round(n_tok / x, 1) for x in v]) for k, v in samples.items()}

    t0 = time.time()
    plans = make(prefill_batch_size=args.n_prompt)
    setup_s = time.time() - t0
    pp = {b: timed(plans, lambda plan: plan.prefill(toks, 0, batch=b), args.n_prompt, lambda plan: plan.reset_kv()) for b in (512, 64)}
    for plan in plans.values():
        plan.freeTornadoExecutionPlan()

    bd = None
    try:
        plans = make(prefill_batch_size=args.batch, n_seqs=args.batch)
    except hip.Gl3Error as e:
        if e.code != hip.E_UNSUPPORTED:
            raise
        plans = None
    if plans is not None:
        B, start = args.batch, 16
        for plan in plans.values():
            for s in range(B):
                plan.prefill_seq(s, toks[s:s + start], 0)
        order = list(range(B))
        cur = [toks[(7 * s) % len(toks)] for s in range(B)]
        ids_of = {}

        def steps(plan):
            c = list(cur)
            for i in range(args.decode_steps):
                _, ids = plan.forward_decode_batch(c, order, [start + i] * B, want_logits=False)
                c = [int(v) for v in ids]
            ids_of[id(plan)] = c
        n_tok = B * args.decode_steps
        bd = timed(plans, steps, n_tok)
        for k in bd:
            bd[k].update(sequences=B, ms_per_step=round(1e3 * n_tok / bd[k]["tok_s"] / args.decode_steps, 3))
        if args.kquant_mix:
            bd["ids_equal"] = ids_of[id(plans["converted"])] == ids_of[id(plans["native"])]
        for plan in plans.values():
            plan.freeTornadoExecutionPlan()
    one = None if args.kquant_mix else "q8_0"      # one plan: the figures themselves, as before; two: {plan: figures}
    pick = lambda d: d if d is None or one is None else d[one]
    print(json.dumps(dict(metric="pp%d tokens/s" % args.n_prompt, value=pp[512]["native" if args.kquant_mix else "q8_0"]["tok_s"], unit="tokens/s", n_gpus=1,
                          reps=args.reps, dtype="i8", data="synthetic",
                          config=dict(workload="Qwen1.5-MoE-A2.7B shape, %s, %d layers, 60 experts top-4, random weights"
                                      % ("K-quant mix, converted against native" if args.kquant_mix else "Q8_0", cfg.n_layers)),
                          pp_b512=pick(pp[512]), pp_b64=pick(pp[64]), batched_decode=pick(bd), setup_s=round(setup_s, 1))))


if __name__ == "__main__":
    main()
