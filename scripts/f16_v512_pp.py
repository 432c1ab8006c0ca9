"""pp512 and static-batched decode of a Llama-3.2-1B-shaped random-weight F16 model on one MI355X, for the 512-bit and the 256-bit
species (GL3_FLAG_VECTOR_512 set / clear) in the same run.

The reference's LlamaBench protocol for pp (512 prompt tokens into an empty cache, no logits) at -b 512 and -b 64, and the tokens/s of
a static-batched decode step of 32 sequences (greedy ids only, positions 16 ..).  A library without the batched state for the 512-bit
species accepts max_batch = 512 and prefills token by token, so the same command measures it (the batched-decode leg is then null).
Prints one JSON line and, with --out, writes it to a file.

    python scripts/f16_v512_pp.py [--layers 16] [--reps 5] [--out profiles/f16_v512_batched.json] [--species 512]

--species 512|256 with --reps 1 --only pp512|bd runs one leg alone: the target of a rocprofv3 --kernel-trace --stats run."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-prompt", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32, help="sequences of the static-batched decode step")
    ap.add_argument("--decode-steps", type=int, default=32)
    ap.add_argument("--species", type=int, nargs="*", default=[512, 256], choices=[256, 512])
    ap.add_argument("--only", choices=["pp512", "pp64", "bd"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    from importlib import import_module
    pkg = ge.load_package()
    synth = pkg.synth
    plan_mod, hip = import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")
    cfg = synth.CONFIGS["llama-3.2-1b"]
    cfg = synth.ModelConfig(**{**cfg.__dict__, "ctx": args.n_prompt + 8, "n_layers": args.layers})
    toks = pkg.javarand.bench_tokens(cfg.vocab, args.n_prompt)

    def model():
        return synth.StreamModel(cfg, synth.GGML_F16, synth.iter_torch(cfg, wtype=synth.GGML_F16, seed=42, device="cuda"))

    def measure(bits):
        flags = hip.FLAG_VECTOR_512 if bits == 512 else 0
        pp = {}
        batches = [b for b in (512, 64) if args.only in (None, "pp%d" % b)]
        if batches:
            plan = plan_mod.HipMasterPlan(model(), prefill_batch_size=args.n_prompt, flags=flags)
            for b in batches:
                plan.prefill(toks, 0, batch=b)                           # warm-up (and graph / buffer set-up)
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
        plan = None
        if args.only in (None, "bd"):
            plan = plan_mod.HipMasterPlan(model(), prefill_batch_size=args.batch, n_seqs=args.batch, flags=flags)
        if plan is not None:
            B, start = args.batch, 16
            order = list(range(B))
            cur = [toks[(7 * s) % len(toks)] for s in range(B)]
            try:
                for s in range(B):
                    plan.prefill_seq(s, toks[s:s + start], 0)
                plan.forward_decode_batch(cur, order, [start] * B, want_logits=False)
            except hip.Gl3Error as e:                                    # a library without the batched state for this species
                if e.code != hip.E_UNSUPPORTED:
                    raise
                plan.freeTornadoExecutionPlan()
                plan = None
        if plan is not None:
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
        return dict(pp_b512=pp.get(512), pp_b64=pp.get(64), batched_decode=bd)

    res = {"species_%d" % bits: measure(bits) for bits in args.species}
    ratio = None
    a, b = res.get("species_512"), res.get("species_256")
    if a and b and a["pp_b512"] and b["pp_b512"]:
        ratio = round(a["pp_b512"]["tok_s"] / b["pp_b512"]["tok_s"], 3)
    first = res["species_%d" % args.species[0]]
    line = json.dumps(dict(metric="pp%d tokens/s" % args.n_prompt, value=(first["pp_b512"] or {}).get("tok_s"), unit="tokens/s", n_gpus=1, reps=args.reps,
                           dtype="f16", data="synthetic",
                           config=dict(workload="Llama-3.2-1B shape, F16, %d layers, random weights" % cfg.n_layers),
                           pp512_species_512_over_256=ratio, **res))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
