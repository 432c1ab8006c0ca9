"""Sampler-alone and tg128 drivers for profiles/topk_sample.md.
    python scripts/topk_sample.py rows VOCAB N topp|topk [STEPS]   # STEPS sampler calls on N rows of seeded logits (run under rocprofv3
                                                                   # --kernel-trace --stats: device time and launches per step)
    python scripts/topk_sample.py table DIR                        # the table from DIR/<vocab>_<n>_<path>/**/*kernel_stats.csv
    python scripts/topk_sample.py tg MODEL LAYERS [TOKENS]         # wall clock per token: greedy, gl3_forward_decode_sample (top-p 0.9),
                                                                   # gl3_forward_decode_sample_topk (k 40, top-p 0.9, min-p 0.05)"""
import csv, dataclasses, glob, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SAMPLER = ("bsm_", "btp_", "topk_sample")      # the sampler's own kernels; the greedy scan and the logits upload belong to the tap, not to it


def plan_of():
    import __graft_entry__ as ge
    from importlib import import_module
    pkg = ge.load_package()
    return pkg, import_module(ge.PKG_NAME + ".plan")


if sys.argv[1] == "rows":
    V, n, path, steps = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], int(sys.argv[5]) if len(sys.argv) > 5 else 50
    pkg, plan_mod = plan_of()
    m = pkg.synth.make_numpy(dataclasses.replace(pkg.synth.CONFIGS["tiny-llama"], vocab=V), seed=5)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64)
    rng = np.random.default_rng(V + n)
    lg = (rng.standard_normal((n, V)) * 3.0).astype(np.float32)
    for s in range(steps):
        coins = rng.random(n).astype(np.float32) * np.float32(0.999)
        if path == "topk":
            plan.sample_rows_topk(lg, 40, 0.8, 0.9, 0.05, coins)
        else:
            plan.sample_rows(lg, 0.8, 0.9, coins)
    print("done", V, n, path, steps)
elif sys.argv[1] == "table":
    print("| vocab | rows | path | launches / step | device us / step |\n|---|---|---|---|---|")
    for d in sorted(glob.glob(os.path.join(sys.argv[2], "*_*_*")), key=lambda d: (int(os.path.basename(d).split("_")[0]), int(os.path.basename(d).split("_")[1]))):
        V, n, path, steps = os.path.basename(d).split("_")
        f = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not f:
            continue
        rows = [r for r in csv.DictReader(open(f[0])) if any(s in r["Name"] for s in SAMPLER)]
        calls, ns = sum(int(r["Calls"]) for r in rows), sum(int(r["TotalDurationNs"]) for r in rows)
        print("| %s | %s | %s | %.1f | %.1f |" % (V, n, path, calls / int(steps), ns / int(steps) / 1e3))
else:
    import torch
    name, nl, ntok = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 128
    pkg, plan_mod = plan_of()
    base = pkg.synth.CONFIGS[name]
    m = pkg.synth.make_torch(pkg.synth.ModelConfig(**{**base.__dict__, "n_layers": nl, "ctx": 2 * ntok + 16}), wtype=8, seed=1, device="cuda")
    plan = plan_mod.HipMasterPlan.initializeTornadoVMPlan(m)
    rng = pkg.javarand.L32X64MixRandom(1)
    steps = {"greedy": lambda t, p: plan.forward_decode_argmax(t, p),
             "top-p": lambda t, p: plan.forward_decode_sample(t, p, 0.8, 0.9, rng.next_float()),
             "top-k": lambda t, p: plan.forward_decode_sample_topk(t, p, 40, 0.8, 0.9, 0.05, rng.next_float())}
    for rep in range(3):                      # alternate the three, so drift lands on all of them
        for kind, step in steps.items():
            tok = 1
            for p in range(8):
                tok = step(tok, p)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for p in range(8, 8 + ntok):
                tok = step(tok, p)
            print("%s rep %d: %.1f us / token (%s, %d layers, vocab %d)" % (kind, rep, (time.perf_counter() - t0) / ntok * 1e6, name, nl, base.vocab))
