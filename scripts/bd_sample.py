"""Static batched decode with the sampler on the device against the greedy step and the logits copy:
python scripts/bd_sample.py [model] [B] [steps] [reps] [only]

ms per step (min / median / max over `reps` repetitions of `steps` timed steps, each repetition ended by one device
synchronisation) of
  (a) forward_decode_batch(want_logits=False)       greedy ids sampled on the device
  (b) forward_decode_batch(want_logits=True)        all logits to the host: what a non-greedy batch costs without the batched
                                                    sampler, the copy only (no host softmax, no heap): a lower bound
  (c) forward_decode_batch_sample, every row (0.7, 0.95)    top-p
  (d) forward_decode_batch_sample, every row (1.0, 0)       categorical
and, on the single-row entry of the same plan at positions 0 .. steps - 1, of
  (e) forward_decode                                 greedy id
  (f) forward_decode_sample (0.7, 0.95)              top-p
  (g) forward_decode_sample (1.0, 0)                 categorical
The seven lines alternate inside every repetition, so they share whatever else the machine is doing.  `only` = a | b | .. | g runs
one line alone (for a kernel trace)."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import __graft_entry__ as ge
pkg = ge.load_package()
from importlib import import_module
plan_mod = import_module(ge.PKG_NAME + ".plan")
name = sys.argv[1] if len(sys.argv) > 1 else "qwen3-4b"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
n = int(sys.argv[3]) if len(sys.argv) > 3 else 32
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
only = sys.argv[5] if len(sys.argv) > 5 else ""
base = pkg.synth.CONFIGS[name]
cfg = pkg.synth.ModelConfig(**{**base.__dict__, "ctx": 136})
m = pkg.synth.StreamModel(cfg, 8, pkg.synth.iter_torch(cfg, seed=1, device="cuda"))
plan = plan_mod.HipMasterPlan.initializeTornadoVMPlan(m, prefill_batch_size=B, n_seqs=B)
toks = np.asarray(pkg.javarand.bench_tokens(cfg.vocab, n * B), np.int32).reshape(n, B)
seqs = np.arange(B, dtype=np.int32)
rng = pkg.javarand.L32X64MixRandom(1234)
coins = np.asarray([rng.next_float() for _ in range(n * B)], np.float32).reshape(n, B)
temp_c, topp_c = np.full(B, 0.7, np.float32), np.full(B, 0.95, np.float32)
temp_d, topp_d = np.full(B, 1.0, np.float32), np.zeros(B, np.float32)
poss = [np.full(B, i, np.int32) for i in range(n)]
lines = {
    "a": ("greedy ids on the device", lambda i: plan.forward_decode_batch(toks[i], seqs, poss[i], want_logits=False)),
    "b": ("all logits to the host", lambda i: plan.forward_decode_batch(toks[i], seqs, poss[i], want_logits=True)),
    "c": ("sampled on the device, top-p (0.7, 0.95)", lambda i: plan.forward_decode_batch_sample(toks[i], seqs, poss[i], temp_c, topp_c, coins[i])),
    "d": ("sampled on the device, categorical (1.0, 0)", lambda i: plan.forward_decode_batch_sample(toks[i], seqs, poss[i], temp_d, topp_d, coins[i])),
    "e": ("single row, greedy id", lambda i: plan.forward_decode_argmax(int(toks[i, 0]), i)),
    "f": ("single row, top-p (0.7, 0.95)", lambda i: plan.forward_decode_sample(int(toks[i, 0]), i, 0.7, 0.95, float(coins[i, 0]))),
    "g": ("single row, categorical (1.0, 0)", lambda i: plan.forward_decode_sample(int(toks[i, 0]), i, 1.0, 0.0, float(coins[i, 0]))),
}
keys = [only] if only else list(lines)
ms = {k: [] for k in keys}
each = {k: [] for k in keys}          # every timed step on its own: a top-p step that met a tie (host heap) stands out
for rep in range(reps + 1):                      # repetition 0 warms every line up (graph capture, buffer growth) and is not kept
    for k in keys:
        step = lines[k][1]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            t1 = time.perf_counter()
            step(i)                                  # returns after its own device synchronisation
            if rep:
                each[k].append((time.perf_counter() - t1) * 1e3)
        torch.cuda.synchronize()
        if rep:
            ms[k].append((time.perf_counter() - t0) / n * 1e3)
print("batched decode %s B=%d, %d steps x %d repetitions, ms per step: min / median / max" % (name, B, n, reps))
for k in keys:
    v = sorted(ms[k])
    e = sorted(each[k])
    print("(%s) %-46s %.3f / %.3f / %.3f   single steps: median %.3f, max %.3f, %d of %d above 1.5 x median" %
          (k, lines[k][0], v[0], v[len(v) // 2], v[-1], e[len(e) // 2], e[-1], sum(x > 1.5 * e[len(e) // 2] for x in e), len(e)))
if not only:
    med = {k: sorted(ms[k])[len(ms[k]) // 2] for k in keys}
    print("sampler cost per step: (c) - (a) = %.3f ms, (d) - (a) = %.3f ms; logits copy: (b) - (a) = %.3f ms" % (med["c"] - med["a"], med["d"] - med["a"], med["b"] - med["a"]))
    print("single-row sampler cost per step: (f) - (e) = %.3f ms, (g) - (e) = %.3f ms" % (med["f"] - med["e"], med["g"] - med["e"]))
    dev, host = plan.topp_counts()
    print("top-p draws answered on the device / by the host heap: %d / %d" % (dev, host))
