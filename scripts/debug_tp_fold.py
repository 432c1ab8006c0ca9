"""Tensor-parallel decode with folded gathers, ranks as threads of ONE fresh process, every rank's logits compared with the CPU oracle bit for bit
(used by tests/test_gpu_tp.py: a fresh process has one hardware queue per rank stream, see tests/conftest.py).
    GL3_TP_FOLD=2 [GL3_TP_FOLD_MASK=m] python scripts/debug_tp_fold.py mid-llama 4 [tokens] [ggml type: 8 Q8_0 | 2 Q4_0 | 1 F16] [schedule]
Without a schedule the ranks decode `tokens` positions from 0.  A schedule, "ctx=1300;batch=64;prefill=120;decode=120-131,764-771;kv=127,128", takes them to
depth instead (`tokens` is then unused): a context of ctx positions, batched prefill of `prefill` tokens in chunks of `batch`, single-token decode
steps over every listed stretch, the token at position p being bench_tokens(vocab, ctx)[p]; rows in between stay zero on both sides.  Beside every
step's logits the greedy id of the device at the last position of every stretch (forward_decode_argmax, the step repeated) and this rank's slice
of the K / V rows at both ends of every stretch and of the prompt, and at the positions of `kv` (optional), are compared, in every layer."""
import sys, os, threading, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "32")
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
from importlib import import_module
plan_mod = import_module(ge.PKG_NAME + ".plan"); hip = import_module(ge.PKG_NAME + ".hip")
from oracle import oracle_c as orc
orc.build()
cfg, tp = sys.argv[1], int(sys.argv[2])
ntok = int(sys.argv[3]) if len(sys.argv) > 3 else 3
wtype = int(sys.argv[4]) if len(sys.argv) > 4 else 8
sched = dict(kv.split("=") for kv in sys.argv[5].split(";")) if len(sys.argv) > 5 else None
base = pkg.synth.CONFIGS[cfg]
if sched:
    base = pkg.synth.ModelConfig(**{**base.__dict__, "ctx": int(sched["ctx"])})
    batch, n_prompt = int(sched["batch"]), int(sched["prefill"])
    stretches = [tuple(int(x) for x in s.split("-")) for s in sched["decode"].split(",")]
    toks = pkg.javarand.bench_tokens(base.vocab, base.ctx)
    steps = [p for lo, hi in stretches for p in range(lo, hi + 1)]
    rows = sorted({p for s in stretches for p in s} | ({0, n_prompt - 1} if n_prompt else set()) | {int(p) for p in sched.get("kv", "").split(",") if p})
else:
    batch, n_prompt, stretches, rows = 1, 0, [], []
    toks = pkg.javarand.bench_tokens(base.vocab, ntok)
    steps = list(range(ntok))
m = pkg.synth.make_numpy(base, wtype=wtype, seed=17)
o = orc.COracle(m, vector_bits=0 if wtype == 8 else 256)
if n_prompt: o.prefill(toks[:n_prompt], 0)
ref = [o.forward(toks[p], p) for p in steps]
ref_kv = {(l, p): o.kv(l, p) for l in range(m.cfg.n_layers) for p in rows}
grp = plan_mod.make_local_group(tp)
out, ids, kvs, err = [None] * tp, [None] * tp, [None] * tp, [None] * tp
ready = threading.Barrier(tp)        # a host-level barrier between plan creation and the first forward

def rank_main(r):
    try:
        plan = plan_mod.HipMasterPlan(m, prefill_batch_size=batch, tp_rank=r, tp_size=tp, local_group=grp)
        if r == 0: print("fold mode %d mask %d" % plan.tp_fold_mode(), flush=True)
        ready.wait()
        for off in range(0, n_prompt, batch):
            plan.tornadoVMForwardBatchPrefill(toks[off:min(off + batch, n_prompt)], off)
        res = []
        for p in steps:
            t0 = time.time(); res.append(plan.forward_decode(toks[p], p)); print("rank %d token %d: %.3f s" % (r, p, time.time() - t0), flush=True)
        # (a repeated step rewrites its K / V row with the same values)
        ids[r] = [plan.forward_decode_argmax(toks[hi], hi) for _, hi in stretches]
        kvs[r] = {key: plan.kv(*key) for key in ref_kv}
        out[r] = res
        plan.freeTornadoExecutionPlan()
    except Exception as e:
        err[r] = e
        ready.abort()

th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(tp)]
t0 = time.time()
[t.start() for t in th]; [t.join(timeout=300) for t in th]
print("errors:", err, "in %.1f s" % (time.time() - t0))
bad = sum(e is not None for e in err)
kvl = m.cfg.kv_dim // tp
for r in range(tp):
    if out[r] is None: bad += 1; continue
    eq = [bool(np.array_equal(out[r][i], ref[i])) for i in range(len(steps))]
    bad += eq.count(False)
    print("rank", r, eq)
    if sched:
        want = [orc.argmax(ref[steps.index(hi)]) for _, hi in stretches]
        kv_eq = [bool(np.array_equal(kvs[r][key][0], ko[r * kvl:(r + 1) * kvl]) and np.array_equal(kvs[r][key][1], vo[r * kvl:(r + 1) * kvl])) for key, (ko, vo) in ref_kv.items()]
        bad += (ids[r] != want) + kv_eq.count(False)
        print("rank", r, "greedy ids", ids[r], "oracle", want, "kv rows (layer, position)", dict(zip(ref_kv, kv_eq)))
sys.exit(1 if bad else 0)
