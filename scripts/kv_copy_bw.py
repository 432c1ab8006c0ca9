"""gl3_kv_seq_copy (prefix fork) at the Llama-3-8B K / V shape: bandwidth of the copy, and the step that reads the copied rows next.

Model: 32 layers, 32 query heads on 8 kv heads of 128 (kv_dim 1024) like Llama-3-8B, but dim 256 / hidden 512 / vocabulary 512 — only n_layers,
kv_dim and ctx matter to the copy.  Q8_0, random weights, 8 sequence slots of 4096 rows (1 GiB of K / V rows per slot), one MI355X.

  copy:  rows [0, R) of slot 0 into F other slots, R in (512, 4096), F in (1, 7).  A call ends in the library's own stream synchronise, so the host
         clock around it is the call time: one host-to-device copy of the destination list, one launch, one wait.  Median over --reps calls after
         a warm-up; bytes = read once + written F times; GB/s over the median.  `floor_us` is the same call for ONE row (64 small workgroups): what a
         call costs before it moves anything.
  next:  the step a fork is made for — one decode row on the destination at position R, right behind a copy of R rows with F = 1 — timed by itself
         (copy and step alternate, so every timed step reads rows the copy has just written).  Its attention reads all 2 * 32 * R copied rows.

gl3_probe_peaks's device-to-device copy figure of the same run is the yardstick (bytes counted the same way: read + written).  Before anything is
timed the source slot is prefilled with 4096 tokens and after the last call copied rows of the first and last layer are compared with the source.
One JSON line on stdout and in --out.  GL3_LIB names another build of the library (e.g. one compiled with -DKVC_NT_STORES=1)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        us.append((time.perf_counter() - t0) * 1e6)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--fan-out", type=int, nargs="+", default=[1, 7])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_seq_copy.json"))
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    from importlib import import_module
    plan_mod, hip = import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")
    ctx, n_seqs = max(a.rows) + 8, max(a.fan_out) + 1
    cfg = pkg.synth.ModelConfig(**{**pkg.synth.CONFIGS["tiny-llama"].__dict__, "name": "llama-3-8b-kv-shape", "n_layers": 32, "n_heads": 32, "n_kv_heads": 8,
                                   "head_size": 128, "ctx": ctx})
    m = pkg.synth.make_numpy(cfg, seed=17)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=512, n_seqs=n_seqs)
    rng = np.random.default_rng(19)
    plan.prefill_seq(0, rng.integers(0, cfg.vocab, max(a.rows)).tolist(), 0)
    row_bytes = 2 * cfg.n_layers * cfg.kv_dim * 4                       # K and V of one position, every layer
    read_gbs, copy_gbs = C.c_double(), C.c_double()
    hip.check(hip.lib().gl3_probe_peaks(0, C.byref(read_gbs), C.byref(copy_gbs), None))
    floor = timed(lambda: plan.kv_seq_copy(0, [1], 0, 1), a.reps, a.warmup)
    res = {"lib": os.path.basename(hip.SO_PATH), "n_layers": cfg.n_layers, "kv_dim": cfg.kv_dim, "ctx": ctx, "n_seqs": n_seqs, "reps": a.reps,
           "probe_hbm_read_gbs": round(read_gbs.value, 1), "probe_copy_gbs": round(copy_gbs.value, 1), "floor_us": round(statistics.median(floor), 1),
           "copy": [], "next_step": []}
    for rows in a.rows:
        for f in a.fan_out:
            dsts = list(range(1, f + 1))
            us = timed(lambda: plan.kv_seq_copy(0, dsts, 0, rows), a.reps, a.warmup)
            med, rd, wr = statistics.median(us), rows * row_bytes, f * rows * row_bytes
            res["copy"].append({"rows": rows, "fan_out": f, "bytes_read": rd, "bytes_written": wr, "us": round(med, 1), "us_min": round(min(us), 1),
                                "us_max": round(max(us), 1), "gbs": round((rd + wr) / med / 1e3, 1), "share_of_probe_copy": round((rd + wr) / med / 1e3 / copy_gbs.value, 3)})
    for rows in a.rows:
        tok = int(rng.integers(0, cfg.vocab))
        step_us = []

        def pair():
            plan.kv_seq_copy(0, [1], 0, rows)
            t0 = time.perf_counter()
            plan.forward_decode_batch([tok], [1], [rows], want_logits=False)
            step_us.append((time.perf_counter() - t0) * 1e6)
        timed(pair, a.reps, a.warmup)
        res["next_step"].append({"rows": rows, "step_us": round(statistics.median(step_us[a.warmup:]), 1)})
    for f in range(1, n_seqs):                                          # what the timed calls left behind: slot f holds the source's rows
        for l in (0, cfg.n_layers - 1):
            for p in (0, 1, min(a.rows) - 1, max(a.rows) // 2 + 1, max(a.rows) - 1):
                k, v = plan.kv_seq(f, l, p)
                ks, vs = plan.kv_seq(0, l, p)
                assert ks.any() and np.array_equal(k, ks) and np.array_equal(v, vs), ("copied rows differ", f, l, p)
    res["rows_checked"] = True
    plan.freeTornadoExecutionPlan()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
