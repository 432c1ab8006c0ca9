"""Token scores on the device against the route without them (profiles/token_score.md).

Model: the `8b-vocab` shape (Llama-3-8B's dim and vocabulary 128256, one layer), Q8_0, random weights, one MI355X.  One step = one
prompt chunk of `rows` tokens from position 0 with every row an output row and the following token as its target, the shape of a
perplexity chunk or of a draft being verified.

  (a) forward_batch_score: the step + score_rows_kernel, 16 bytes per row back
  (b) forward_batch with every row wanted, f32[rows][vocab] logits copied out, and the NumPy scoring the tests use as their reference
      (v - max, exp in double, the strictly sequential f32 sum) on the host
  (b') the step and the logits copy of (b) alone: what (b) costs before any host arithmetic

The three alternate in one process after a warm-up of each; every call ends in the library's own stream synchronise (host clock).
Median and spread over --steps calls each.  GL3_SCORE_TIMING=1 makes the library time score_rows_kernel with HIP events and print it
to stderr; this script sets it for itself, re-reads its own stderr file and reports the median."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32 = np.float32


def host_scores(logits, targets):
    from oracle import oracle_np
    out = np.empty((len(targets), 4), F32)
    for i, v in enumerate(logits):
        mx = v.max()
        e = np.exp((v - mx).astype(np.float64)).astype(F32)
        s = F32(oracle_np.seq_sum(e))
        out[i] = (e[targets[i]] / s, v[targets[i]], mx, s)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-steps", type=int, default=5, help="calls of (b): its host part takes seconds at 512 rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_score.json"))
    ap.add_argument("--stderr-file", default=None, help="where this process's stderr goes (the kernel times are read back from it)")
    a = ap.parse_args()
    os.environ["GL3_SCORE_TIMING"] = "1"
    import __graft_entry__ as ge
    pkg = ge.load_package()
    from importlib import import_module
    plan_mod = import_module(ge.PKG_NAME + ".plan")
    max_batch = max(a.rows)
    cfg = pkg.synth.ModelConfig(**{**pkg.synth.CONFIGS["8b-vocab"].__dict__, "ctx": max(64, max_batch)})
    m = pkg.synth.make_numpy(cfg, seed=11)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=max_batch)
    rng = np.random.default_rng(13)
    result = {"model": "8b-vocab", "vocab": cfg.vocab, "max_batch": max_batch, "steps": a.steps, "cases": []}
    for rows in a.rows:
        toks = rng.integers(0, cfg.vocab, rows + 1).tolist()
        args = (toks[:rows], [0] * rows, list(range(rows)))
        want, targets = [1] * rows, toks[1:]
        score = lambda: plan.forward_batch_score(*args, targets, None, want)
        copy = lambda: plan.forward_batch(*args, want)
        host = lambda: host_scores(copy()[0], targets)
        s, ids = score()
        ref = host()
        same = all(np.array_equal(s[f], ref[:, k]) for k, f in enumerate(("prob", "logit", "max", "sum")))
        copy()
        t = {"a": [], "b": [], "b_copy": []}
        for i in range(a.steps):
            for name, fn in (("a", score), ("b_copy", copy)) + ((("b", host),) if i < a.host_steps else ()):
                t0 = time.perf_counter(); fn(); t[name].append((time.perf_counter() - t0) * 1e3)
        case = {"rows": rows, "bit_identical_to_host_route": bool(same)}
        for name, v in t.items():
            case[name + "_ms"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
    plan.freeTornadoExecutionPlan()
    sys.stderr.flush()
    if a.stderr_file and os.path.exists(a.stderr_file):
        us = {}
        for rows_s, v in re.findall(r"score_rows_kernel rows (\d+): ([0-9.]+) us", open(a.stderr_file).read()):
            us.setdefault(int(rows_s), []).append(float(v))
        for case in result["cases"]:
            v = us.get(case["rows"], [])[1:]                      # the first launch loads the code object
            if v:
                case["score_rows_kernel_us"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
