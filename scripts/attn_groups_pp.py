"""pp512 of the Qwen2.5-7B shape (kvMul 7: head groups of 4 + 3) and the Phi-3-mini shape (head size 96) on one MI355X, with this build's library and
with another build's (the parent commit's) in the same session.

The reference's LlamaBench protocol for pp (512 prompt tokens, no logits), random Q8_0 weights, 4 layers of each shape:
    pp512 at -b 512 and at -b 64 into an empty cache, and pp512 at -b 512 behind an untimed prefill of 4096 positions (d4096).
Each (library, shape) runs in a child process of its own (GL3_LIB is read when the binding loads); the two libraries alternate shape by shape.
Prints one JSON line and, with --out, writes it to a file.  Samples are tokens/s of one repetition; the ratio is new median / parent median,
and a point counts as slower only when the new median is below the parent's slowest repetition.

    python scripts/attn_groups_pp.py --parent-lib /path/to/parent/libgpullama_hip.so [--layers 4] [--reps 5] [--out profiles/attn_head_groups.json]

--child SHAPE [--only pp512|pp64|d4096 --reps 1] runs one shape with the library GL3_LIB names (default: this build's): the target of a
rocprofv3 --kernel-trace --stats run of one chunk."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ("qwen2.5-7b", "phi-3-mini")
POINTS = ("pp512", "pp64", "d4096")


def child(args):
    import __graft_entry__ as ge
    from importlib import import_module
    pkg = ge.load_package()
    synth = pkg.synth
    plan_mod = import_module(ge.PKG_NAME + ".plan")
    depth = 4096
    cfg = synth.CONFIGS[args.child]
    cfg = synth.ModelConfig(**{**cfg.__dict__, "ctx": depth + args.n_prompt + 8, "n_layers": args.layers})
    toks = pkg.javarand.bench_tokens(cfg.vocab, depth + args.n_prompt)
    plan = plan_mod.HipMasterPlan(synth.StreamModel(cfg, synth.GGML_Q8_0, synth.iter_torch(cfg, wtype=synth.GGML_Q8_0, seed=42, device="cuda")),
                                  prefill_batch_size=args.n_prompt)
    res = {}
    for point in POINTS:
        if args.only not in (None, point):
            continue
        batch = 64 if point == "pp64" else args.n_prompt
        start = depth if point == "d4096" else 0
        plan.reset_kv()
        if start:
            plan.prefill(toks[:start], 0, batch=args.n_prompt)              # untimed: the context the timed chunk attends to
        plan.prefill(toks[start:start + args.n_prompt], start, batch=batch)      # warm-up
        samples = []
        for _ in range(args.reps):
            t1 = time.perf_counter()
            plan.prefill(toks[start:start + args.n_prompt], start, batch=batch)      # (the same rows again: the cache behind them is unchanged)
            samples.append(args.n_prompt / (time.perf_counter() - t1))
        res[point] = dict(min=round(min(samples), 1), median=round(statistics.median(samples), 1), max=round(max(samples), 1),
                          samples_tok_s=[round(s, 1) for s in samples], attn_rows=plan.attn_rows())
    plan.freeTornadoExecutionPlan()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-prompt", type=int, default=512)
    ap.add_argument("--parent-lib", default=None, help="libgpullama_hip.so of the build to compare against")
    ap.add_argument("--child", choices=SHAPES, default=None)
    ap.add_argument("--only", choices=POINTS, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    libs = [("new", None)] + ([("parent", os.path.abspath(args.parent_lib))] if args.parent_lib else [])
    res = {name: {} for name, _ in libs}
    for shape in SHAPES:
        for name, lib in libs:
            env = dict(os.environ)
            env.pop("GL3_LIB", None)
            if lib:
                env["GL3_LIB"] = lib
            cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--layers", str(args.layers), "--reps", str(args.reps),
                   "--n-prompt", str(args.n_prompt)] + (["--only", args.only] if args.only else [])
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
            if out.returncode != 0:                                          # nothing more on the GPU behind a failed child
                raise SystemExit("%s / %s failed (%d):\n%s" % (name, shape, out.returncode, (out.stdout + out.stderr)[-2000:]))
            res[name][shape] = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            print(name, shape, json.dumps(res[name][shape]), file=sys.stderr, flush=True)
    ratios, slower = {}, []
    if "parent" in res:
        for shape in SHAPES:
            ratios[shape] = {}
            for point, new in res["new"][shape].items():
                old = res["parent"][shape][point]
                ratios[shape][point] = round(new["median"] / old["median"], 3)
                if new["median"] < old["min"]:
                    slower.append("%s %s" % (shape, point))
    line = json.dumps(dict(metric="pp%d tokens/s" % args.n_prompt, value=res["new"][SHAPES[0]].get("pp512", {}).get("median"), unit="tokens/s", n_gpus=1,
                           reps=args.reps, dtype="q8_0", data="synthetic",
                           config=dict(workload="Qwen2.5-7B and Phi-3-mini shapes, Q8_0, %d layers, random weights" % args.layers),
                           new_over_parent_median=ratios, slower_than_parent_spread=slower, **res))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
