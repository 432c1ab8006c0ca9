"""What a draft-tree step costs (profiles/spec_tree.md).

    python scripts/spec_tree_bench.py step [--root TREE] [--modes tree,linear] [--layers 8] [--reps 7] [--inner 5] [--only M,DEPTH]
                                           [--depths 0,4096] [--ms 8,16,64]
    python scripts/spec_tree_bench.py tool [--n-gen 128] [--reps 7] [--draft 7]

step: a Llama-3-8B-shaped random-weight Q8_0 model cut to --layers layers, context 4224, one sequence.  Per prefix depth (--depths) and
m in --ms: `tree` = one gl3_forward_batch_verify_tree over one binary tree of m rows (parents[i] = (i - 1) / 2), `linear` = one
gl3_forward_batch_verify over a chain of the same m tokens; `tree_tiled` / `tree_pair` = the tree step on a plan of its own created under
GL3_PF_TREE_TILED_MIN=0,1 / =1000000000,1 (the tiled form wherever the shape allows / never).  The modes alternate in one process after a warm-up call of each; a sample is
--inner calls in a row (host clock; every call ends in the library's stream synchronise).  --root names the checkout whose package and
library are loaded: a checkout of the parent commit with `--modes linear` is the yardstick, run in turn with this tree.  --only M,DEPTH with
--reps 1 --inner 1 runs one case alone behind its warm-up: the target of a rocprofv3 --kernel-trace --stats run.
tool: tools/gl3_spec_run --branches 1 against --branches 3 at equal --draft on a Llama-3.2-1B-shaped GGUF and the 64-id prompt that repeats an
8-id unit (scripts/spec_decode_bench.py's setup), alternated over --reps processes each after one untimed pass; both must print the same ids.
Prints one JSON line."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(root):
    sys.path.insert(0, root)
    import __graft_entry__ as ge
    from importlib import import_module
    pkg = ge.load_package()
    return pkg, import_module(ge.PKG_NAME + ".plan")


def step(args):
    import torch
    pkg, plan_mod = load(args.root)
    synth = pkg.synth
    depths, ms = tuple(int(x) for x in args.depths.split(",")), tuple(int(x) for x in args.ms.split(","))
    cfg = synth.ModelConfig(**{**synth.CONFIGS["llama-3-8b"].__dict__, "n_layers": args.layers, "ctx": 4096 + 128})
    toks = pkg.javarand.bench_tokens(cfg.vocab, cfg.ctx)
    modes = args.modes.split(",")
    # a plan per GL3_PF_TREE_TILED_MIN setting (read when the plan is created): `tree` and `linear` share the plan of the defaults
    setting = {"tree": None, "linear": None, "tree_tiled": "0,1", "tree_pair": "1000000000,1"}
    plans = {}
    for k in modes:
        if setting[k] not in plans:
            os.environ.pop("GL3_PF_TREE_TILED_MIN", None)
            if setting[k]:
                os.environ["GL3_PF_TREE_TILED_MIN"] = setting[k]
            plans[setting[k]] = plan_mod.HipMasterPlan(
                synth.StreamModel(cfg, synth.GGML_Q8_0, synth.iter_torch(cfg, wtype=synth.GGML_Q8_0, seed=42, device="cuda")), prefill_batch_size=64)
    only = tuple(int(x) for x in args.only.split(",")) if args.only else None
    out = {"root": os.path.abspath(args.root), "layers": args.layers, "cases": {}}
    done = 0
    for depth in sorted(depths):
        if done < depth:
            for plan in plans.values():
                plan.prefill_seq(0, toks[done:depth], done)
            done = depth
        for m in ms:
            if only and only != (m, depth):
                continue
            row = [toks[depth]] + [1000 + i for i in range(1, m)]        # siblings carry distinct tokens
            parents = [-1] + [(i - 1) // 2 for i in range(1, m)]
            tree_pos = [depth + (i + 1).bit_length() - 1 for i in range(m)]

            def call(k):
                plan = plans[setting[k]]
                if k == "linear":
                    return lambda: plan.forward_batch_verify(row, [0] * m, list(range(depth, depth + m)))
                return lambda: plan.forward_batch_verify_tree(row, [0] * m, tree_pos, parents)
            calls = {k: call(k) for k in modes}
            rows = {}
            for k, f in calls.items():
                f()
                if k != "linear":
                    rows[k] = [int(x) for x in plans[setting[k]].attn_rows()]      # the attention form that served the tree step
            samples = {k: [] for k in calls}
            for _ in range(args.reps):
                for k, f in calls.items():
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    for _ in range(args.inner):
                        f()
                    samples[k].append(round(1e3 * (time.perf_counter() - t1) / args.inner, 4))
            out["cases"]["m%d depth%d" % (m, depth)] = {k: dict(median_ms=statistics.median(v), samples_ms=v) for k, v in samples.items()}
            if rows:
                out["cases"]["m%d depth%d" % (m, depth)]["attn_rows"] = rows
    for plan in plans.values():
        plan.freeTornadoExecutionPlan()
    print(json.dumps(out))


def tool(args):
    import torch
    pkg, _ = load(HERE)
    synth = pkg.synth
    cfg = synth.CONFIGS["llama-3.2-1b"]
    prompt = pkg.javarand.bench_tokens(cfg.vocab, 8) * 8
    exe = os.path.join(HERE, "tools", "gl3_spec_run")
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "m.gguf")
        synth.make_torch(cfg, wtype=synth.GGML_Q8_0, seed=42, device=torch.device("cuda", 0)).write_gguf(path)
        torch.cuda.empty_cache()
        ids = None
        for rep in range(args.reps + 1):                                 # repetition 0 is untimed
            for b in (1, 3):
                o = subprocess.run([exe, "-m", path, "--ids", ",".join(map(str, prompt)), "-n", str(args.n_gen), "--draft", str(args.draft),
                                    "--branches", str(b), "-b", "16"], capture_output=True, text=True, timeout=600)
                assert o.returncode == 0, o.stderr
                got = o.stdout.split("generated:")[1].split()
                ids = ids or got
                assert got == ids, "branches %d printed other ids" % b
                if rep:
                    r = res.setdefault("branches %d" % b, {"tok_s": []})
                    r["tok_s"].append(float(re.search(r"tok_s=([\d.]+)", o.stderr).group(1)))
                    r.update({k: int(re.search(r"\b%s=(\d+)" % k, o.stderr).group(1)) for k in ("steps", "drafted", "accepted", "tokens")})
                    r["step_us"] = re.search(r"step_us=(\S*)", o.stderr).group(1)
    print(json.dumps({"draft": args.draft, "n_gen": args.n_gen, "results": res}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["step", "tool"])
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--modes", default="tree,linear")
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--depths", default="0,4096")
    ap.add_argument("--ms", default="8,16,64")
    ap.add_argument("--n-gen", type=int, default=128)
    ap.add_argument("--draft", type=int, default=7)
    a = ap.parse_args()
    (step if a.part == "step" else tool)(a)
