"""tools/gl3_spec_draft_run with and without --chain, against the same host built from the parent commit (profiles/spec_chain.md):

    python scripts/spec_chain_bench.py --baseline-dir PARENT_TREE [--target llama-3-8b] [--draft-model llama-3.2-1b] [--n-gen 128]
                                       [--reps 3] [--out FILE]

The protocol of scripts/spec_draft_bench.py: two Q8_0 GGUFs written from the synthetic models (fixed seeds) into a temporary directory, its
prompt, and, alternating over --reps repetitions after one untimed pass of every variant, one process each of
    tools/gl3_run, tools/gl3_spec_run --draft 4                      this build and PARENT_TREE's: code this feature does not touch
    tools/gl3_spec_draft_run --draft 2 / 4, greedy and --temperature 0.8 --seed 7:
        this build, this build with --chain, PARENT_TREE's build
PARENT_TREE is a checkout of the parent commit with its csrc/ built (each host finds its own library through its rpath).  Asserted on every
pass: a --chain run prints the ids of the run without it, the parent's build prints them too, and greedy runs print the ids of tools/gl3_run.
draft_ms per drafted token is what the chain is measured by; tok/s is what each host itself reports.  --out is rewritten after every
repetition, so a run that is cut short leaves what it had."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def run(cmd):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (cmd, out.stderr)
    return [int(x) for x in out.stdout.split("generated:")[1].split()], out.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", default="llama-3-8b")
    ap.add_argument("--draft-model", default="llama-3.2-1b")
    ap.add_argument("--n-gen", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-dir", required=True)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pkg = ge.load_package()
    synth = pkg.synth
    tcfg, dcfg = synth.CONFIGS[args.target], synth.CONFIGS[args.draft_model]
    assert tcfg.vocab == dcfg.vocab
    prompt = pkg.javarand.bench_tokens(tcfg.vocab, 8) * 8
    N, NEW = len(prompt), args.n_gen
    ids_arg = ",".join(map(str, prompt))
    builds = {"": os.path.join(ROOT, "tools"), " (parent build)": os.path.join(os.path.abspath(args.baseline_dir), "tools")}
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for cfg, seed in ((tcfg, 42), (dcfg, 43)):
            paths.append(os.path.join(tmp, "%s.gguf" % cfg.name))
            model = synth.make_torch(cfg, wtype=synth.GGML_Q8_0, seed=seed, device=torch.device("cuda", 0))
            model.write_gguf(paths[-1])
            del model
            torch.cuda.empty_cache()
        plain = ["-m", paths[0], "--protocol", "llama", "--bos", str(prompt[0]), "--ids", ",".join(map(str, prompt[1:])), "-n", str(N - 1 + NEW)]
        spec = ["-m", paths[0], "--ids", ids_arg, "-n", str(NEW), "--draft", "4", "-b", "16"]
        draft = ["-m", paths[0], "-md", paths[1], "--ids", ids_arg, "-n", str(NEW), "-b", "16"]
        variants = []                                    # (name, command, the variant whose ids it must print)
        for tag, tools in builds.items():
            variants.append(("gl3_run" + tag, [os.path.join(tools, "gl3_run")] + plain, "gl3_run"))
        for tag, tools in builds.items():
            variants.append(("gl3_spec_run --draft 4" + tag, [os.path.join(tools, "gl3_spec_run")] + spec, "gl3_run"))
        for K in (2, 4):
            for mode, extra in (("greedy", []), ("--temperature 0.8", ["--temperature", "0.8", "--seed", "7"])):
                name = "--draft %d %s" % (K, mode)
                same = "gl3_run" if mode == "greedy" else name
                for tag, tools in builds.items():
                    variants.append((name + tag, [os.path.join(tools, "gl3_spec_draft_run")] + draft + ["--draft", str(K)] + extra, same))
                variants.append((name + " --chain", [os.path.join(builds[""], "gl3_spec_draft_run")] + draft + ["--draft", str(K)] + extra + ["--chain"], same))
        rows = {v: {"target": args.target, "draft_model": args.draft_model, "variant": v, "n_gen": NEW, "tok_s_all": [], "draft_ms_per_draft_all": []}
                for v, _, _ in variants}
        ids_of = {}
        for rep in range(args.reps + 1):                  # pass 0 is not timed
            for v, cmd, same in variants:
                ids, err = run(cmd)
                assert ids_of.setdefault(same, ids) == ids and len(ids) == NEW, (v, "ids differ from " + same)
                if not rep:
                    continue
                r = rows[v]
                if v.startswith("gl3_run"):
                    r["tok_s_all"].append(float(re.search(r"generated \d+ in [\d.]+ ms \(([\d.]+) tok/s\)", err).group(1)))
                    continue
                r["tok_s_all"].append(float(re.search(r"tok_s=([\d.]+)", err).group(1)))
                for k in ("steps", "drafted", "accepted"):
                    r[k] = int(re.search(r"\b%s=(\d+)" % k, err).group(1))
                dm = re.search(r"draft_ms=([\d.]+)", err)
                if dm and r["drafted"]:
                    r["draft_ms_per_draft_all"].append(float(dm.group(1)) / r["drafted"])
            results = []
            for v, _, _ in variants:
                r = dict(rows[v])
                if r["tok_s_all"]:
                    r["tok_s_median"] = statistics.median(r["tok_s_all"])
                if r["draft_ms_per_draft_all"]:
                    r["draft_ms_per_draft_median"] = statistics.median(r["draft_ms_per_draft_all"])
                results.append(r)
            if args.out:
                with open(args.out, "w") as f:
                    json.dump(results, f, indent=1)
            print("pass %d of %d done" % (rep, args.reps), flush=True)
        for r in results:
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
