"""tools/gl3_spec_run against tools/gl3_run on synthetic weights (profiles/spec_decode.md):

    python scripts/spec_decode_bench.py [--models llama-3.2-1b,llama-3-8b] [--n-gen 128] [--reps 3] [--baseline-run PATH] [--out FILE]

Per model: a Q8_0 GGUF written from the synthetic model (fixed seed) into a temporary directory, a prompt that repeats an 8-id unit, and,
alternating over --reps repetitions after one untimed pass of every variant (page cache, code objects), one process each of
    tools/gl3_run                      the plain greedy loop (single-token steps, one graph replay per id)
    --baseline-run PATH                the same host built from another commit (it finds its library through its own rpath)
    tools/gl3_spec_run --draft 0/2/4/7 prompt-lookup drafts, one gl3_forward_batch_verify per step, -b 16
Every process must print the ids of the first one.  tok/s is what the host itself reports: ids over its host clock around steps that end in a
device synchronise, so the first step's one-time work (graph capture) is inside.  Acceptance on random-weight models says nothing about
real text."""
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
    ap.add_argument("--models", default="llama-3.2-1b,llama-3-8b")
    ap.add_argument("--n-gen", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-run", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pkg = ge.load_package()
    synth = pkg.synth
    results = []
    for name in args.models.split(","):
        cfg = synth.CONFIGS[name]
        prompt = pkg.javarand.bench_tokens(cfg.vocab, 8) * 8
        N, NEW = len(prompt), args.n_gen
        ids_arg = ",".join(map(str, prompt))
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "m.gguf")
            model = synth.make_torch(cfg, wtype=synth.GGML_Q8_0, seed=42, device=torch.device("cuda", 0))
            model.write_gguf(path)
            del model
            torch.cuda.empty_cache()
            # gl3_run's begin-of-text slot holds the first prompt id: the same (token, position) sequence as gl3_spec_run's
            plain = ["-m", path, "--protocol", "llama", "--bos", str(prompt[0]), "--ids", ",".join(map(str, prompt[1:])), "-n", str(N - 1 + NEW)]
            variants = [("gl3_run", [os.path.join(ROOT, "tools", "gl3_run")] + plain)]
            if args.baseline_run:
                variants.append(("gl3_run (baseline build)", [args.baseline_run] + plain))
            for K in (0, 2, 4, 7):
                variants.append(("gl3_spec_run --draft %d" % K, [os.path.join(ROOT, "tools", "gl3_spec_run"), "-m", path, "--ids", ids_arg, "-n", str(NEW),
                                                                 "--draft", str(K), "-b", "16"]))
            rows = {v: {"model": name, "variant": v, "n_gen": NEW, "tok_s_all": []} for v, _ in variants}
            ref = None
            for rep in range(args.reps + 1):                  # pass 0 is not timed
                for v, cmd in variants:
                    ids, err = run(cmd)
                    ref = ids if ref is None else ref
                    assert ids == ref and len(ids) == NEW, (name, v, "ids differ from the plain loop")
                    if not rep:
                        continue
                    if "spec_run" in v:
                        rows[v]["tok_s_all"].append(float(re.search(r"tok_s=([\d.]+)", err).group(1)))
                        for k in ("steps", "drafted", "accepted"):
                            rows[v][k] = int(re.search(r"\b%s=(\d+)" % k, err).group(1))
                        rows[v]["step_us_by_rows"] = dict(x.split(":") for x in re.search(r"step_us=(\S+)", err).group(1).split(","))
                    else:
                        rows[v]["tok_s_all"].append(float(re.search(r"generated \d+ in [\d.]+ ms \(([\d.]+) tok/s\)", err).group(1)))
            for v, _ in variants:
                rows[v]["tok_s_median"] = statistics.median(rows[v]["tok_s_all"])
                results.append(rows[v])
                print(json.dumps(rows[v]), flush=True)
            print(json.dumps({"model": name, "distinct_ids": len(set(ref))}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
