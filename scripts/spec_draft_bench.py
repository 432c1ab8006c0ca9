"""tools/gl3_spec_draft_run against tools/gl3_run and tools/gl3_spec_run on synthetic weights (profiles/spec_draft.md):

    python scripts/spec_draft_bench.py [--target llama-3-8b] [--draft-model llama-3.2-1b] [--n-gen 128] [--reps 3]
                                       [--baseline-run PATH] [--baseline-spec-run PATH] [--out FILE]

Two Q8_0 GGUFs written from the synthetic models (fixed seeds) into a temporary directory, the prompt of scripts/spec_decode_bench.py, and,
alternating over --reps repetitions after one untimed pass of every variant, one process each of
    tools/gl3_run, tools/gl3_spec_run --draft 4           the hosts whose code paths this feature does not touch
    --baseline-run / --baseline-spec-run PATH             the same hosts built from another commit (each finds its library through its rpath)
    tools/gl3_spec_draft_run --draft 4                    greedy: must print the ids of the plain loop
    tools/gl3_spec_draft_run --draft 2 / 4 --temperature 0.8 --seed 7
tok/s is what each host itself reports.  Acceptance on random-weight models says nothing about real text."""
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
    ap.add_argument("--baseline-run", default=None)
    ap.add_argument("--baseline-spec-run", default=None)
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
    tool = lambda name: os.path.join(ROOT, "tools", name)
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
        draft = lambda K, extra: [tool("gl3_spec_draft_run"), "-m", paths[0], "-md", paths[1], "--ids", ids_arg, "-n", str(NEW), "--draft", str(K),
                                  "-b", "16"] + extra
        variants = [("gl3_run", [tool("gl3_run")] + plain, True)]
        if args.baseline_run:
            variants.append(("gl3_run (baseline build)", [args.baseline_run] + plain, True))
        variants.append(("gl3_spec_run --draft 4", [tool("gl3_spec_run")] + spec, True))
        if args.baseline_spec_run:
            variants.append(("gl3_spec_run --draft 4 (baseline build)", [args.baseline_spec_run] + spec, True))
        variants.append(("gl3_spec_draft_run --draft 4", draft(4, []), True))
        for K in (2, 4):
            variants.append(("gl3_spec_draft_run --draft %d --temperature 0.8" % K, draft(K, ["--temperature", "0.8", "--seed", "7"]), False))
        rows = {v: {"target": args.target, "draft_model": args.draft_model, "variant": v, "n_gen": NEW, "tok_s_all": []} for v, _, _ in variants}
        ref, sampled = None, {}
        for rep in range(args.reps + 1):                  # pass 0 is not timed
            for v, cmd, greedy in variants:
                ids, err = run(cmd)
                if greedy:
                    ref = ids if ref is None else ref
                    assert ids == ref and len(ids) == NEW, (v, "ids differ from the plain loop")
                else:
                    assert sampled.setdefault(v, ids) == ids and len(ids) == NEW, (v, "ids differ between repetitions")
                if not rep:
                    continue
                if "spec_" in v:
                    rows[v]["tok_s_all"].append(float(re.search(r"tok_s=([\d.]+)", err).group(1)))
                    for k in ("steps", "drafted", "accepted"):
                        rows[v][k] = int(re.search(r"\b%s=(\d+)" % k, err).group(1))
                    rows[v]["step_us_by_rows"] = dict(x.split(":") for x in re.search(r"step_us=(\S+)", err).group(1).split(","))
                    dm = re.search(r"draft_ms=([\d.]+)", err)
                    if dm:
                        rows[v]["draft_ms"] = float(dm.group(1))
                        rows[v]["decode_ms"] = float(re.search(r"decode_ms=([\d.]+)", err).group(1))
                else:
                    rows[v]["tok_s_all"].append(float(re.search(r"generated \d+ in [\d.]+ ms \(([\d.]+) tok/s\)", err).group(1)))
        results = []
        for v, _, _ in variants:
            rows[v]["tok_s_median"] = statistics.median(rows[v]["tok_s_all"])
            results.append(rows[v])
            print(json.dumps(rows[v]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
