"""tools/gl3_spec_batch_run with and without --no-chain, and tools/gl3_spec_draft_run --chain once per request (profiles/spec_batch.md):

    python scripts/spec_batch_bench.py [--target llama-3-8b] [--draft-model llama-3.2-1b] [--draft-layers N] [--requests 8] [--np 8]
                                       [--n-gen 64] [--reps 3] [--out FILE]

The protocol of scripts/spec_draft_bench.py: two Q8_0 GGUFs written from the synthetic models (fixed seeds; --draft-layers cuts the draft
model to its first N layers' shape) into a temporary directory, --requests prompts of 24 to 64 ids, and, alternating over --reps
repetitions after one untimed pass of every variant, for --draft 2 / 4, greedy and --temperature 0.8 --seed 7:
    gl3_spec_batch_run -np NP                     the batched chain: one gl3_forward_decode_batch_chain per step
    gl3_spec_batch_run -np NP --no-chain          k gl3_forward_decode_batch_sample calls (+ gl3_draft_probs_put_row) per step
    gl3_spec_draft_run --chain, once per request  B separate chains: one process per request, their decode times and ids added up
Asserted on every pass: --no-chain prints the ids and the counts line of the run with the chain, and request r's ids are those of the
single-sequence host at --seed 7 + r.  Reported per variant: tokens/s (all requests' ids over decode_ms), draft_ms per speculation step
and host waits on the draft plan per step (draft_calls / steps: every forward call on the draft plan waits for the device once).  --out
is rewritten after every repetition, so a run that is cut short leaves what it had."""
import argparse
import dataclasses
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

TOOLS = os.path.join(ROOT, "tools")


def run(cmd):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (cmd, out.stderr)
    return out.stdout, out.stderr


def field(err, name, kind=float):
    return kind(re.search(r"\b%s=([\d.]+)" % name, err).group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", default="llama-3-8b")
    ap.add_argument("--draft-model", default="llama-3.2-1b")
    ap.add_argument("--draft-layers", type=int, default=0)
    ap.add_argument("--requests", type=int, default=8)
    ap.add_argument("--np", type=int, default=8)
    ap.add_argument("--n-gen", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pkg = ge.load_package()
    synth = pkg.synth
    tcfg, dcfg = synth.CONFIGS[args.target], synth.CONFIGS[args.draft_model]
    if args.draft_layers:
        dcfg = dataclasses.replace(dcfg, n_layers=args.draft_layers, name="%s-%dlayers" % (dcfg.name, args.draft_layers))
    assert tcfg.vocab == dcfg.vocab
    stream = pkg.javarand.bench_tokens(tcfg.vocab, 64 * args.requests)
    prompts = [stream[64 * r:64 * r + 24 + (40 * r) // max(args.requests - 1, 1)] for r in range(args.requests)]
    NEW, R = args.n_gen, args.requests
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for cfg, seed in ((tcfg, 42), (dcfg, 43)):
            paths.append(os.path.join(tmp, "%s.gguf" % cfg.name))
            model = synth.make_torch(cfg, wtype=synth.GGML_Q8_0, seed=seed, device=torch.device("cuda", 0))
            model.write_gguf(paths[-1])
            del model
            torch.cuda.empty_cache()
        pfile = os.path.join(tmp, "prompts.txt")
        with open(pfile, "w") as f:
            f.write("".join(",".join(map(str, p)) + "\n" for p in prompts))
        variants = []                                    # (name, kind, K, mode arguments)
        for K in (2, 4):
            for mode, extra in (("greedy", []), ("--temperature 0.8", ["--temperature", "0.8"])):
                for kind in ("batch chain", "batch --no-chain", "single chains"):
                    variants.append(("--draft %d %s: %s" % (K, mode, kind), kind, K, extra))
        rows = {v[0]: {"target": tcfg.name, "draft_model": dcfg.name, "variant": v[0], "requests": R, "np": args.np, "n_gen": NEW, "tok_s_all": [],
                       "draft_ms_per_step_all": [], "draft_waits_per_step_all": []} for v in variants}
        seen = {}
        for rep in range(args.reps + 1):                  # pass 0 is not timed
            for name, kind, K, extra in variants:
                key = name.split(":")[0]
                if kind == "single chains":
                    ids, decode_ms, draft_ms, steps, calls = [], 0.0, 0.0, 0, 0
                    for r, p in enumerate(prompts):
                        out, err = run([os.path.join(TOOLS, "gl3_spec_draft_run"), "-m", paths[0], "-md", paths[1], "--ids", ",".join(map(str, p)), "-n", str(NEW),
                                        "--draft", str(K), "-b", str(K + 1), "--seed", str(7 + r), "--chain"] + extra)
                        ids.append([int(x) for x in out.split("generated:")[1].split()])
                        decode_ms += field(err, "decode_ms"); draft_ms += field(err, "draft_ms")
                        steps += field(err, "steps", int)
                    calls = steps                                 # one chain per step; that host does not count its catch-up calls
                    tok_s = sum(map(len, ids)) / (decode_ms * 1e-3)
                    counts = None
                else:
                    out, err = run([os.path.join(TOOLS, "gl3_spec_batch_run"), "-m", paths[0], "-md", paths[1], "--prompts", pfile, "-np", str(args.np), "-n", str(NEW),
                                    "--draft", str(K), "--seed", "7"] + extra + (["--no-chain"] if kind == "batch --no-chain" else []))
                    ids = [[int(x) for x in l.split(":")[1].split()] for l in out.splitlines()]
                    counts = [l for l in err.splitlines() if l.startswith("steps=")][0]
                    steps, calls = field(err, "steps", int), field(err, "draft_calls", int)
                    draft_ms, tok_s = field(err, "draft_ms"), field(err, "tok_s")
                    assert seen.setdefault(key + " counts", counts) == counts, (name, counts)
                assert seen.setdefault(key, ids) == ids and all(len(i) == NEW for i in ids), (name, "ids differ")
                if not rep:
                    continue
                r = rows[name]
                r["tok_s_all"].append(tok_s)
                r["steps"] = steps
                r["draft_ms_per_step_all"].append(draft_ms / steps)
                r["draft_waits_per_step_all"].append(calls / steps)
                if counts:
                    r["counts"] = counts
            results = []
            for v in variants:
                r = dict(rows[v[0]])
                for k in ("tok_s", "draft_ms_per_step", "draft_waits_per_step"):
                    if r[k + "_all"]:
                        r[k + "_median"] = statistics.median(r[k + "_all"])
                        r[k + "_range"] = [min(r[k + "_all"]), max(r[k + "_all"])]
                results.append(r)
            if args.out:
                with open(args.out, "w") as f:
                    json.dump(results, f, indent=1)
            print("pass %d of %d done" % (rep, args.reps), flush=True)
        for r in results:
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
