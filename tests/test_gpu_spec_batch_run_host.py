"""tools/gl3_spec_batch_run: continuous-batching speculative decoding with a draft model, every step ONE gl3_forward_decode_batch_chain on the
draft plan and ONE gl3_forward_batch_verify_dist on the target.  5 requests on 2 slots (slots are reused): request r's ids are tools/gl3_run's
greedy ids at temperature 0 and those of tools/gl3_spec_draft_run --chain --seed S+r at a temperature; --no-chain (k calls of
gl3_forward_decode_batch_sample + gl3_draft_probs_put_row) prints the same ids and the same counts line; a -b below NP * (K + 1) exits 2."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "gl3_spec_batch_run")
DRAFT_RUN = os.path.join(ROOT, "tools", "gl3_spec_draft_run")
RUN = os.path.join(ROOT, "tools", "gl3_run")
NEW, NP, SEED = 12, 2, 7
LENGTHS = (7, 3, 9, 5, 4)


def batch_run(paths, prompts_file, draft, extra, np_=NP, batch=None, ok=True):
    """-> ([ids of request r], the counts line)"""
    b = NP * (int(draft) + 1) if batch is None else batch
    out = subprocess.run([EXE, "-m", paths[0], "-md", paths[1], "--prompts", prompts_file, "-np", str(np_), "-n", str(NEW), "--draft", str(draft),
                          "-b", str(b)] + extra, capture_output=True, text=True, timeout=180)
    if not ok:
        return out
    assert out.returncode == 0, out.stderr
    lines = [l for l in out.stderr.splitlines() if l.startswith("steps=")]
    assert len(lines) == 1 and any(l.startswith("timing: ") and " draft_ms=" in l for l in out.stderr.splitlines()), out.stderr
    rows = out.stdout.splitlines()
    assert [r.split(":")[0] for r in rows] == ["request %d" % r for r in range(len(LENGTHS))], out.stdout
    return [[int(x) for x in r.split(":")[1].split()] for r in rows], lines[0]


def counts(line):
    return {k: int(v) for k, v in (f.split("=") for f in line.split())}


@pytest.fixture(scope="module")
def setup(pkg, tmp_path_factory):
    cfg = pkg.synth.CONFIGS["tiny-llama"]
    d = tmp_path_factory.mktemp("spec_batch")
    paths = [str(d / "target.gguf"), str(d / "draft.gguf")]
    synth = pkg.synth
    tm = synth.make_numpy(cfg, seed=85)
    tm.write_gguf(paths[0])
    synth.make_numpy(dataclasses.replace(cfg, n_layers=1), seed=86).write_gguf(paths[1])
    # A 1-layer draft that sometimes agrees with the target under greedy decoding (two random models never do): the target's embedding,
    # first layer and output tensors, with the first layer's down projection taken from another seed.  Chosen on the CPU oracle: over the five
    # prompts below it has 3 drafts accepted at --draft 2 (request 2: both drafts of one step, so that request catches up while the request in
    # the other slot was rejected; request 4: one of two) and 3 at --draft 4 (2 of 3 and 1 of 4: partial acceptances), every other draft rejected.
    c1 = dataclasses.replace(cfg, n_layers=1)
    other = synth.make_numpy(cfg, seed=86)
    near = {n: (other if n == "blk.0.ffn_down.weight" else tm).tensors[n] for n, *_ in synth.tensor_specs(c1, tm.wtype)}
    paths.append(str(d / "draft_near.gguf"))
    synth.SynthModel(c1, tm.wtype, near).write_gguf(paths[2])
    g = np.random.default_rng(85)
    prompts = [g.integers(0, cfg.vocab, n).tolist() for n in LENGTHS]
    f = str(d / "prompts.txt")
    with open(f, "w") as fh:
        fh.write("".join(",".join(map(str, p)) + "\n" for p in prompts))
    return paths, prompts, f


@pytest.fixture(scope="module")
def greedy_ids(setup):
    """tools/gl3_run's greedy ids of every prompt, once for the module"""
    paths, prompts, _ = setup
    ids = []
    for p in prompts:
        out = subprocess.run([RUN, "-m", paths[0], "--protocol", "llama", "--bos", str(p[0]), "--ids", ",".join(map(str, p[1:])), "-n", str(len(p) - 1 + NEW)],
                             capture_output=True, text=True, timeout=180)
        assert out.returncode == 0, out.stderr
        ids.append([int(x) for x in out.stdout.split("generated:")[1].split()])
    return ids


@pytest.mark.parametrize("draft", ["2", "4"])
def test_greedy_requests_are_gl3_run(setup, greedy_ids, draft):
    """The draft is the one the fixture chose on the CPU oracle: some drafts stand, most do not, so in one step a request catches up while
    another was rejected, and runs are accepted in part (0 < a < k)."""
    paths, _, f = setup
    near = [paths[0], paths[2]]
    chained = batch_run(near, f, draft, [])
    plain = batch_run(near, f, draft, ["--no-chain"])
    assert chained == plain, (chained, plain)
    assert chained[0] == greedy_ids and all(len(r) == NEW for r in chained[0])
    c = counts(chained[1])
    assert 0 < c["accepted"] < c["drafted"] and c["accepted"] == 3 and c["tokens"] == NEW * len(LENGTHS), chained[1]
    # the random draft: nothing stands, the ids are the same
    ids, line = batch_run(paths, f, draft, [])
    assert ids == greedy_ids and counts(line)["drafted"] > 0, line


def test_a_draft_that_is_the_target_is_always_accepted(setup, greedy_ids):
    """The target's own file as the draft model: every greedy draft stands, so every step ends with the catch-up of the draft plan, and the
    ids are still gl3_run's; at a temperature q == p bit for bit and every draft is accepted too."""
    paths, _, f = setup
    same = [paths[0], paths[0]]
    for extra in ([], ["--no-chain"]):
        ids, line = batch_run(same, f, "4", extra)
        c = counts(line)
        assert ids == greedy_ids and c["accepted"] == c["drafted"] > 0, line
    sampled = [batch_run(same, f, "4", ["--temperature", "0.8", "--seed", str(SEED)] + extra) for extra in ([], ["--no-chain"])]
    c = counts(sampled[0][1])
    assert sampled[0] == sampled[1] and c["accepted"] == c["drafted"] > 0, sampled


@pytest.mark.parametrize("draft", ["2", "4"])
def test_sampled_requests_are_the_single_sequence_host(setup, draft):
    paths, prompts, f = setup
    args = ["--temperature", "0.8", "--seed", str(SEED)]
    chained = batch_run(paths, f, draft, args)
    plain = batch_run(paths, f, draft, args + ["--no-chain"])
    assert chained == plain, (chained, plain)
    c = counts(chained[1])
    assert c["drafted"] > 0 and c["accepted"] > 0 and c["tokens"] == NEW * len(LENGTHS), chained[1]
    for r, p in enumerate(prompts):
        out = subprocess.run([DRAFT_RUN, "-m", paths[0], "-md", paths[1], "--ids", ",".join(map(str, p)), "-b", str(int(draft) + 1), "-n", str(NEW),
                              "--draft", draft, "--temperature", "0.8", "--seed", str(SEED + r), "--chain"], capture_output=True, text=True, timeout=180)
        assert out.returncode == 0, out.stderr
        assert [int(x) for x in out.stdout.split("generated:")[1].split()] == chained[0][r], r


def test_a_batch_too_small_for_every_run_is_refused(setup):
    paths, _, f = setup
    out = batch_run(paths, f, "4", [], batch=NP * 5 - 1, ok=False)
    assert out.returncode == 2 and "NP * (K + 1)" in out.stderr and not out.stdout
