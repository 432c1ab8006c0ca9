"""tools/gl3_spec_draft_run (plain C++ over the C-ABI: a draft plan and a target plan, one gl3_draft_probs_put per sampled draft, one
gl3_forward_batch_verify_dist per step) on two tiny synthetic GGUFs: greedy, it prints the target's plain greedy ids — tools/gl3_run's —
whatever the draft model; at a temperature its ids and its step / draft / accept counts are those of the loop replayed in Python on the two
CPU oracles with the same coin stream (verify_dist_ref.simulate_draft_run)."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import verify_dist_ref as vd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "gl3_spec_draft_run")
RUN = os.path.join(ROOT, "tools", "gl3_run")
NEW, BATCH = 24, 8


def draft_run(paths, prompt, extra):
    out = subprocess.run([EXE, "-m", paths[0], "-md", paths[1], "--ids", ",".join(map(str, prompt)), "-b", str(BATCH), "-n", str(NEW)] + extra,
                         capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stderr
    lines = [l for l in out.stderr.splitlines() if l.startswith("steps=")]
    assert len(lines) == 1 and any(l.startswith("timing: ") for l in out.stderr.splitlines()), out.stderr
    counts = tuple(int(re.search(r"\b%s=(\d+)" % k, lines[0]).group(1)) for k in ("steps", "drafted", "accepted", "tokens"))
    return [int(x) for x in out.stdout.split("generated:")[1].split()], counts


@pytest.fixture(scope="module")
def setup(pkg, tmp_path_factory):
    cfg = pkg.synth.CONFIGS["tiny-llama"]
    d = tmp_path_factory.mktemp("spec_draft")
    paths = [str(d / "target.gguf"), str(d / "draft.gguf")]
    pkg.synth.make_numpy(cfg, seed=85).write_gguf(paths[0])
    pkg.synth.make_numpy(dataclasses.replace(cfg, n_layers=1), seed=86).write_gguf(paths[1])
    return paths, np.random.default_rng(85).integers(0, cfg.vocab, 7).tolist()


def simulate(pkg, orc, paths, prompt, **kw):
    oracles = [orc.COracle(pkg.synth.SynthModel.from_gguf(p)) for p in paths]
    for o in oracles:
        o.prefill(prompt[:-1], 0)
    gen, steps, drafted, accepted = vd.simulate_draft_run(prompt, oracles[0].forward, oracles[1].forward, NEW, batch=BATCH, **kw)
    return gen, (steps, drafted, accepted, len(gen))


def test_greedy_ids_are_the_plain_greedy_ids_whatever_the_draft_model(pkg, orc, setup):
    paths, prompt = setup
    want, counts = simulate(pkg, orc, paths, prompt, rng=pkg.javarand.L32X64MixRandom(1234), draft=4)
    got, got_counts = draft_run(paths, prompt, ["--draft", "4"])
    assert got == want and got_counts == counts and len(got) == NEW
    # the same (token, position) sequence through tools/gl3_run: its begin-of-text slot holds the first prompt id
    out = subprocess.run([RUN, "-m", paths[0], "--protocol", "llama", "--bos", str(prompt[0]), "--ids", ",".join(map(str, prompt[1:])),
                          "-n", str(len(prompt) - 1 + NEW)], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stderr
    assert [int(x) for x in out.stdout.split("generated:")[1].split()] == got
    # the target drafting for itself: every draft stands
    same, same_counts = draft_run([paths[0], paths[0]], prompt, ["--draft", "4"])
    assert same == got and same_counts[1] == same_counts[2] > 0


def test_sampled_ids_and_counters_are_the_simulation(pkg, orc, setup):
    paths, prompt = setup
    want, counts = simulate(pkg, orc, paths, prompt, rng=pkg.javarand.L32X64MixRandom(7), draft=4, temperature=0.8)
    assert 0 < counts[2] < counts[1]                                    # drafts stand, and at least one step rejects
    got, got_counts = draft_run(paths, prompt, ["--draft", "4", "--temperature", "0.8", "--seed", "7"])
    assert got == want and got_counts == counts


def test_a_greedy_draft_at_a_temperature_is_the_one_hot_rule(pkg, orc, setup):
    paths, prompt = setup
    want, counts = simulate(pkg, orc, paths, prompt, rng=pkg.javarand.L32X64MixRandom(7), draft=3, temperature=0.8, draft_temperature=0.0)
    got, got_counts = draft_run(paths, prompt, ["--draft", "3", "--temperature", "0.8", "--seed", "7", "--draft-temperature", "0"])
    assert got == want and got_counts == counts
