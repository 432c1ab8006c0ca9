"""tools/gl3_spec_draft_run --chain: the drafts of a speculation step and their puts as ONE gl3_forward_decode_chain on the draft plan.  The chain
carries the same coins in the same order, so the ids on stdout and the steps / drafted / accepted / tokens line on stderr are those of the run
without --chain, greedy and at a temperature; the greedy ids are tools/gl3_run's."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "gl3_spec_draft_run")
RUN = os.path.join(ROOT, "tools", "gl3_run")
NEW, BATCH = 24, 8


def draft_run(paths, prompt, extra):
    """-> (ids, the counts line)"""
    out = subprocess.run([EXE, "-m", paths[0], "-md", paths[1], "--ids", ",".join(map(str, prompt)), "-b", str(BATCH), "-n", str(NEW)] + extra,
                         capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stderr
    lines = [l for l in out.stderr.splitlines() if l.startswith("steps=")]
    assert len(lines) == 1 and any(l.startswith("timing: ") and " draft_ms=" in l for l in out.stderr.splitlines()), out.stderr
    return [int(x) for x in out.stdout.split("generated:")[1].split()], lines[0]


@pytest.fixture(scope="module")
def setup(pkg, tmp_path_factory):
    cfg = pkg.synth.CONFIGS["tiny-llama"]
    d = tmp_path_factory.mktemp("spec_draft_chain")
    paths = [str(d / "target.gguf"), str(d / "draft.gguf")]
    pkg.synth.make_numpy(cfg, seed=85).write_gguf(paths[0])
    pkg.synth.make_numpy(dataclasses.replace(cfg, n_layers=1), seed=86).write_gguf(paths[1])
    return paths, np.random.default_rng(85).integers(0, cfg.vocab, 7).tolist()


def test_greedy_chain_run_is_the_run_without_it_and_gl3_run(setup):
    paths, prompt = setup
    for draft in ("2", "4"):
        plain = draft_run(paths, prompt, ["--draft", draft])
        chained = draft_run(paths, prompt, ["--draft", draft, "--chain"])
        assert chained == plain and len(plain[0]) == NEW and " drafted=0 " not in plain[1], (draft, plain, chained)
    out = subprocess.run([RUN, "-m", paths[0], "--protocol", "llama", "--bos", str(prompt[0]), "--ids", ",".join(map(str, prompt[1:])),
                          "-n", str(len(prompt) - 1 + NEW)], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stderr
    assert [int(x) for x in out.stdout.split("generated:")[1].split()] == chained[0]


@pytest.mark.parametrize("draft", ["2", "4"])
def test_sampled_chain_run_is_the_run_without_it(setup, draft):
    paths, prompt = setup
    args = ["--draft", draft, "--temperature", "0.8", "--seed", "7"]
    plain = draft_run(paths, prompt, args)
    chained = draft_run(paths, prompt, args + ["--chain"])
    assert chained == plain and len(plain[0]) == NEW and " accepted=0 " not in plain[1], (plain, chained)
