"""tools/gl3_spec_run (plain C++ over the C-ABI: prompt-lookup drafts, one gl3_forward_batch_verify per step) on a tiny synthetic GGUF with
a repetitive prompt: it prints exactly the ids of plain greedy decoding — the CPU oracle's and tools/gl3_run's — and its step / draft /
accept counts are those of the drafting rule replayed over the oracle's ids (verify_ref.simulate_spec_run, a pure function of ids)."""
import os
import re
import subprocess

import numpy as np
import pytest

import verify_ref as vr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "gl3_spec_run")
RUN = os.path.join(ROOT, "tools", "gl3_run")
# Chosen on the CPU oracle: the prompt is a 5-id unit repeated, followed by the first PRE ids of this model's own greedy continuation, so the
# ids generated behind it are in the history (draftable at their first generated occurrence) and still break the history's patterns.
SEED, PRE, NEW, BATCH = 81, 16, 28, 8


def spec_run(path, prompt, extra):
    out = subprocess.run([EXE, "-m", path, "--ids", ",".join(map(str, prompt)), "-b", str(BATCH)] + extra, capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stderr
    lines = [l for l in out.stderr.splitlines() if l.startswith("steps=")]
    assert len(lines) == 1, out.stderr
    counts = tuple(int(re.search(r"\b%s=(\d+)" % k, lines[0]).group(1)) for k in ("steps", "drafted", "accepted", "tokens"))
    return [int(x) for x in out.stdout.split("generated:")[1].split()], counts


@pytest.fixture(scope="module")
def setup(pkg, orc, tmp_path_factory):
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["tiny-llama"], seed=SEED)
    path = str(tmp_path_factory.mktemp("spec") / "m.gguf")
    m.write_gguf(path)
    unit = np.random.default_rng(SEED).integers(0, m.cfg.vocab, 5).tolist()
    base = unit * 3 + unit[:2]
    o = orc.COracle(pkg.synth.SynthModel.from_gguf(path))
    o.prefill(base[:-1], 0)
    ids, tok = [], base[-1]
    for i in range(PRE + NEW):
        tok = orc.argmax(o.forward(tok, len(base) - 1 + i))
        ids.append(tok)
    return path, base + ids[:PRE], ids[PRE:]


def test_speculative_greedy_ids_are_the_plain_greedy_ids(setup):
    path, prompt, greedy = setup
    want, steps, drafted, accepted = vr.simulate_spec_run(prompt, greedy, NEW, draft=4, ngram=3, batch=BATCH)
    assert want == greedy and accepted > 0 and drafted > accepted and steps < NEW      # drafts stand, and at least one step rejects
    got, counts = spec_run(path, prompt, ["-n", str(NEW), "--draft", "4"])
    assert got == greedy
    assert counts == (steps, drafted, accepted, NEW)
    # the same (token, position) sequence through tools/gl3_run: its begin-of-text slot holds the first prompt id
    out = subprocess.run([RUN, "-m", path, "--protocol", "llama", "--bos", str(prompt[0]), "--ids", ",".join(map(str, prompt[1:])),
                          "-n", str(len(prompt) - 1 + NEW)], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stderr
    assert [int(x) for x in out.stdout.split("generated:")[1].split()] == got


def test_draft_0_and_other_draft_lengths(setup):
    path, prompt, greedy = setup
    got, counts = spec_run(path, prompt, ["-n", str(NEW), "--draft", "0"])
    assert got == greedy and counts == (NEW, 0, 0, NEW)                   # plain decoding through the same entry: one id per step
    want = vr.simulate_spec_run(prompt, greedy, NEW, draft=7, ngram=2, batch=BATCH)
    got, counts = spec_run(path, prompt, ["-n", str(NEW), "--draft", "7", "--ngram", "2"])
    assert got == greedy and counts == want[1:] + (NEW,)


def test_a_stop_id_ends_generation_inside_accepted_drafts(setup):
    path, prompt, greedy = setup
    chosen = None
    for j, x in enumerate(greedy):                                       # a stop id whose first occurrence has accepted drafts behind it
        if greedy.index(x) != j:
            continue
        gen, steps, drafted, accepted = vr.simulate_spec_run(prompt, greedy, NEW, draft=4, ngram=3, batch=BATCH, stop={x})
        assert gen == greedy[:j + 1]
        if accepted + steps > len(gen):
            chosen = (x, gen, (steps, drafted, accepted, len(gen)))
            break
    assert chosen is not None
    x, gen, want = chosen
    got, counts = spec_run(path, prompt, ["-n", str(NEW), "--draft", "4", "--stop", "%d,%d" % (x, 999999)])
    assert got == gen and got[-1] == x and counts == want
