"""tools/gl3_perplexity (plain C++ over the C-ABI) against llama-perplexity's protocol restated on the CPU oracle.

About 200 random ids, -c 32 -b 24 -np 3: six windows of 32 tokens (the tail is dropped), each forwarded from position 0 in a slot of its
own, the rows at positions 16 .. 30 scored against the following token; 24-row steps make windows straddle steps and several windows
share a step.  The expected numbers come from the oracle's logits with the tool's formulas: ln p = (double) (logit - max) - log((double)
sum) with the f32 (logit, max, sum) of FloatTensor.softmaxInPlace, a window's nll the sum of -ln p in position order, ppl = exp(sum of the
windows' nll / count).  log and exp are math.log / math.exp — the C library's, as in the tool — so every printed %.17g value must be
EQUAL to the Python double: no tolerance."""
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle_np

pytestmark = pytest.mark.gpu
F32 = np.float32
EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gl3_perplexity")
CTX = 32


def run(path, ids_path, extra=("-c", str(CTX), "-b", "24", "-np", "3")):
    return subprocess.run([EXE, "-m", path, "--ids", str(ids_path)] + list(extra), capture_output=True, text=True, timeout=180)


def test_perplexity_matches_the_oracle(pkg, orc, tmp_path):
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["tiny-llama"], seed=41)
    path = str(tmp_path / "m.gguf")
    m.write_gguf(path)
    ids = np.random.default_rng(43).integers(0, m.cfg.vocab, 203).tolist()
    ids_file = tmp_path / "ids.txt"
    ids_file.write_text(",".join(map(str, ids)) + "\n")
    out = run(path, ids_file)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    n_win = len(ids) // CTX
    assert n_win == 6 and len(lines) == n_win + 1
    o = orc.COracle(pkg.synth.SynthModel.from_gguf(path))
    total, count = 0.0, 0
    for k in range(n_win):
        w = ids[k * CTX:(k + 1) * CTX]
        nll, cnt = 0.0, 0
        for pos in range(CTX - 1):
            v = o.forward(w[pos], pos)                    # a new window starts at position 0 again: attention reads nothing above a row
            if pos < CTX // 2:
                continue
            mx = v.max()
            s = F32(oracle_np.seq_sum(np.exp((v - mx).astype(np.float64)).astype(F32)))
            lnp = float(F32(v[w[pos + 1]] - mx)) - math.log(float(s))
            nll += -lnp
            cnt += 1
        head, _, rest = lines[k].partition(":")
        f = rest.split()
        assert head == "window %d" % k and f[0] == "nll" and f[2] == "over", lines[k]
        assert float(f[1]) == nll and int(f[3]) == cnt == CTX - 1 - CTX // 2, (k, f[1], repr(nll))
        total += nll
        count += cnt
    f = lines[-1].split()
    assert f[0] == "ppl" and float(f[1]) == math.exp(total / count), (lines[-1], repr(math.exp(total / count)))
    assert 1.0 < float(f[1]) < 10.0 * m.cfg.vocab

    bad = tmp_path / "bad.txt"
    bad.write_text("1,2,x,4\n")
    assert run(path, bad).returncode == 2                                        # malformed ids file
    short = tmp_path / "short.txt"
    short.write_text("1,2,3\n")
    assert run(path, short).returncode == 2                                      # fewer than CTX ids
    assert run(path, ids_file, ("-c", "2", "-b", "24")).returncode == 2         # no position to score
    assert run(path, ids_file, ("-c", "32", "-b", "1")).returncode == 2
    assert run(path, ids_file, ("-c", "32", "-b", "24", "-np", "0")).returncode == 2
    assert run(path, ids_file, ("-c", "32")).returncode == 2                     # -b missing
    assert run(path, ids_file, ("-c", "32", "-b", "24", "--what")).returncode == 2
