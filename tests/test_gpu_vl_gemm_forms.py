"""The forms of the batched Q4_0 / Q8_0-f32act GEMM stay bit-exact, each in its own pytest process (the library reads its switches once):
   default                      gemm_vlq_mfma_kernel<.., 4> with vqm_tile_of from 192 tiles of 64 x 64, gemm_vlq_kernel below — normal suite
   GL3_VLQ_MFMA=0               gemm_vlq_kernel at every size
   GL3_VQM_XCD_TOKENS=0         the matrix-pipe kernel on vl_tile_of
   GL3_VQM_OCC2=1               its 143-register build, one workgroup per CU
   GL3_VLQ_MFMA_MIN_TILES=1     the matrix-pipe kernel for every launch of more than 16 tokens: the small shapes of the older tests, and the
                                edge VALUES of tests/edge_models.py (subnormal / zero / negative / 2^15 block scales, quants at their bounds, zero
                                and subnormal-scaled activations), reach the K = 1 f32 MFMA products.  A step of at most 16 tokens still stays on
                                gemm_vlq_kernel under this switch: that is the rule (ntok > VLQ_TOK comes first), so of the edge models' launches
                                the chunks [37, 20] move to the matrix pipe and the 5-row static-batched step does not."""
import os
import subprocess
import sys

import pytest

import vl_gemm_shapes as vs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")


def run(files, select, env, timeout):
    out = subprocess.run([sys.executable, "-m", "pytest"] + [os.path.join(TESTS, f) for f in files] + ["-m", "gpu", "-x", "-q", "-k", select, "-p", "no:cacheprovider"],
                         capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **env), cwd=ROOT)
    tail = out.stdout[-1500:] + out.stderr[-500:]
    assert out.returncode == 0, tail
    assert " passed" in out.stdout and "failed" not in out.stdout and "skipped" not in out.stdout, tail
    return out.stdout


@pytest.mark.parametrize("env", [{"GL3_VLQ_MFMA": "0"}, {"GL3_VQM_XCD_TOKENS": "0"}, {"GL3_VQM_OCC2": "1"}], ids=["valu-only", "vl_tile_of", "occ2"])
def test_grid_rows_under_a_form(env):
    """One step per case that takes the matrix-pipe kernel by default (resid 193, store 193, g8 449, rows 33 and 65), both block formats"""
    select = "(%s) and (q4v256 or q8f32)" % " or ".join("%s-q" % r for r in vs.FORM_ROWS)
    out = run(["test_gpu_vl_gemm_shapes.py"], select, env, 600)
    assert "%d passed" % (len(vs.FORM_ROWS) * 2 * 2) in out, out[-1500:]      # two weight types, the descending and the ascending leg


@pytest.mark.parametrize("files,select,count", [
    (["test_gpu_value_edges.py"], "test_other_weight_types and (q4_0-v256 or q8_0-f32act)", 4),
    (["test_gpu_decode.py"], "test_batched_prefill_of_the_f32_activation_types or test_static_batched_decode_of_the_f32_activation_types", 13)],
    ids=["edge-values", "older-shapes"])
def test_older_tests_on_the_matrix_pipe(files, select, count):
    """GL3_VLQ_MFMA_MIN_TILES=1 (see above): the "all" edge models of both block formats, and the batched prefill / static-batched decode
    tests of the f32-activation types, unedited"""
    out = run(files, select, {"GL3_VLQ_MFMA_MIN_TILES": "1"}, 600)
    assert "%d passed" % count in out, out[-1500:]
