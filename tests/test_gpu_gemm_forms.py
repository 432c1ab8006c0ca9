"""The forms of the batched-prefill GEMM stay bit-exact.  The library reads its switches once per process, so every form runs the > 64-token prefill
parity tests (ragged small shapes to the 8B / 1B layers at 512 tokens) in its own pytest subprocess.
   default                     pf_gemm3_kernel for qkv / wo / down, the tall one-round tiling (pf_gemm3t_kernel) or the 128 x 128 tiling for gate + up — normal suite
   GL3_PF_GEMM3_TALL=-1        gate + up on the 128 x 128 tiling everywhere;  =4..7 the tall tiling with that many row fragments on EVERY shape
   GL3_PF_GEMM3_TALL_KB=1      one block per K stage of the tall tiling (default: two)
   GL3_PF_GEMM3_SHAPE=1|2|3|4  128 x 128 / 96 x 128 / 64 x 128 / 64 x 64 workgroup tiles for every non-SwiGLU projection
   GL3_PF_GEMM3_QOUT=0         hb leaves the tall tiling as f32 and is quantised by its own launch
test_gemm3_grid_rows_under_a_form repeats rows of the grid of tests/gemm3_shapes.py (every chunk row compared) under these switches.
These tilings are what different matrix shapes take by default; the switches force each of them onto the test shapes.  The prefill attention has
its own forms (test_prefill_attention_forms), and so has the static-batched decode step (test_static_batched_decode_forms:
GL3_NO_FUSED_BD_ATTN / GL3_NO_FUSED_QUANT)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("env", [{"GL3_PF_GEMM3_TALL": "-1"}, {"GL3_PF_GEMM3_TALL": "4"}, {"GL3_PF_GEMM3_TALL": "5", "GL3_PF_GEMM3_TALL_KB": "1"},
                                 {"GL3_PF_GEMM3_TALL": "7", "GL3_PF_GEMM3_SHAPE": "1"}, {"GL3_PF_GEMM3_TALL": "6", "GL3_PF_GEMM3_SHAPE": "2"}],
                         ids=["g3-128x128", "tall4", "tall5-one-block-stages", "tall7-shape1", "tall6-shape2"])
def test_prefill_parity_of_a_gemm_form(env):
    e = dict(os.environ, **env)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_decode.py"), os.path.join(ROOT, "tests", "test_gpu_fullsize.py"),
                          "-m", "gpu", "-x", "-q", "-k", "chunks_above_64 or prefill512", "-p", "no:cacheprovider"],
                         capture_output=True, text=True, timeout=800, env=e, cwd=ROOT)
    tail = out.stdout[-1500:] + out.stderr[-500:]
    assert out.returncode == 0, tail
    assert " passed" in out.stdout and "failed" not in out.stdout, tail


G3_FORMS = [{"GL3_PF_GEMM3_TALL": "4"}, {"GL3_PF_GEMM3_TALL_KB": "1"}, {"GL3_PF_GEMM3_TALL": "-1"}, {"GL3_PF_GEMM3_SHAPE": "1"}, {"GL3_PF_GEMM3_SHAPE": "2"},
            {"GL3_PF_GEMM3_SHAPE": "3"}, {"GL3_PF_GEMM3_SHAPE": "4"}, {"GL3_PF_GEMM3_QOUT": "0"}, {"GL3_PF_GEMM3_TALL": "6", "GL3_PF_GEMM3_TALL_KB": "1"}]


@pytest.mark.parametrize("env", G3_FORMS, ids=["-".join("%s=%s" % (k[13:].lower(), v) for k, v in e.items()) for e in G3_FORMS])
def test_gemm3_grid_rows_under_a_form(env):
    """FORM_ROWS of tests/gemm3_shapes.py (every row of a chunk, K / V of every row, the step behind; logits of every flagged row) under a
    tiling the grid's defaults do not reach on those shapes: GL3_PF_GEMM3_TALL=4 is the only way NFR 4 runs, and the only way the tall
    kernel meets a single token tile (65, 97 tokens), fewer rows than one tile (hidden 96) and K of one block; TALL_KB=1 the one-block
    stages on the default NFR 5 (and NFR 6 everywhere); TALL=-1 the 128 x 128 SwiGLU tiling at hidden 8224; SHAPE=1 the 128 x 128 tile on
    the residual epilogue (its only run, with every token tail: gemm3_shapes.FORM_ROWS says why), =2 the 96 x 128 tile on row counts 96 does not divide, =3 64 x 128 where 96 x 128 is the default, =4 the
    64 x 64 tile with its own token tiling; QOUT=0 the f32 hb behind the tall kernel."""
    import gemm3_shapes as gs
    select = " or ".join("%s]" % r for r in gs.FORM_ROWS)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_gemm3_shapes.py"), "-m", "gpu", "-x", "-q", "-k", select,
                          "-p", "no:cacheprovider"], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env), cwd=ROOT)
    tail = out.stdout[-1500:] + out.stderr[-500:]
    assert out.returncode == 0, tail
    assert "%d passed" % len(gs.FORM_ROWS) in out.stdout and "failed" not in out.stdout and "skipped" not in out.stdout, tail


@pytest.mark.parametrize("env,select", [
    ({"GL3_PF_FUSED_ATTN": "0"}, "chunks_above_64 or prefill512 or long_context_prefill or behind_1000 or batched_prefill_is_bit"),
    ({"GL3_PF_FUSED_ATTN": "0", "GL3_PF_SCORES_MFMA": "0", "GL3_PF_PV_MFMA": "0"}, "chunks_above_64 or long_context_prefill or behind_1000"),
    ({"GL3_PF_FUSED_ATTN": "0", "GL3_PF_SCORES_MFMA": "0", "GL3_PF_SCORES_PK": "0", "GL3_PF_PV_MFMA": "0"}, "chunks_above_64 or long_context_prefill"),
    ({"GL3_PF_FUSED_MFMA": "0"}, "chunks_above_64 or llama3_8b_shaped_layer_prefill512"),
    ({"GL3_PF_FUSED_V1": "1"}, "chunks_above_64 or long_context_prefill")],
    ids=["three-kernels", "three-kernels-valu-packed", "three-kernels-valu-scalar", "one-launch-valu-packed", "one-launch-r4"])
def test_prefill_attention_forms(env, select):
    """The forms of the prefill attention stay bit-exact, each in its own process (switches are read once):
       default                      one launch with MFMA products (pf_attn_fused3_kernel) while a tile's score rows fit LDS, else pf_scores_mfma_kernel ->
                                    pf_softmax_rows_kernel -> pf_pv_mfma_kernel (kvMul 4, head size 128 / 64; other shapes: the VALU kernels)
       GL3_PF_FUSED_ATTN=0          the three kernels from position 0
       GL3_PF_SCORES_MFMA=0 / GL3_PF_PV_MFMA=0     packed-f32 VALU products (pf_scores_pk_kernel, pf_pv_ring_kernel); + GL3_PF_SCORES_PK=0: the scalar
                                    scores kernel (pf_scores_tiled_kernel) with pf_pv_ring_kernel
       GL3_PF_FUSED_MFMA=0 / GL3_PF_FUSED_V1=1     the one-launch kernel with packed-f32 VALU products (fused2) / the r4 kernel
    Ragged chunks, chunks at non-zero positions, the 8B / 1B layers at 512 tokens and behind 1000 positions."""
    e = dict(os.environ, **env)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_decode.py"), os.path.join(ROOT, "tests", "test_gpu_fullsize.py"),
                          "-m", "gpu", "-x", "-q", "-k", select, "-p", "no:cacheprovider"],
                         capture_output=True, text=True, timeout=900, env=e, cwd=ROOT)
    tail = out.stdout[-1500:] + out.stderr[-500:]
    assert out.returncode == 0, tail
    assert " passed" in out.stdout and "failed" not in out.stdout, tail


@pytest.mark.parametrize("env", [{"GL3_NO_FUSED_BD_ATTN": "1"}, {"GL3_NO_FUSED_QUANT": "1"}, {"GL3_NO_FUSED_BD_ATTN": "1", "GL3_NO_FUSED_QUANT": "1"}],
                         ids=["three-kernel-attention", "separate-quantise-launches", "both"])
def test_static_batched_decode_forms(env):
    """The A/B forms of the static-batched decode step stay bit-exact, each in its own process (switches are read once):
       default                      attn_head_kernel below 128 positions, with the attention output and hb written as the next GEMM's int8 operand
       GL3_NO_FUSED_BD_ATTN=1       pf_rope_kv_kernel -> pf_attn_scores_kernel -> pf_attn_softmax_pv_kernel from position 0: the only way the suite
                                    runs them on shallow rows (and with every row of a step below 128)
       GL3_NO_FUSED_QUANT=1         the separate quantise launches (pf_norm_quant_kernel<PQ_PLAIN>) behind attention and gate + up, at every batch size
    Runs the depth / mixed-depth / tile-class / windowed / sampler tests of test_gpu_batch_decode_depth.py and the static-batched tests of test_gpu_decode.py."""
    e = dict(os.environ, **env)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_batch_decode_depth.py"), os.path.join(ROOT, "tests", "test_gpu_decode.py"),
                          "-m", "gpu", "-x", "-q", "-k", "batch_decode_depth or static_batched", "-p", "no:cacheprovider"],
                         capture_output=True, text=True, timeout=850, env=e, cwd=ROOT)
    tail = out.stdout[-1500:] + out.stderr[-500:]
    assert out.returncode == 0, tail
    assert " passed" in out.stdout and "failed" not in out.stdout and "skipped" not in out.stdout, tail
