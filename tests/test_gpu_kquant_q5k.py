"""Native Q5_K storage (GL3_FLAG_KQUANT_NATIVE / _BATCH): the device requantisation of Q5_K tiles on crafted super-blocks, and whole
models through the protocols, shapes and step sizes of test_gpu_kquant_native.py and test_gpu_kquant_native_batch.py.  All exact."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import __graft_entry__ as ge
import test_gpu_kquant_native_batch as nb
from test_gpu_kquant_native import Q4_K, Q5_K, Q6_K
from test_gpu_kquant_native import test_native_kquant_plan_matches_the_oracle_on_converted_tensors as decode_case
from test_gpu_kquant_requant import D_LIST, NSB, _patterns

pytestmark = pytest.mark.gpu


def q5_k_m(name):       # Q6_K for attn_v, every second ffn_down and output
    layer = int(name.split(".")[1]) if name.startswith("blk.") else 0
    return Q6_K if ("attn_v" in name or name == "output.weight" or ("ffn_down" in name and layer % 2 == 0)) else Q5_K


def pairs(name):        # a SwiGLU pair of Q5_K gate with Q4_K up, and a qkv of Q5_K, Q4_K, Q6_K
    return Q4_K if ("ffn_up" in name or "attn_k" in name) else Q6_K if "attn_v" in name else Q5_K


BATCHED = {"q5_k_m": (0, 256, 768, 2, 8, 2, 32, q5_k_m), "q5_k_m-1536": (0, 1536, 3328, 1, 12, 2, 128, q5_k_m)}
nb.MODELS.update(BATCHED)      # nb.ref() / nb.plan_of() make the reference and the plan of a model once


def q5_k_blocks(rng):
    """q4_k_blocks' (scale, min) pairs — each of 0..63 x 0..63 through the packed decode of j < 4 and of j >= 4 — with quant patterns
    over 32 levels, every third sub-block wholly in 0..15 and every third wholly in 16..31 (fifth bits all clear / all set)."""
    n = np.arange(NSB * 8)
    pair = np.where(n < 4096, n, (n - 4096) // 8 * 8 + (n % 8 + 4) % 8) % 4096
    s, m = (pair // 64).reshape(NSB, 8), (pair % 64).reshape(NSB, 8)
    b = np.zeros((NSB, 176), np.uint8)
    i = np.arange(NSB)
    b[:, 0:2] = D_LIST[i % 5].view(np.uint8).reshape(NSB, 2)
    b[:, 2:4] = D_LIST[i // 5 % 5].view(np.uint8).reshape(NSB, 2)
    b[:, 4:8] = (s[:, :4] & 63) | ((s[:, 4:] >> 4) << 6)
    b[:, 8:12] = (m[:, :4] & 63) | ((m[:, 4:] >> 4) << 6)
    b[:, 12:16] = (s[:, 4:] & 15) | ((m[:, 4:] & 15) << 4)
    third = (n % 3)[:, None]
    q = np.where(third == 0, _patterns(rng, NSB * 8, 32), _patterns(rng, NSB * 8, 16) + 16 * (third - 1)).reshape(NSB, 4, 2, 32)
    b[:, 16:48] = ((q.reshape(NSB, 8, 32) >> 4) << np.arange(8)[None, :, None]).sum(axis=1)      # bit j of byte e: sub-block j
    b[:, 48:] = ((q[:, :, 0] & 15) | ((q[:, :, 1] & 15) << 4)).reshape(NSB, 128)
    return b


@pytest.mark.parametrize("rows", [16, 40])
def test_device_requantisation_of_q5_k_equals_the_load_time_conversion(pkg, rows):
    L = import_module(ge.PKG_NAME + ".hip").lib()
    src = np.ascontiguousarray(q5_k_blocks(np.random.default_rng(5)).reshape(-1))
    want = np.zeros(NSB * 8 * 34, np.uint8)
    got = np.zeros_like(want)
    assert L.gl3_kquant_to_q8_0(Q5_K, src.ctypes.data_as(C.c_void_p), NSB * 256, want.ctypes.data_as(C.c_void_p)) == 0
    assert L.gl3_debug_kquant_requant(0, Q5_K, src.ctypes.data_as(C.c_void_p), rows, NSB // rows * 256, got.ctypes.data_as(C.c_void_p)) == 0
    bad = np.flatnonzero((got.reshape(-1, 34) != want.reshape(-1, 34)).any(axis=1))
    assert bad.size == 0, (bad[:8], got.reshape(-1, 34)[bad[:2]], want.reshape(-1, 34)[bad[:2]])


#        id            arch dim   hidden layers heads kv hs  tied   types                 flags (1 = GL3_FLAG_NO_GRAPH)
CASES = [("q5_k_m",      0, 256,  768,  2,     8,    2, 32,  False, q5_k_m,               0),
         ("q5_k_m-eager", 0, 256, 768,  2,     8,    2, 32,  False, q5_k_m,               1),
         ("q5_k-tied",   0, 1536, 3072, 1,     12,   2, 128, True,  lambda n: Q5_K,       0),
         ("q5_k",        0, 1792, 3328, 1,     14,   2, 128, False, lambda n: Q5_K,       0),
         ("pairs",       0, 3328, 512,  1,     26,   2, 128, False, pairs,                0),
         ("phi3",        4, 256,  512,  2,     8,    8, 32,  False, lambda n: Q5_K,       0)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_single_token_decode(pkg, orc, tmp_path, case):
    decode_case(pkg, orc, tmp_path, case)      # 4 prefilled tokens, 6 decode steps, one sampled step against COracle
    if case[0] == "q5_k-tied":                 # every row count is a multiple of 16: 23.25 of Q8T's 34 bytes per block
        size = {}
        for flags in (128, 0):                 # GL3_FLAG_KQUANT_NATIVE, the default plan
            plan = import_module(ge.PKG_NAME + ".plan").HipMasterPlan.from_gguf(str(tmp_path / "kq.gguf"), flags=flags)
            size[flags] = plan.weight_bytes()
            plan.freeTornadoExecutionPlan()
        assert size[128] * 34 <= size[0] * (23.25 + 1), size


@pytest.mark.parametrize("n", [1, 17, 64, 65])
@pytest.mark.parametrize("name", BATCHED)
def test_prompt_chunk(pkg, orc, tmp_path_factory, name, n):
    nb.test_prompt_chunk(pkg, orc, tmp_path_factory, name, n)


@pytest.mark.parametrize("name", BATCHED)
def test_static_batched_decode_of_17_sequences_and_a_mixed_step(pkg, orc, tmp_path_factory, name):
    nb.test_static_batched_decode_at_mixed_depths(pkg, orc, tmp_path_factory, (name, 17, 0))
    nb.test_mixed_step_of_decode_rows_and_a_prompt_chunk(pkg, orc, tmp_path_factory, name)      # two decode rows and a 21-token chunk


def test_score_of_more_than_64_rows_through_logits_slabs(pkg, orc, tmp_path_factory, monkeypatch):
    """70 logits rows with the smallest expansion scratch: every matrix runs as row slabs through kq_expand_q8t_kernel"""
    monkeypatch.setenv("GL3_KQ_EXPAND_BYTES", "1")
    path, toks, logits, o, cfg = nb.ref("q5_k_m", pkg, orc, tmp_path_factory)
    plan = import_module(ge.PKG_NAME + ".plan").HipMasterPlan.from_gguf(path, prefill_batch_size=nb.MAXB, flags=256)
    scores, ids = plan.forward_batch_score(toks[:70], [0] * 70, range(70), toks[1:71], want_logits=[1] * 70)
    assert np.array_equal(scores["logit"], np.array([logits[p][toks[p + 1]] for p in range(70)], np.float32))
    assert ids.tolist() == [int(np.argmax(logits[p])) for p in range(70)]
    plan.freeTornadoExecutionPlan()
