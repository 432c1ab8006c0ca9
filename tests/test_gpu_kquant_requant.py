"""The decode matvec's device requantisation of native Q4_K / Q6_K tiles (GL3_FLAG_KQUANT_NATIVE: repack at upload, then the Q8_0
block rebuilt in registers) against the load-time conversion gl3_kquant_to_q8_0, byte for byte, on crafted super-blocks."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

NSB = 1040                                                     # super-blocks: 16 rows x 65, or 40 rows (a padded strip) x 26
# f16 d / dmin: typical, 0, negative, the third f16 subnormal, 65504
D_LIST = np.array([0x2A4C, 0x0000, 0x9F45, 0x0003, 0x7BFF], np.uint16)


def _patterns(rng, n_sub, levels):
    """[n_sub, 32] quant values: every level present / one value / only the two extremes / a random sub-range, in rotation."""
    q = np.empty((n_sub, 32), np.int64)
    for n in range(n_sub):
        kind = n % 4
        if kind == 0:
            q[n] = rng.permutation(np.arange(max(32, levels)) % levels)[:32]      # 16 levels: all of them; 64: 32 distinct ones
        elif kind == 1:
            q[n] = (0, levels - 1, n // 4 % levels)[n // 4 % 3]
        elif kind == 2:
            q[n] = rng.integers(0, 2, 32) * (levels - 1)
        else:
            lo = rng.integers(0, levels)
            q[n] = rng.integers(lo, rng.integers(lo, levels) + 1, 32)
    return q


def q4_k_blocks(rng):
    """Every (scale, min) pair of 0..63 x 0..63 twice, the second time four sub-block positions on, so that each pair goes through the
    packed 12-byte decode of j < 4 and of j >= 4."""
    n = np.arange(NSB * 8)
    pos = n % 8
    pair = np.where(n < 4096, n, (n - 4096) // 8 * 8 + (pos + 4) % 8) % 4096
    s, m = (pair // 64).reshape(NSB, 8), (pair % 64).reshape(NSB, 8)
    b = np.zeros((NSB, 144), np.uint8)
    i = np.arange(NSB)
    b[:, 0:2] = D_LIST[i % 5].view(np.uint8).reshape(NSB, 2)
    b[:, 2:4] = D_LIST[i // 5 % 5].view(np.uint8).reshape(NSB, 2)
    b[:, 4:8] = (s[:, :4] & 63) | ((s[:, 4:] >> 4) << 6)
    b[:, 8:12] = (m[:, :4] & 63) | ((m[:, 4:] >> 4) << 6)
    b[:, 12:16] = (s[:, 4:] & 15) | ((m[:, 4:] & 15) << 4)
    q = _patterns(rng, NSB * 8, 16).reshape(NSB, 4, 2, 32)     # sub-block 2p = low nibbles, 2p + 1 = high nibbles of bytes 32p ..
    b[:, 16:] = (q[:, :, 0] | (q[:, :, 1] << 4)).reshape(NSB, 128)
    return b


def q6_k_blocks(rng):
    """All 256 int8 scales, neighbouring sub-blocks (the two halves of a 32-block) 37 apart; every level, only -32, only 31."""
    b = np.zeros((NSB, 210), np.uint8)
    i = np.arange(NSB)
    b[:, 192:208] = (16 * i[:, None] + 37 * np.arange(16)[None, :] + i[:, None] // 16) & 255
    b[:, 208:210] = D_LIST[i % 5].view(np.uint8).reshape(NSB, 2)
    q = _patterns(rng, NSB * 8, 64).reshape(NSB, 2, 4, 32)     # [half][group][element]
    lo, hi = q & 15, q >> 4
    b[:, 0:128] = np.concatenate([lo[:, :, 0] | (lo[:, :, 2] << 4), lo[:, :, 1] | (lo[:, :, 3] << 4)], axis=2).reshape(NSB, 128)
    b[:, 128:192] = (hi[:, :, 0] | (hi[:, :, 1] << 2) | (hi[:, :, 2] << 4) | (hi[:, :, 3] << 6)).reshape(NSB, 64)
    return b


@pytest.mark.parametrize("rows", [16, 40])
@pytest.mark.parametrize("ggml_type, make", [(12, q4_k_blocks), (14, q6_k_blocks)], ids=["q4_k", "q6_k"])
def test_device_requantisation_equals_the_load_time_conversion(pkg, ggml_type, make, rows):
    L = import_module(ge.PKG_NAME + ".hip").lib()
    src = np.ascontiguousarray(make(np.random.default_rng(5)).reshape(-1))
    k = NSB // rows * 256
    want = np.zeros(NSB * 8 * 34, np.uint8)
    got = np.zeros_like(want)
    assert L.gl3_kquant_to_q8_0(ggml_type, src.ctypes.data_as(C.c_void_p), NSB * 256, want.ctypes.data_as(C.c_void_p)) == 0
    assert L.gl3_debug_kquant_requant(0, ggml_type, src.ctypes.data_as(C.c_void_p), rows, k, got.ctypes.data_as(C.c_void_p)) == 0
    bad = np.flatnonzero((got.reshape(-1, 34) != want.reshape(-1, 34)).any(axis=1))
    assert bad.size == 0, (bad[:8], got.reshape(-1, 34)[bad[:2]], want.reshape(-1, 34)[bad[:2]])
