"""exact_seqsum_lds (csrc/gl3_seqsum.h) through gl3_debug_sumsq at the ends of its range, one quad either side of 4096 and a length whose
last threads' segments are partly padding, bit for bit against the NumPy sequential chain of tests/test_gpu_seqsum.py.  The inputs aim at
the straight-line translation and list phases: a binade crossing in the first segment of every fourth thread (64 hard segments spread over
all four wavefronts), a rounding tie at every add, one giant element, all zeros."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
from test_gpu_seqsum import seq_sumsq

pytestmark = pytest.mark.gpu

LENGTHS = (1024, 1028, 2048, 4092, 4096, 4100, 5120)


def binade_steps(n):
    """Squares 2^-60 everywhere; at the second element of 64 evenly spread quads a spike whose square is about the sum of all spikes before
    it, so the running sum enters a new binade inside that quad (the first segment of a thread at every length of LENGTHS but the ragged
    ones, where it is the first or second)."""
    x = np.full(n, 2.0 ** -30, np.float32)
    for j in range(64):
        x[(j * n // 64) // 4 * 4 + 1] = np.float32(2.0 ** ((j - 20) / 2.0))
    return x


def inputs(n):
    rng = np.random.default_rng(n)
    yield "gaussian", rng.standard_normal(n).astype(np.float32)
    yield "binade-steps", binade_steps(n)
    x = np.ones(n, np.float32); x[0] = 4096.0              # 2^24 + 1: half an ulp, a tie at every add
    yield "pow2-ties", x
    x = np.full(n, 2.0 ** -60, np.float32); x[n // 3] = 2.0 ** 60
    yield "one-giant", x
    yield "zeros", np.zeros(n, np.float32)


@pytest.mark.parametrize("n", LENGTHS)
def test_exact_sum_at_range_ends_and_ragged_lengths(pkg, n):
    from importlib import import_module
    L = import_module(ge.PKG_NAME + ".hip").lib()
    out = C.c_float()
    for name, x in inputs(n):
        x = np.ascontiguousarray(x, np.float32)
        assert L.gl3_debug_sumsq(0, x.ctypes.data_as(C.c_void_p), x.size, C.byref(out)) == 0
        ref = seq_sumsq(x)
        assert np.float32(out.value).view(np.uint32) == np.float32(ref).view(np.uint32), (name, n, out.value, float(ref))
