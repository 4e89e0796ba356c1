"""CPU checks of the soft-output definition (rub_mimo_amd/soft.py, DESIGN.md "Soft output"):
the per-dimension max-log LLR against brute force over the constellation, the post-detection
MSE on the golden fixtures' own estimates, and the C-ABI's argument errors. No GPU calls."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import ref
from rub_mimo_amd import _lib, soft

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def brute_force_llr(y, order):
    """Max-log LLRs by definition: over all order points, bit i of the index from its MSB."""
    nb = soft.qam_bits(order) * 2
    pts = np.array([ref.qam_point(i, order) for i in range(order)], np.complex128)
    d2 = np.abs(np.asarray(y, np.complex128)[:, None] - pts[None, :]) ** 2
    idx = np.arange(order)
    out = np.empty((len(y), nb))
    for i in range(nb):
        one = ((idx >> (nb - 1 - i)) & 1) == 1
        out[:, i] = d2[:, one].min(axis=1) - d2[:, ~one].min(axis=1)
    return out


@pytest.mark.parametrize("order", [4, 16, 64, 256])
def test_llr_reference_matches_brute_force(order):
    rng = np.random.default_rng(order)
    lv = soft.qam_levels(order)
    n = 4096
    # inside and well outside the grid; the first points exactly on a level in one or both
    # dimensions (values a float32 holds, as qam_demap reads them)
    y = (rng.uniform(-1.6, 1.6, n) + 1j * rng.uniform(-1.6, 1.6, n)) * (lv[-1] + 0.3)
    y[:256] = rng.choice(lv, 256) + 1j * y[:256].imag
    y[128:384] = y[128:384].real + 1j * rng.choice(lv, 256)
    y = y.astype(np.complex64).astype(np.complex128)
    assert np.any(np.abs(y.real) > lv[-1] * 1.2) and np.any(np.abs(y.imag) > lv[-1] * 1.2)
    nu = rng.uniform(1e-4, 1.0, n)
    got = soft.llr_reference(y, nu, order, llr_scale=0.7)
    want = 0.7 * brute_force_llr(y, order) / nu[:, None]
    assert got.shape == (n, 2 * soft.qam_bits(order))
    assert np.all(np.abs(got - want) <= 1e-9 * (1.0 + np.abs(want)))
    # the levels are the oracle's constellation
    b = soft.qam_bits(order)
    pts = np.array([ref.qam_point(i, order) for i in range(order)])
    assert np.allclose(np.unique(np.round(pts.real, 6)), np.round(lv, 6), atol=1e-6)
    # sign rule: a non-zero LLR's sign is the hard decision's bit (positive = 0)
    hard = np.array([ref.qam_demap(complex(v), order) for v in y])
    for i in range(2 * b):
        bit = (hard >> (2 * b - 1 - i)) & 1
        nz = got[:, i] != 0
        assert np.array_equal(got[nz, i] < 0, bit[nz] == 1), i


def test_llr_reference_nan_and_floor():
    y = np.array([np.nan + 0.1j, 0.3 - 0.2j])
    out = soft.llr_reference(y, np.array([1.0, 0.0]), 16)
    assert np.all(out[0, :2] == 0.0) and np.all(out[0, 2:] != 0.0)
    assert np.all(np.abs(out[1]) > 1e28)      # nu floored at 1e-30, not a division by zero


@pytest.mark.parametrize("name", ["m128_4x4_mmse", "m256_8x8_mmse"])
def test_mse_reference_is_the_mmse_error_covariance(name):
    """For MMSE weights nu = s2 diag((G^H G + s2 I)^-1). The fixture's W is the fp32 rounding
    of an fp64 solve (relative error 6e-8 per entry) and nu is quadratic in it, so 1e-3 of the
    peak leaves three orders of margin."""
    g = load(name)
    occ = np.flatnonzero(g["p"] != 0)
    s2 = float(g["noise_var"])
    nu = soft.mse_reference(g["G"], g["W"], g["gain"], s2, occ)
    G = g["G"].astype(np.complex128)[occ]
    N = G.shape[-1]
    A = np.conj(G.transpose(0, 2, 1)) @ G + s2 * np.eye(N)
    want = s2 * np.real(np.diagonal(np.linalg.inv(A), axis1=1, axis2=2)).T
    assert nu.shape == want.shape == (N, len(occ))
    assert np.abs(nu - want).max() <= 1e-3 * nu.max()


@pytest.mark.parametrize("name", ["m64_2x2_zf2", "m64_1x1_zf"])
def test_zero_forcing_leaves_no_interference(name):
    g = load(name)
    occ = np.flatnonzero(g["p"] != 0)
    noise, isi = soft.mse_terms(g["G"], g["W"], g["gain"], float(g["noise_var"]), occ)
    assert np.all(noise > 0)
    assert np.all(isi <= 1e-6 * noise)


def test_null_handles_are_argument_errors():
    L = _lib.lib()
    a = _lib.SoftDemap(16, 16, 1, 1, 0, _lib.LLR_I8, 1.0)
    assert L.mimo_rx_soft_demap(None, C.byref(a), None) == -1
    buf = (C.c_float * 4)()
    assert L.mimo_rx_batch_mse(None, C.cast(buf, C.c_void_p), 1) == -1
    assert _lib.LLR_I8 == 0 and _lib.LLR_F32 == 1


def test_quantise_i8_rounds_half_to_even_and_saturates():
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, 127.5, 1e9, -1e9, np.inf, -np.inf,
                  0.49, -3.7], np.float32)
    want = np.array([0, 2, 2, 0, -2, -2, 126, 127, 127, -127, 127, -127, 0, -4], np.int8)
    got = soft.quantise_i8(v)
    assert got.dtype == np.int8 and np.array_equal(got, want)
