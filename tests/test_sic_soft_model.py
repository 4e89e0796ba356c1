"""CPU checks of the soft-output SIC definition (rub_mimo_amd/sic.py sic_llr, DESIGN.md
"Soft-output SIC"): the sign rule against the slicer, stage 0 against the linear soft output,
brute force over the oracle's constellation, the failed-solve and s2 = 0 cases, and the C-ABI's
struct and null arguments. No GPU calls."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import ref
from rub_mimo_amd import _lib, sic, soft

ORDERS = [4, 16, 64, 256]


def rand_z(rng, order, n):
    """Points inside and well outside the grid, some exactly on a level, as float32 holds them."""
    lv = soft.qam_levels(order)
    z = (rng.uniform(-1.6, 1.6, n) + 1j * rng.uniform(-1.6, 1.6, n)) * (lv[-1] + 0.3)
    z[:64] = rng.choice(lv, 64) + 1j * z[:64].imag
    z[32:96] = z[32:96].real + 1j * rng.choice(lv, 64)
    return z.astype(np.complex64).astype(np.complex128)


@pytest.mark.parametrize("order", ORDERS)
def test_sign_of_a_nonzero_llr_is_the_bit_of_the_slicer(order):
    rng = np.random.default_rng(100 + order)
    z = rand_z(rng, order, 4096)
    nu = rng.uniform(1e-4, 1.0, z.shape)
    llr = sic.sic_llr(z, nu, order, llr_scale=0.3)
    nb = 2 * soft.qam_bits(order)
    assert llr.shape == z.shape + (nb,)
    idx = sic.qam_demap_f32(z, order).astype(np.int64)
    assert len(np.unique(idx)) > 1
    for i in range(nb):
        bit = (idx >> (nb - 1 - i)) & 1
        nz = llr[:, i] != 0
        assert np.array_equal(llr[nz, i] < 0, bit[nz] == 1), i


@pytest.mark.parametrize("order", ORDERS)
def test_sic_llr_matches_brute_force_over_the_oracle_constellation(order):
    rng = np.random.default_rng(200 + order)
    z = rand_z(rng, order, 2048)
    nu = rng.uniform(1e-4, 1.0, z.shape)
    nb = 2 * soft.qam_bits(order)
    pts = np.array([ref.qam_point(i, order) for i in range(order)], np.complex128)
    d2 = np.abs(z[:, None] - pts[None, :]) ** 2
    idx = np.arange(order)
    want = np.empty((len(z), nb))
    for i in range(nb):
        one = ((idx >> (nb - 1 - i)) & 1) == 1
        want[:, i] = 0.7 * (d2[:, one].min(axis=1) - d2[:, ~one].min(axis=1)) / nu
    got = sic.sic_llr(z, nu, order, llr_scale=0.7)
    assert np.all(np.abs(got - want) <= 1e-9 * (1.0 + np.abs(want)))


@pytest.mark.parametrize("N,order", [(2, 4), (3, 16), (4, 64), (8, 256)])
def test_mmse_stage0_is_the_linear_soft_output_of_the_unbiased_symbol(N, order):
    """MMSE stage 0 is z = y_(pi_0) / beta_0 with nu_sic = (1 - beta_0) / beta_0: sic_llr of the
    model's own z and nu_sic equals llr_reference of y / beta_0 with that MSE, to 1e-12 of the
    LLR's terms: the numerator is a difference of squares of size A^2, A = max(|x|, l_max), so
    the bound is 1e-12 (|LLR| + llr_scale A^2 / nu), x the part of z the bit depends on."""
    rng = np.random.default_rng(300 + N)
    J, n, s2 = 48, 6, 0.03
    G = rng.standard_normal((J, N, N)) + 1j * rng.standard_normal((J, N, N))
    order_, T, Ct, nu = sic.sic_tables(G, s2, s2)
    y = (rng.standard_normal((N, n, J)) + 1j * rng.standard_normal((N, n, J))) * 0.7
    z, _ = sic.sic_apply(y, order_, T, Ct, order)
    ar = np.arange(J)
    pi0 = order_[:, 0].astype(np.int64)
    Q = np.conj(G.transpose(0, 2, 1)) @ G
    E = np.linalg.inv(Q + s2 * np.eye(N))
    beta = 1.0 - s2 * np.real(E[ar, pi0, pi0])                    # [J]
    got = sic.sic_llr(z[pi0, :, ar], nu[ar, pi0][:, None], order, llr_scale=0.5)
    want = soft.llr_reference(y[pi0, :, ar] / beta[:, None], ((1.0 - beta) / beta)[:, None],
                              order, llr_scale=0.5)
    b = soft.qam_bits(order)
    assert got.shape == (J, n, 2 * b)
    zz = y[pi0, :, ar] / beta[:, None]
    lmax = soft.qam_levels(order)[-1]
    A = np.concatenate([np.repeat(np.maximum(np.abs(zz.real), lmax)[..., None], b, -1),
                        np.repeat(np.maximum(np.abs(zz.imag), lmax)[..., None], b, -1)], -1)
    term = 0.5 * A ** 2 / ((1.0 - beta) / beta)[:, None, None]
    assert np.all(np.abs(got - want) <= 1e-12 * (np.abs(want) + term))
    assert np.all(np.abs(want).max(axis=-1) > 0)


def test_a_singular_carrier_gives_zeros_and_a_noiseless_one_takes_the_floor():
    G = np.zeros((3, 2, 2), np.complex128)
    G[0] = [[1, 0.5], [0.2, 1]]
    G[2] = [[1, 0.1], [0.3, -1]]
    order, T, Ct, nu = sic.sic_tables(G, 0.0, 0.0)      # carrier 1: Q = 0, s2 = 0
    failed = sic.failed_carriers(T)
    assert np.array_equal(failed, [False, True, False])
    assert np.all(nu == 0.0)                            # good carriers too: s2 = 0
    rng = np.random.default_rng(7)
    y = rng.standard_normal((2, 5, 3)) + 1j * rng.standard_normal((2, 5, 3))
    z, _ = sic.sic_apply(y, order, T, Ct, 16)           # [N][n][J]
    llr = sic.sic_llr(z, nu.T[:, None, :], 16, failed=failed[None, None, :])
    assert llr.shape == (2, 5, 3, 4)
    assert np.all(llr[:, :, 1] == 0.0)
    good = llr[:, :, [0, 2]]
    assert np.all(np.isfinite(good)) and np.all(good != 0.0)
    assert np.all(np.abs(good) > 1e20)                  # delta / 1e-30, not a division by zero
    # without the flag the failed carrier is floored like the others: z = 0 there
    # (the less significant bits: its z is 0, midway between the halves the others tell apart)
    assert np.all(sic.sic_llr(z, nu.T[:, None, :], 16)[:, :, 1][..., [1, 3]] != 0.0)
    # a NaN z gives 0 in the dimension it touches
    out = sic.sic_llr(np.array([np.nan + 0.1j]), 0.5, 16)
    assert np.all(out[0, :2] == 0.0) and np.all(out[0, 2:] != 0.0)


def test_null_handle_and_null_struct_are_argument_errors():
    L = _lib.lib()
    a = _lib.SicSoft(16, 32, 48, 64, 1, 1, 0, _lib.LLR_I8, 1.0)
    assert L.mimo_rx_sic_soft(None, C.byref(a), None) == -1
    assert L.mimo_rx_sic_soft(None, None, None) == -1


def test_sic_soft_struct_layout(tmp_path):
    """The ctypes mirror of mimo_sic_soft matches the C header field for field."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mimo_rx.h"',
             'int main(void) {', 'printf("size %zu\\n", sizeof(mimo_sic_soft));']
    for fname, _ in _lib.SicSoft._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(mimo_sic_soft, %s));' % (fname, fname))
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(_lib.SicSoft)
    assert [f for f, _ in _lib.SicSoft._fields_] == [
        "d_sym", "d_llr", "d_out_sym", "d_out_idx", "n_frames", "max_out_syms", "out_layout",
        "format", "llr_scale"]
    for fname, _ in _lib.SicSoft._fields_:
        assert int(got[fname]) == getattr(_lib.SicSoft, fname).offset, fname
