"""CPU checks of the ordered MMSE-SIC definition (rub_mimo_amd/sic.py, DESIGN.md "SIC
detection"): identities of the tables, the genie and forced-order properties, and the symbol
error counts of the linear and the SIC detector on the oracle's own frames. No GPU calls."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import ref
from rub_mimo_amd import _lib, sic, soft


def rand_G(rng, J, N):
    return rng.standard_normal((J, N, N)) + 1j * rng.standard_normal((J, N, N))


@pytest.mark.parametrize("N", [1, 2, 3, 4, 8])
def test_stage0_is_the_unbiased_linear_mmse_output(N):
    """With lam = s2, T[0] = e_(pi_0) / beta_0: stage 0 only rescales y_(pi_0)."""
    rng = np.random.default_rng(10 + N)
    G = rand_G(rng, 64, N)
    s2 = 0.03
    order, T, Ct, nu = sic.sic_tables(G, s2, s2)
    Q = np.conj(G.transpose(0, 2, 1)) @ G
    E = np.linalg.inv(Q + s2 * np.eye(N))
    d = np.real(np.diagonal(E, axis1=1, axis2=2))
    assert np.array_equal(order[:, 0], np.argmin(d, axis=1))
    for j in range(64):
        p = order[j, 0]
        beta = 1.0 - s2 * d[j, p]
        want = np.zeros(N, np.complex128)
        want[p] = 1.0 / beta
        assert np.abs(T[j, 0] - want).max() <= 1e-12, j
        assert abs(nu[j, p] - (1.0 - beta) / beta) <= 1e-12
        assert sorted(order[j]) == list(range(N))
    assert np.all(Ct[:, np.triu_indices(N)[0], np.triu_indices(N)[1]] == 0)


@pytest.mark.parametrize("N,qam", [(2, 4), (3, 16), (4, 64), (8, 256)])
def test_genie_zero_forcing_recovers_the_transmitted_indices(N, qam):
    """y = (Q + lam I)^-1 G^H G s with lam = 0 and s2 = 0: every stage's z is its own
    constellation point (to rounding), so the indices come back exactly."""
    rng = np.random.default_rng(20 + N)
    J, n = 48, 5
    G = rand_G(rng, J, N)
    tx = rng.integers(0, qam, (N, n, J)).astype(np.uint8)
    s = sic.qam_points(tx, qam)
    Q = np.conj(G.transpose(0, 2, 1)) @ G
    # y[u][n][j] = ((Q)^-1 G^H G s)_u
    y = np.einsum("juv,vnj->unj", np.linalg.inv(Q) @ Q, s)
    order, T, Ct, nu = sic.sic_tables(G, 0.0, 0.0)
    z, idx = sic.sic_apply(y, order, T, Ct, qam)
    assert np.array_equal(idx, tx)
    assert np.abs(z - s).max() <= 1e-6
    assert np.all(nu == 0.0)
    # and with a small s2 in the ordering / nulling (lam still 0): still exact without noise
    order2, T2, C2, nu2 = sic.sic_tables(G, 1e-4, 0.0)
    _, idx2 = sic.sic_apply(y, order2, T2, C2, qam)
    assert np.array_equal(idx2, tx)
    assert np.all(nu2 > 0.0)


def test_diagonal_channel_needs_no_cancellation():
    rng = np.random.default_rng(3)
    J, N = 32, 4
    g = rng.uniform(0.2, 2.0, (J, N)) * np.exp(2j * np.pi * rng.uniform(size=(J, N)))
    G = np.zeros((J, N, N), np.complex128)
    G[:, np.arange(N), np.arange(N)] = g
    for lam in (0.0, 0.01):
        order, T, Ct, nu = sic.sic_tables(G, 0.01, lam)
        assert np.all(Ct == 0.0)
        want = np.argsort(-np.abs(g), axis=1, kind="stable")
        assert np.array_equal(order, want)
        # nu_sic of a lone stream: s2 / |g|^2
        assert np.allclose(nu, 0.01 / np.abs(g) ** 2, rtol=1e-12)


@pytest.mark.parametrize("N", [2, 4, 8])
def test_forced_order_reproduces_the_free_tables(N):
    rng = np.random.default_rng(40 + N)
    G = rand_G(rng, 40, N)
    free = sic.sic_tables(G, 0.02, 0.02)
    forced = sic.sic_tables(G, 0.02, 0.02, order=free[0])
    for a, b in zip(free, forced):
        assert np.array_equal(a, b)
    # another order gives other tables, and a larger MSE at stage 0
    rev = free[0][:, ::-1]
    other = sic.sic_tables(G, 0.02, 0.02, order=rev)
    assert np.array_equal(other[0], rev)
    ar = np.arange(40)
    assert np.all(other[3][ar, rev[:, 0]] >= free[3][ar, free[0][:, 0]])


def test_singular_carrier_gets_zero_tables():
    G = np.zeros((3, 2, 2), np.complex128)
    G[0] = [[1, 0.5], [0.2, 1]]
    G[2] = [[1, 0.1], [0.3, -1]]
    order, T, Ct, nu = sic.sic_tables(G, 0.0, 0.0)      # carrier 1: Q = 0, s2 = 0
    assert np.array_equal(order[1], [0, 1])
    assert np.all(T[1] == 0) and np.all(Ct[1] == 0) and np.all(nu[1] == 0)
    assert np.any(T[0] != 0) and np.any(T[2] != 0)


def test_demap_restatement_matches_the_oracle_slicer():
    rng = np.random.default_rng(5)
    for qam in (4, 16, 64, 256):
        lv = soft.qam_levels(qam)
        z = (rng.uniform(-1.5, 1.5, 2000) + 1j * rng.uniform(-1.5, 1.5, 2000)) * (lv[-1] + 0.2)
        z = z.astype(np.complex64)
        want = np.array([ref.qam_demap(complex(v), qam) for v in z], np.uint8)
        assert np.array_equal(sic.qam_demap_f32(z, qam), want)
        pts = np.array([ref.qam_point(i, qam) for i in range(qam)])
        assert np.array_equal(sic.qam_points(np.arange(qam), qam).astype(np.complex64),
                              pts.astype(np.complex64))
    nan = np.array([np.nan + 0.1j, 0.1 + np.nan * 1j, np.inf - np.inf * 1j])
    got = sic.qam_demap_f32(nan, 16)
    assert got[0] >> 2 == 0 and got[1] & 3 == 0


# M, cp, N, nac, pid, qam, detector, all-carriers allocation, seed (the issue's table)
ORACLE_CASES = {
    "qam64_mmse_4x4": (128, 32, 4, 8, 8, 64, ref.DET_MMSE, False, 77),
    "qam16_zf_allocc": (256, 32, 2, 4, 10, 16, ref.DET_ZF, True, 76),
}


@functools.lru_cache(maxsize=None)
def oracle_counts(name):
    M, cp, N, nac, pid, qam, det, allocc, seed = ORACLE_CASES[name]
    p = np.full(M, 2, np.uint8) if allocc else None
    lin = sicn = total = 0
    for f in range(3):
        rx, tx_idx, _ = ref.synth_frame(M, cp, N, nac, pid, qam, seed=seed, frame=f, offset=-1,
                                        snr_db=30.0, p=p)
        o = ref.FrameSyncRef(M, cp, N, nac, pid_max=pid, detector=det, keep_identity_bias=False,
                             p=p)
        assert o.execute(rx) == ref.STATE_MIMO, (name, f)
        sym = o.symbols()                                  # [n][N][M_occ]
        n = min(len(sym), pid)
        assert n == pid, (name, f, len(sym))
        occ = np.flatnonzero(o.p != 0)
        s2 = o.get_noise_var()
        G = o.get_G()[occ]
        y = sym[:n].transpose(1, 0, 2)                     # [N][n][M_occ]
        order, T, Ct, _ = sic.sic_tables(G, s2, s2 if det == ref.DET_MMSE else 0.0)
        _, idx = sic.sic_apply(y, order, T, Ct, qam)
        lin += int(np.sum(sic.qam_demap_f32(y, qam) != tx_idx[:, :n]))
        sicn += int(np.sum(idx != tx_idx[:, :n]))
        total += idx.size
    return lin, sicn, total


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_sic_makes_fewer_symbol_errors_on_the_oracle_frames(name):
    """Three synthetic frames at 30 dB through the CPU oracle (G, noise variance, equalised
    symbols), then the definition: 3825 < 4378 of 12288 (4x4 MMSE 64-QAM) and 6 < 115 of 15360
    (2x2 ZF 16-QAM) when this was written."""
    lin, sicn, total = oracle_counts(name)
    print("%s: linear %d, SIC %d symbol errors of %d" % (name, lin, sicn, total))
    assert sicn < lin


def test_null_handles_are_argument_errors():
    L = _lib.lib()
    a = _lib.SicDetect(16, 32, 48, 1, 1, 0)
    assert L.mimo_rx_sic_detect(None, C.byref(a), None) == -1
    buf = (C.c_float * 4)()
    assert L.mimo_rx_sic_mse(None, C.cast(buf, C.c_void_p), 1) == -1
    assert L.mimo_rx_sic_order(None, C.cast(buf, C.c_void_p), 1) == -1


def test_sic_detect_struct_layout(tmp_path):
    """The ctypes mirror of mimo_sic_detect matches the C header field for field."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mimo_rx.h"',
             'int main(void) {', 'printf("size %zu\\n", sizeof(mimo_sic_detect));']
    for fname, _ in _lib.SicDetect._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(mimo_sic_detect, %s));' % (fname, fname))
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(_lib.SicDetect)
    for fname, _ in _lib.SicDetect._fields_:
        assert int(got[fname]) == getattr(_lib.SicDetect, fname).offset, fname
