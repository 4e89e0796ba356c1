"""CPU checks of the layered tree-search definition (rub_mimo_amd/lord.py, DESIGN.md "Layered
tree search"): exactness against an exhaustive max-log ML search at N = 2, the ML lower bound at
N = 4, the N = 1 closed form, the order rule, the regularised factor and the erasures, the
information of its LLRs against the linear detector's, a float32 restatement of the kernel's
arithmetic (lord_kernels.hip) against the float64 model, which sets the tolerance ratio the GPU
tests use, the `ambiguous` mask, and the share of ambiguous entries on the oracle's frames of
every GPU test case. No GPU calls."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from oracle import ref
from rub_mimo_amd import _lib, fec, lord, pic, sic, soft

U = 2.0 ** -24


def _rayleigh(rng, N, J, n, order, snr_db, lam_is_s2=True):
    """i.i.d. Rayleigh G [J][N][N] known exactly, unit-energy symbols, noise CN(0, s2),
    s2 = 10^(-snr_db / 10), and the linear decode's output y = (Q + lam I)^-1 G^H X by stream
    [N][n][J] (the geometry of test_pic_model.py)."""
    s2 = 10.0 ** (-snr_db / 10.0)
    G = (rng.standard_normal((J, N, N)) + 1j * rng.standard_normal((J, N, N))) / np.sqrt(2.0)
    sent = rng.integers(0, order, (N, n, J)).astype(np.uint8)
    s = sic.qam_points(sent, order)
    w = (rng.standard_normal((N, n, J)) + 1j * rng.standard_normal((N, n, J))) * np.sqrt(s2 / 2.0)
    X = np.einsum("jru,unj->rnj", G, s) + w
    return (G, s2, sent, s, X) + (_decode(G, X, s2 if lam_is_s2 else 0.0),)


def _decode(G, X, lam):
    N = G.shape[-1]
    Gh = np.conj(G.transpose(0, 2, 1))
    return np.einsum("jur,rnj->unj", np.linalg.inv(Gh @ G + lam * np.eye(N)) @ Gh, X)


def _bit_table(order):
    nb = 2 * soft.qam_bits(order)
    return (np.arange(order)[:, None] >> (nb - 1 - np.arange(nb))) & 1          # [C][2b]


def _exhaustive(Q, m, order):
    """D(s) = s^H Q s - 2 Re(s^H m) over all order^N vectors: the per-target, per-bit minima
    [N][n][J][2b][2] and the ML vector's indices [N][n][J]. Q [J][N][N], m [n][J][N]."""
    N = Q.shape[-1]
    pts = sic.qam_points(np.arange(order), order)
    vec = np.array(list(itertools.product(range(order), repeat=N)))             # [V][N]
    S = pts[vec]                                                                # [V][N]
    quad = np.real(np.einsum("vt,jtu,vu->jv", np.conj(S), Q, S))                # [J][V]
    lin = np.real(np.einsum("vt,njt->njv", np.conj(S), m))
    D = quad[None] - 2.0 * lin                                                  # [n][J][V]
    bits = _bit_table(order)
    nb = bits.shape[1]
    mins = np.zeros((N,) + D.shape[:2] + (nb, 2))
    for t in range(N):
        for i in range(nb):
            for v in (0, 1):
                mins[t, :, :, i, v] = D[:, :, bits[vec[:, t], i] == v].min(-1)
    best = vec[np.argmin(D, axis=-1)]                                           # [n][J][N]
    return mins, best.transpose(2, 0, 1), D.min(-1)


def _model_mins(D, order):
    bits = _bit_table(order)
    nb = bits.shape[1]
    out = np.zeros(D.shape[:-1] + (nb, 2))
    for i in range(nb):
        for v in (0, 1):
            out[..., i, v] = D[..., bits[:, i] == v].min(-1)
    return out


@pytest.mark.parametrize("order,mmse", [(4, False), (16, True), (16, False)])
def test_two_streams_are_exactly_max_log_ml(order, mmse):
    """2x2 QPSK and 16-QAM on random G against the exhaustive search over all L^4 vectors: LLRs
    equal to 1e-9 relative (of the larger of the LLR and one unit of s^H Q s / s2) and idx equal.
    No exclusions: the one sliced stream is the exact minimiser, so the result is continuous in
    its inputs. That needs the factor without regularisation at N = 2 (lord.lord_reg): with
    s2 in it the chain slices the biased estimate, which is the minimiser of D(s) + s2 |s|^2 and
    not of D(s), and some 16-QAM LLRs at 14 dB are then off by 1 % (QPSK, of constant modulus,
    is exact either way). The tables are kept in float64 here (fp32_tables=False): the stored
    fp32 factor moves the metric by 1e-7 relative."""
    rng = np.random.default_rng(800 + order)
    N, J, n = 2, 96, 6
    G, s2, _, _, _, y = _rayleigh(rng, N, J, n, order, 14.0, mmse)
    lam = s2 if mmse else 0.0
    out = lord.lord_frame(y, G, s2, lam, order, llr_scale=0.7, fp32_tables=False)
    Q = out["Q"]
    m = np.einsum("jtu,unj->njt", Q, y) + lam * y.transpose(1, 2, 0)
    mins, best, _ = _exhaustive(Q, m, order)
    want = 0.7 * (mins[..., 1] - mins[..., 0]) / s2
    unit = 0.7 * np.abs(Q).max() / s2
    assert np.all(np.abs(out["llr"] - want) <= 1e-9 * np.maximum(np.abs(want), unit))
    assert np.array_equal(out["idx"], best)
    assert not out["erased"].any()


def test_four_streams_never_beat_the_exhaustive_search():
    """4x4 QPSK (256 vectors): every per-bit minimum of the model, less |yt|^2 = m^H (Q + s2 I)^-1
    m, is >= the exhaustive one, and equal to it wherever the chain found the ML vector, which it
    does on most entries at 10 dB."""
    rng = np.random.default_rng(811)
    N, J, n, order = 4, 64, 6, 4
    G, s2, _, _, _, y = _rayleigh(rng, N, J, n, order, 10.0)
    out = lord.lord_frame(y, G, s2, s2, order, fp32_tables=False)
    Q = out["Q"]
    m = np.einsum("jtu,unj->njt", Q, y) + s2 * y.transpose(1, 2, 0)
    const = np.real(np.einsum("njt,jtu,nju->nj", np.conj(m), np.linalg.inv(Q + s2 * np.eye(N)), m))
    mins, best, dmin = _exhaustive(Q, m, order)
    got = _model_mins(out["D"], order) - const[None, :, :, None, None]
    tol = 1e-9 * (1.0 + np.abs(mins))
    assert np.all(got >= mins - tol)
    found = np.abs(got.min(axis=(-1, -2)) - dmin[None]) <= 1e-9 * (1.0 + np.abs(dmin[None]))
    assert np.all(out["idx"][found] == best[found])
    eq = np.abs(got - mins) <= tol
    print("4x4 QPSK: the chain found the ML vector on %.3f of the entries, %.3f of the per-bit "
          "minima are the exhaustive ones" % (found.mean(), eq.mean()))
    assert found.mean() > 0.5 and eq.mean() > 0.5 and not eq.all()


@pytest.mark.parametrize("order,mmse", [(4, False), (16, True), (64, False), (256, True)])
def test_one_stream_is_the_scalar_demapper(order, mmse):
    """N = 1: the max-log LLRs of z = m / Q with error power s2 / Q, and idx its slicer."""
    rng = np.random.default_rng(820 + order)
    J, n = 64, 6
    G, s2, _, _, _, y = _rayleigh(rng, 1, J, n, order, 12.0, mmse)
    lam = s2 if mmse else 0.0
    out = lord.lord_frame(y, G, s2, lam, order, llr_scale=2.0, fp32_tables=False)
    q = out["Q"][:, 0, 0].real
    z = (q + lam)[None, None, :] * y / q[None, None, :]
    want = soft.llr_reference(z, (s2 / q)[None, None, :], order, llr_scale=2.0)
    assert np.all(np.abs(out["llr"] - want) <= 1e-9 * np.maximum(np.abs(want), 1.0))
    assert np.array_equal(out["idx"], sic.qam_demap_f32(z, order))


def test_order_factor_and_erasures():
    """The others by decreasing stored Q[u][u], ties to the lower index, the target last;
    U^H U = P (Q + s2 I) P^T (N = 4) with a real positive diagonal, regularised whatever lam is; a
    carrier whose Q holds an inf and a frame with noise_var <= 0 or NaN are erased."""
    rng = np.random.default_rng(830)
    N, J = 4, 8
    G = (rng.standard_normal((J, N, N)) + 1j * rng.standard_normal((J, N, N))) / np.sqrt(2.0)
    G[0] = np.diag([1.0, 3.0, 2.0, 4.0])         # column energies 1, 9, 4, 16
    G[1] = np.diag([2.0, 1.0, 2.0, 2.0])         # ties
    s2 = 0.05
    Q, perm, Uf, erased = lord.lord_tables(G, s2)
    assert not erased.any()
    assert perm[0].tolist() == [[2, 1, 3, 0], [0, 2, 3, 1], [0, 1, 3, 2], [0, 2, 1, 3]]
    assert perm[1].tolist() == [[1, 3, 2, 0], [3, 2, 0, 1], [1, 3, 0, 2], [1, 2, 0, 3]]
    for j in range(J):
        qd = Q[j].diagonal().real
        for t in range(N):
            p = perm[j, t]
            assert p[-1] == t and sorted(p.tolist()) == list(range(N))
            det = p[:-1][::-1]                   # detection order o_0, o_1, ...
            assert np.all(np.diff(qd[det]) <= 0)
            Ut = Uf[j, t]
            assert np.all(np.tril(Ut, -1) == 0) and np.all(Ut.diagonal().real > 0)
            assert np.all(Ut.diagonal().imag == 0)
            A = (Q[j] + s2 * np.eye(N))[np.ix_(p, p)]
            assert np.abs(np.conj(Ut.T) @ Ut - A).max() <= 4e-7 * np.abs(A).max()
    # N = 2: no regularisation (lord.lord_reg)
    Q2, perm2, U2, _ = lord.lord_tables(G[:, :2, :2], s2)
    for j in range(J):
        for t in range(2):
            assert perm2[j, t].tolist() == [1 - t, t]
            A = Q2[j][np.ix_(perm2[j, t], perm2[j, t])]
            assert np.abs(np.conj(U2[j, t].T) @ U2[j, t] - A).max() <= 4e-7 * np.abs(A).max()
    # erasures
    y = rng.standard_normal((N, 3, J)) + 1j * rng.standard_normal((N, 3, J))
    Gi = G.copy()
    Gi[3, 1, 2] = np.inf
    out = lord.lord_frame(y, Gi, s2, 0.0, 16, with_bound=True)
    assert out["erased"].tolist() == [j == 3 for j in range(J)]
    assert np.all(out["llr"][:, :, 3] == 0) and np.all(out["idx"][:, :, 3] == 0)
    assert np.any(out["llr"][:, :, 2] != 0) and not out["ambiguous"][:, :, 3].any()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        out = lord.lord_frame(y, G, bad, 0.0, 16)
        assert out["erased"].all() and np.all(out["llr"] == 0) and np.all(out["idx"] == 0)


def test_int8_is_the_quantised_float_output():
    rng = np.random.default_rng(840)
    G, s2, _, _, _, y = _rayleigh(rng, 2, 32, 4, 16, 12.0)
    out = lord.lord_frame(y, G, s2, s2, 16, llr_scale=3.0)
    q = lord.lord_llr_i8(out["llr"])
    assert q.dtype == np.int8 and np.array_equal(q, soft.quantise_i8(out["llr"]))
    assert np.any(np.abs(q) == 127) and np.any(np.abs(q) < 127) and not np.any(q == -128)


# SNRs (10 log10(1 / s2), unit-variance channel entries) that put the unbiased linear MMSE
# detector of 4x4 64-QAM near 0.6 and 0.75 bit of GMI per bit
GMI_SNRS = (12.0, 16.0)


@pytest.mark.parametrize("snr", GMI_SNRS)
def test_lord_carries_more_information_than_the_linear_detector(snr):
    """4x4 64-QAM on perfectly known i.i.d. Rayleigh channels, 256 carriers x 12 symbols,
    default_rng(1): GMI per bit of the LORD LLRs strictly above the unbiased linear MMSE
    detector's (pic.pic_frame with no priors).
    Measured (linear, LORD): 0.596, 0.614 at 12 dB; 0.753, 0.827 at 16 dB."""
    N, order, J, n = 4, 64, 256, 12
    G, s2, sent, _, _, y = _rayleigh(np.random.default_rng(1), N, J, n, order, snr)
    lin = sic.llr_gmi(pic.pic_frame(y, G, s2, s2, None, 1.0, order)["llr"], sent, order)
    got = sic.llr_gmi(lord.lord_frame(y, G, s2, s2, order)["llr"], sent, order)
    print("4x4 64-QAM %.0f dB: GMI per bit linear MMSE %.3f, LORD %.3f" % (snr, lin, got))
    assert got > lin


# ---- the kernel's arithmetic restated in float32 -------------------------------------------
def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64)
            + np.asarray(c, np.float64)).astype(np.float32)


def _mac(acc, a, b):
    """sic_mac: acc += a b as two fused multiply-adds per component, a's real part first."""
    ar, ai = a
    xr = _fma(ai, -b[1], _fma(ar, b[0], acc[0]))
    xi = _fma(ai, b[0], _fma(ar, b[1], acc[1]))
    return xr, xi


def _slice_f32(er, ei, order):
    """sic_slice: the levels of both dimensions and the point (2 m - (L - 1)) scale, float32."""
    f = np.float32
    b = soft.qam_bits(order)
    L = 1 << b
    inv = sic.qam_inv_scale(order)
    scale = f(1.0 / np.sqrt(2.0 * (L * L - 1.0) / 3.0))

    def level(v):
        t = (v * inv + f(L)) * f(0.5)
        return np.clip(np.where(np.isnan(t), f(0.0), np.floor(t)), 0, L - 1).astype(np.int64)

    mi, mq = level(er), level(ei)
    return mi, mq, (2 * mi - (L - 1)).astype(f) * scale, (2 * mq - (L - 1)).astype(f) * scale


def lord_f32(y, Q, perm, Uf, s2, lam, order):
    """lord_pass_kernel in float32 numpy, operation for operation (the fused multiply-adds
    through float64 products), on the model's tables (stored fp32 values; the reciprocal
    diagonal is rounded from the float64 reciprocal). y [N][n][J] complex64. Returns (D
    [N][n][J][C] float64 by candidate index, code [N][n][J][C] int64, the sliced levels of the
    chain packed 8 bits per position and dimension)."""
    f = np.float32
    N, n, J = y.shape
    b = soft.qam_bits(order)
    L = 1 << b
    scale = f(1.0 / np.sqrt(2.0 * (L * L - 1.0) / 3.0))
    s2, lam = f(s2), f(lam)
    yr, yi = y.real.astype(f), y.imag.astype(f)
    Qr, Qi = Q.real.astype(f), Q.imag.astype(f)
    shape = (n, J)
    bc = lambda a: np.broadcast_to(a[None, :], shape)
    m = []
    for u in range(N):
        acc = (lam * yr[u], lam * yi[u])
        for v in range(N):
            acc = _mac(acc, (bc(Qr[:, u, v]), bc(Qi[:, u, v])), (yr[v], yi[v]))
        m.append(acc)
    D = np.zeros((N, n, J, L * L))
    code = np.zeros((N, n, J, L * L), np.int64)
    gdec = lambda g: g ^ (g >> 1) ^ (g >> 2) ^ (g >> 3)
    for t in range(N):
        ud = [bc(Uf[:, t, k, k].real.astype(f)) for k in range(N)]
        ur = [bc((1.0 / Uf[:, t, k, k].real).astype(f)) for k in range(N)]
        uo = {(k, i): (bc(Uf[:, t, k, i].real.astype(f)), bc(Uf[:, t, k, i].imag.astype(f)))
              for k in range(N) for i in range(k + 1, N)}
        if N > 1:
            yt = []
            for k in range(N):
                pk = bc(perm[:, t, k])
                acc = (np.choose(pk, [mm[0] for mm in m]), np.choose(pk, [mm[1] for mm in m]))
                for i in range(k):
                    acc = _mac(acc, (-uo[i, k][0], uo[i, k][1]), yt[i])
                yt.append((acc[0] * ur[k], acc[1] * ur[k]))
        else:
            yt = [m[0]]
        for gI in range(L):
            cr = f(2 * gdec(gI) - (L - 1)) * scale
            cr2 = cr * cr
            if N > 1:
                base = [(_fma(-cr, uo[k, N - 1][0], yt[k][0]), _fma(-cr, uo[k, N - 1][1], yt[k][1]))
                        for k in range(N - 1)]
                base.append((_fma(-cr, ud[N - 1], yt[N - 1][0]), yt[N - 1][1]))
            else:
                base = [(cr * yt[0][0], None)]
            for gQ in range(L):
                ci = f(2 * gdec(gQ) - (L - 1)) * scale
                en = _fma(ci, ci, cr2)
                cd = np.zeros(shape, np.int64)
                if N == 1:
                    dot = _fma(ci, yt[0][1], base[0][0])
                    Dc = _fma(bc(Qr[:, 0, 0]), en, f(-2.0) * dot)
                else:
                    sv = [None] * N
                    ry = _fma(-ci, ud[N - 1], base[N - 1][1])
                    acc = _fma(ry, ry, base[N - 1][0] * base[N - 1][0])
                    for k in range(N - 2, -1, -1):
                        u = uo[k, N - 1]
                        av = (_fma(ci, u[1], base[k][0]), _fma(-ci, u[0], base[k][1]))
                        for i in range(N - 2, k, -1):
                            av = _mac(av, (-uo[k, i][0], -uo[k, i][1]), sv[i])
                        mi, mq, px, py = _slice_f32(av[0] * ur[k], av[1] * ur[k], order)
                        cd = cd | (mi << (16 * k)) | (mq << (16 * k + 8))
                        sv[k] = (px, py)
                        rx, rz = _fma(-ud[k], px, av[0]), _fma(-ud[k], py, av[1])
                        acc = _fma(rz, rz, _fma(rx, rx, acc))
                        en = _fma(py, py, _fma(px, px, en))
                    Dc = _fma(-s2, en, acc) if N > 2 else acc
                assert Dc.dtype == f
                c = (gI << b) | gQ
                D[t, :, :, c] = Dc
                code[t, :, :, c] = cd
    return D, code


# the GPU cases' geometries (tests/test_gpu_lord.py): N, QAM order, MMSE
RESTATED = [(2, 4, False), (2, 16, False), (4, 64, True), (4, 256, True), (1, 16, False)]


@pytest.mark.parametrize("N,order,mmse", RESTATED)
def test_float32_restatement_of_the_kernels_arithmetic(N, order, mmse):
    """The kernel's per-symbol arithmetic in float32 against the float64 model on the same
    complex64 G, 30 dB i.i.d. Rayleigh (512 carriers x 4 symbols). With u = 2^-24, kappa the
    2-norm condition number of Q + s2 I and mag the magnitude sum of lord.lord_detect, on every
    entry whose candidates all slice as the model's do it measures the worst
      |dD32 - dD64| / (u kappa mag),
    dD the difference of the two minima behind an LLR, and asserts it below lord.D_RATIO_F32,
    the recorded figure the GPU bound is 8x of. Every entry on which an LLR or the hard decision
    is off by more than the GPU tolerance must carry the model's `ambiguous` flag, and at N <= 2
    the mask is empty.
    Measured worst ratios: 0.79 (2x2 QPSK), 0.68 (2x2 16-QAM), 0.046 (4x4 64-QAM), 0.044 (4x4
    256-QAM; kappa is pessimistic for the chains), 1.44 (1x1 16-QAM); entries with a different
    slicing, all of which the mask covers: 0, 0, 2, 5, 0; entries off by more than the bound
    outside the mask: none. On these draws, whose kappa reaches the thousands, the mask holds
    0 / 0 / 0.071 / 0.215 / 0 of the entries: the cap of 2 % is a property of the GPU cases'
    channels (the last test below), not of every channel."""
    rng = np.random.default_rng(860 + N + order)
    J, n = 512, 4
    G, s2, _, _, X, _ = _rayleigh(rng, N, J, n, order, 30.0, mmse)
    G = G.astype(np.complex64)
    s2 = float(np.float32(s2))
    lam = s2 if mmse else 0.0
    y = _decode(G.astype(np.complex128), X, lam).astype(np.complex64)
    ref_ = lord.lord_frame(y, G, s2, lam, order, with_bound=True)
    D32, code32 = lord_f32(y, ref_["Q"], ref_["perm"], ref_["U"], s2, lam, order)
    d32 = lord.delta_of(D32, order)
    same = np.all(code32 == ref_["code"], axis=-1)                               # [N][n][J]
    unit = U * ref_["cond"][None, None, :] * ref_["mag"]
    err = np.abs(d32 - ref_["delta"]).max(-1)
    ratio = float((err / unit)[same].max())
    amb = ref_["ambiguous"]
    off = (err > ref_["tol"]) | ((np.argmin(D32, -1) != ref_["idx"]) & (ref_["gap"] > ref_["tol"]))
    print("N %d %d-QAM: worst dD ratio %.3f, ambiguous %.4f, different slicings %d, entries off "
          "by more than the bound %d" % (N, order, ratio, amb.mean(), int((~same).sum()),
                                         int(off.sum())))
    assert ratio <= lord.D_RATIO_F32
    assert not np.any(off & ~amb)
    if N <= 2:
        assert not amb.any()


# ---- the share of ambiguous entries on the oracle's frames of the GPU test cases ------------
# M, cp, N, nac, pid, qam, detector, sctype, synthesiser seed: tests/test_gpu_lord.py's table
GPU_CASES = {
    "qpsk_zf2": (64, 16, 2, 4, 10, 4, ref.DET_ZF2, None, 79),
    "qam16_zf_allocc": (256, 32, 2, 4, 10, 16, ref.DET_ZF, "all", 76),
    "qam64_mmse_4x4": (128, 32, 4, 8, 8, 64, ref.DET_MMSE, None, 84),
    "qpsk_zf_guard_2blocks": (64, 16, 2, 4, 34, 4, ref.DET_ZF, "liquid", 79),
    "qam16_zf_1x1": (64, 16, 1, 4, 10, 16, ref.DET_ZF, None, 79),
    "qam256_mmse_4x4": (64, 16, 4, 2, 8, 256, ref.DET_MMSE, None, 84),
}


def oracle_frames(M, cp, N, nac, pid, qam, det, sct, seed, snr_db=30.0, frames=(0, 2),
                  threshold=0.95, bias=True):
    """The oracle's synthesiser and framesync on the frames the GPU tests keep (frame 1 is
    replaced by noise there): per frame (y [N][n][M_occ], G_occ, s2, lam, tx_idx)."""
    p = {"all": np.full(M, 2, np.uint8), "liquid": ref.liquid_sctype(M), None: None}[sct]
    out = []
    for f in frames:
        rx, tx_idx, _ = ref.synth_frame(M, cp, N, nac, pid, qam, seed=seed, frame=f, offset=-1,
                                        snr_db=snr_db, p=p)
        o = ref.FrameSyncRef(M, cp, N, nac, pid_max=pid, detector=det,
                             keep_identity_bias=bias, p=p, threshold=threshold)
        assert o.execute(rx) == ref.STATE_MIMO, f
        sym = o.symbols()                                  # [n][N][M_occ]
        occ = np.flatnonzero(o.p != 0)
        s2 = float(np.float32(o.get_noise_var()))
        out.append((sym.transpose(1, 0, 2), o.get_G()[occ], s2,
                    s2 if det == ref.DET_MMSE else 0.0, tx_idx))
    return out


@pytest.mark.parametrize("name", list(GPU_CASES))
def test_ambiguous_share_of_the_gpu_cases_on_the_oracle_frames(name):
    """The mask is a cap, not a tolerance: at most 2 % of the written entries of every GPU test
    case may be ambiguous. Evaluated here on the oracle's frames of each case, with no GPU; a
    case over the cap gets another seed, the cap stays.
    Measured shares: 0 at N <= 2; 4x4 64-QAM 0.0042 and 4x4 256-QAM 0.0143 with seed 84 (two
    channels of kappa 16 to 19). With test_gpu_pic.py's seeds 77 and 79 the shares are 0.031 and
    0.514 (kappa up to 153 and 844), and of seeds 70..99 no other keeps the 256-QAM case under
    the cap."""
    M, cp, N, nac, pid, qam, det, sct, seed = GPU_CASES[name]
    amb = tot = 0
    for y, G, s2, lam, _ in oracle_frames(*GPU_CASES[name]):
        out = lord.lord_frame(y, G, s2, lam, qam, with_bound=True)
        amb += int(out["ambiguous"].sum())
        tot += out["ambiguous"].size
    print("%s: ambiguous %d of %d entries (%.4f)" % (name, amb, tot, amb / tot))
    assert tot > 0 and amb <= 0.02 * tot
    if N <= 2:
        assert amb == 0


# ---- the end-to-end case of tests/test_gpu_lord.py, chosen here ------------------------------
LOOP = dict(M=256, cp=32, N=4, nac=16, pid=12, qam=64, snr=20.0, seed=75)


@functools.lru_cache(maxsize=None)
def loop_counts():
    """Info-bit errors of the two float64 model chains (LORD, and pic_frame with no priors)
    through fec.decode_siso on the oracle's frames 0 and 2 of the end-to-end case: rate 1/2, one
    codeword per (stream, symbol) row through the code's linearity, int8 LLRs at scale 4."""
    c = LOOP
    nb = 2 * soft.qam_bits(c["qam"])
    errs = np.zeros(2, np.int64)
    fr = oracle_frames(c["M"], c["cp"], c["N"], c["nac"], c["pid"], c["qam"], ref.DET_MMSE, None,
                       c["seed"], snr_db=c["snr"], threshold=0.85, bias=False)
    for f, (y, G, s2, lam, sent) in zip((0, 2), fr):
        y = y[:, :c["pid"]]
        N, n, J = y.shape
        rows = sent.reshape(N * n, J)
        n_c = J * nb
        _, n_info, _ = fec.geometry(fec.R12, n_c)
        info = np.random.default_rng(11 + f).integers(0, 2, (N * n, n_info)).astype(np.uint8)
        cw = fec.encode(fec.R12, n_c, info)
        x = ((rows.astype(np.int64)[..., None] >> (nb - 1 - np.arange(nb))) & 1).reshape(N * n, n_c)
        flip = (x.astype(np.uint8) ^ cw) == 1
        for i, llr in enumerate((lord.lord_frame(y, G, s2, lam, c["qam"], llr_scale=4.0)["llr"],
                                 pic.pic_frame(y, G, s2, lam, None, 4.0, c["qam"],
                                               llr_scale=4.0)["llr"])):
            q = soft.quantise_i8(llr).reshape(N * n, n_c)
            _, _, il, _ = fec.decode_siso(fec.R12, n_c, np.where(flip, -q, q).astype(np.int8),
                                          mode=fec.SISO_EXT)
            errs[i] += int(np.sum((il[:, :n_info] < 0) != info))
    return errs.tolist()


def test_lord_decodes_with_no_more_errors_than_the_linear_detector_on_the_oracle_frames():
    """The end-to-end case of the GPU test (4x4 64-QAM, 20 dB, seed 75, threshold 0.85) on the
    CPU first: LORD's int8 LLRs through the soft-output decoder leave no more info-bit errors
    than the NULL-prior PIC pass's. Measured: LORD 18, linear 5058."""
    e_lord, e_lin = loop_counts()
    print("info-bit errors after one decoder pass: LORD %d, linear MMSE %d" % (e_lord, e_lin))
    assert e_lord <= e_lin and e_lin > 0


def test_null_handle_and_null_struct_are_argument_errors():
    L = _lib.lib()
    a = _lib.LordSoft(16, 32, 48, 1, 1, 0, _lib.LLR_I8, 1.0)
    assert L.mimo_rx_lord_soft(None, C.byref(a), None) == -1
    assert L.mimo_rx_lord_soft(None, None, None) == -1


def test_lord_soft_struct_layout(tmp_path):
    """The ctypes mirror of mimo_lord_soft matches the C header field for field."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mimo_rx.h"',
             'int main(void) {', 'printf("size %zu\\n", sizeof(mimo_lord_soft));']
    for fname, _ in _lib.LordSoft._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(mimo_lord_soft, %s));' % (fname, fname))
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(_lib.LordSoft)
    for fname, _ in _lib.LordSoft._fields_:
        assert int(got[fname]) == getattr(_lib.LordSoft, fname).offset, fname
