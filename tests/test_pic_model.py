"""CPU checks of the soft-input MMSE-PIC definition (rub_mimo_amd/pic.py, DESIGN.md "Soft-input
MMSE-PIC"): the factorised prior moments against the softmax over the levels, pic_detect against
the receive-domain textbook filter, the zero-prior, certain-prior and N = 1 limits, the detector's
information against the quality of its priors, the loop through the soft-output decoder, and a
float32 restatement of the kernel's arithmetic (pic_kernels.hip) against the float64 model, which
sets the tolerance ratios the GPU tests use. No GPU calls."""
import ctypes as C

import numpy as np
import pytest

from rub_mimo_amd import _lib, fec, pic, sic, soft

ORDERS = [4, 16, 64, 256]
U = 2.0 ** -24


def _rayleigh(rng, N, J, n, order, snr_db, lam_is_s2=True):
    """i.i.d. Rayleigh G [J][N][N] known exactly, unit-energy symbols, noise CN(0, s2), and the
    linear decode's output y = (Q + lam I)^-1 G^H X by stream [N][n][J] (the geometry of
    test_sic_softfb_model.py)."""
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


def _bits_of(idx, order):
    nb = 2 * soft.qam_bits(order)
    return (np.asarray(idx).astype(np.int64)[..., None] >> (nb - 1 - np.arange(nb))) & 1


def _genie(sent, order):
    return np.where(_bits_of(sent, order) == 1, -127, 127).astype(np.int8)


def _gaussian_priors(rng, sent, order, sigma, prior_scale):
    """Consistent Gaussian a-priori LLRs of standard deviation sigma (mean +-sigma^2 / 2 by the
    transmitted bit), as int8 at prior_scale."""
    bits = _bits_of(sent, order)
    lam = (1 - 2 * bits) * sigma * sigma / 2.0 + sigma * rng.standard_normal(bits.shape)
    return np.clip(np.rint(lam * prior_scale), -127, 127).astype(np.int8)


@pytest.mark.parametrize("order", ORDERS)
def test_nested_moments_are_the_softmax_over_the_levels(order):
    """b = 1..4, every int8 value including -128, |lam| up to 64 (prior_scale 2) and beyond:
    within 1e-12 of the softmax on the factorised form's own levels, the exact products
    (2 m - (L - 1)) scale, and within 5e-7 of it on qam_point's levels, which are those products
    rounded to fp32 (2^-24 relative on levels whose squares reach 2.6)."""
    rng = np.random.default_rng(700 + order)
    nb = 2 * soft.qam_bits(order)
    p = rng.integers(-128, 128, (4096, nb)).astype(np.int8)
    p[:8] = rng.choice(np.array([-128, -127, 0, 1, 127], np.int8), (8, nb))
    p[8] = 0
    L = 1 << soft.qam_bits(order)
    exact = (2.0 * np.arange(L) - (L - 1)) * float(np.float32(1.0 / np.sqrt(2.0 * (L * L - 1.0) / 3.0)))
    assert np.abs(exact - soft.qam_levels(order)).max() <= 1e-7
    for ps in (2.0, 4.0, 0.5, 64.0):
        sn, vn = pic.prior_moments_nested(p, ps, order)
        sb, v = pic.prior_moments(p, ps, order, levels=exact)
        assert np.abs(sb - sn).max() <= 1e-12 and np.abs(v - vn).max() <= 1e-12, ps
        sb, v = pic.prior_moments(p, ps, order)
        assert np.abs(sb - sn).max() <= 5e-7 and np.abs(v - vn).max() <= 5e-7, ps
    sb, v = pic.prior_moments(p[8], 1.0, order)
    assert abs(sb) <= 1e-15 and abs(v - 1.0) <= 1e-6      # uniform: the constellation's energy
    with pytest.raises(TypeError):
        pic.prior_moments(p.astype(np.int16), 1.0, order)


@pytest.mark.parametrize("N,order,mmse", [(2, 4, False), (2, 16, True), (4, 64, True),
                                          (4, 256, False)])
def test_detect_is_the_receive_domain_filter(N, order, mmse):
    """z^ and nu against w_t = C_t^-1 g_t, C_t = G diag(v, v_t := 1) G^H + s2 I, unbiased, from G
    and X directly; 1e-9 relative."""
    rng = np.random.default_rng(710 + N + order)
    J, n = 24, 6
    G, s2, sent, _, X, y = _rayleigh(rng, N, J, n, order, 15.0, mmse)
    prior = rng.integers(-128, 128, (N, n, J, 2 * soft.qam_bits(order))).astype(np.int8)
    sbar, v = pic.prior_moments(prior, 8.0, order)
    z, nu, mu = pic.pic_detect(y, G, s2, s2 if mmse else 0.0, sbar, v)
    for j in range(J):
        for k in range(n):
            for t in range(N):
                vt = v[:, k, j].copy()
                vt[t] = 1.0
                Ct = (G[j] * vt) @ np.conj(G[j].T) + s2 * np.eye(N)
                sb = sbar[:, k, j].copy()
                sb[t] = 0.0
                w = np.linalg.solve(Ct, G[j][:, t])
                g = np.real(np.vdot(w, G[j][:, t]))
                zt = np.vdot(w, X[:, k, j] - G[j] @ sb) / g
                assert abs(z[t, k, j] - zt) <= 1e-9 * abs(zt)
                assert abs(nu[t, k, j] - (1.0 / g - 1.0)) <= 1e-9 * (1.0 / g - 1.0)
    assert np.all(mu > 0) and np.all(nu > 0)


@pytest.mark.parametrize("N,order", [(2, 16), (4, 64)])
def test_zero_priors_give_the_unbiased_linear_mmse(N, order):
    """sbar = 0 exactly; v is the energy of qam_point's fp32 levels, 1 to within 2e-7, so z^ and
    nu are the linear detector's to 1e-6 and not to rounding."""
    rng = np.random.default_rng(720 + N)
    J, n = 48, 8
    G, s2, _, _, _, y = _rayleigh(rng, N, J, n, order, 14.0)
    out = pic.pic_frame(y, G, s2, s2, None, 1.0, order)
    Q = np.conj(G.transpose(0, 2, 1)) @ G
    E = np.linalg.inv(Q + s2 * np.eye(N))
    beta = 1.0 - s2 * np.real(np.diagonal(E, axis1=1, axis2=2)).T              # [N][J]
    assert np.abs(out["z"] - y / beta[:, None, :]).max() <= 1e-6
    nu_lin = ((1.0 - beta) / beta)[:, None, :]
    assert np.abs(out["nu"] / nu_lin - 1.0).max() <= 1e-6
    assert np.all(out["sbar"] == 0) and np.abs(out["v"] - 1.0).max() <= 1e-6
    # stream pi_0: the SIC tables' stage-0 row and nu_sic
    order_, T, _, nu_sic = sic.sic_tables(G, s2, s2)
    ar = np.arange(J)
    pi0 = order_[:, 0].astype(np.int64)
    z0 = np.einsum("ju,unj->nj", T[:, 0, :], y)
    assert np.abs(out["z"][pi0, :, ar].T - z0).max() <= 1e-6
    assert np.abs(out["nu"][pi0, 0, ar] / nu_sic[ar, pi0] - 1.0).max() <= 1e-6


@pytest.mark.parametrize("N,order", [(2, 4), (4, 64), (4, 256)])
def test_certain_priors_reach_the_matched_filter_bound(N, order):
    rng = np.random.default_rng(730 + N + order)
    J, n = 32, 6
    G, s2, sent, s, _, y = _rayleigh(rng, N, J, n, order, 12.0)
    out = pic.pic_frame(y, G, s2, s2, _genie(sent, order), 1.0, order)
    Qtt = np.real(np.einsum("jrt,jrt->tj", np.conj(G), G))
    assert np.abs(out["nu"] / (s2 / Qtt)[:, None, :] - 1.0).max() <= 1e-6
    assert np.abs(out["sbar"] - s).max() <= 1e-12 and out["v"].max() <= 1e-12


@pytest.mark.parametrize("order", ORDERS)
def test_one_stream_does_not_depend_on_the_priors(order):
    rng = np.random.default_rng(740 + order)
    J, n = 40, 6
    G, s2, sent, _, _, y = _rayleigh(rng, 1, J, n, order, 10.0)
    nb = 2 * soft.qam_bits(order)
    ref = pic.pic_detect(y, G, s2, s2, 0.0, 1.0)
    for prior in (rng.integers(-128, 128, (1, n, J, nb)).astype(np.int8), _genie(sent, order)):
        sbar, v = pic.prior_moments(prior, 2.0, order)
        v = np.maximum(v, 1e-3)                  # mu = Q / (Q v + s2): v = 0 cancels as well
        z, nu, _ = pic.pic_detect(y, G, s2, s2, sbar, v)
        assert np.abs(z - ref[0]).max() <= 1e-12 and np.abs(nu / ref[1] - 1.0).max() <= 1e-10
        a, b = pic.pic_frame(y, G, s2, s2, prior, 2.0, order), pic.pic_frame(y, G, s2, s2, None,
                                                                             2.0, order)
        assert np.array_equal(a["z"], b["z"]) and np.array_equal(a["llr"], b["llr"])


def test_information_follows_the_priors_at_18_db():
    """The 4x4 64-QAM 18 dB Rayleigh case of test_sic_softfb_model.py (J = 256 carriers x 40
    symbols, default_rng(1), perfect G, MMSE) with consistent Gaussian priors of standard
    deviation 0, 2, 4 as int8 at prior_scale 4: the GMI per bit of the output LLRs increases
    strictly, at sigma 0 it is within 0.01 of the linear detector's 0.820, and the measured over
    the predicted error power lies in [0.9, 1.1].
    Measured: GMI 0.820, 0.842, 0.935; ratios 0.989, 0.982, 0.996."""
    N, order, J, n = 4, 64, 256, 40
    rng = np.random.default_rng(1)
    G, s2, sent, s, _, y = _rayleigh(rng, N, J, n, order, 18.0)
    gmi, ratio = [], []
    for sigma in (0.0, 2.0, 4.0):
        prior = _gaussian_priors(np.random.default_rng(int(10 * sigma) + 5), sent, order, sigma, 4.0)
        out = pic.pic_frame(y, G, s2, s2, prior, 4.0, order)
        gmi.append(sic.llr_gmi(out["llr"], sent, order))
        ratio.append(float(np.mean(np.abs(out["z"] - s) ** 2) / np.mean(out["nu"])))
    print("GMI %s, measured / predicted error power %s" % (np.round(gmi, 3), np.round(ratio, 3)))
    assert gmi[0] < gmi[1] < gmi[2]
    assert abs(gmi[0] - 0.820) <= 0.01
    assert all(0.9 <= r <= 1.1 for r in ratio)


def _loop_errors(rng, N, order, J, n, snr_db, rate, passes=2, scale=4.0):
    """Random codewords, one per (stream, symbol) row of J carriers, through a Rayleigh channel
    per carrier; pic_frame -> int8 at `scale` -> fec.decode_siso (EXT) -> priors at the same
    scale -> pic_frame ... Returns the info-bit errors after every pass."""
    nb = 2 * soft.qam_bits(order)
    n_c = J * nb
    _, n_info, _ = fec.geometry(rate, n_c)
    info = rng.integers(0, 2, (N, n, n_info)).astype(np.uint8)
    sent = fec.qam_indices(fec.encode(rate, n_c, info), nb)                     # [N][n][J]
    s2 = 10.0 ** (-snr_db / 10.0)
    G = (rng.standard_normal((J, N, N)) + 1j * rng.standard_normal((J, N, N))) / np.sqrt(2.0)
    w = (rng.standard_normal((N, n, J)) + 1j * rng.standard_normal((N, n, J))) * np.sqrt(s2 / 2.0)
    y = _decode(G, np.einsum("jru,unj->rnj", G, sic.qam_points(sent, order)) + w, s2)
    prior, errs = None, []
    for _ in range(passes):
        out = pic.pic_frame(y, G, s2, s2, prior, scale, order, llr_scale=scale)
        rows = soft.quantise_i8(out["llr"]).reshape(N * n, n_c)
        ext, _, il, _ = fec.decode_siso(rate, n_c, rows, mode=fec.SISO_EXT)
        errs.append(int(np.sum((il[:, :n_info] < 0) != info.reshape(N * n, n_info))))
        prior = ext.reshape(N, n, J, nb)
    return errs


def test_the_loop_through_the_soft_output_decoder_removes_errors():
    """4x4 16-QAM, 64 carriers, rate 1/2, 7 dB, 96 rows, default_rng(3): info-bit errors after
    the first pass (zero priors), strictly fewer after the second. Measured: 62 -> 0."""
    errs = _loop_errors(np.random.default_rng(3), 4, 16, 64, 24, 7.0, fec.R12)
    print("info-bit errors per pass: %s" % errs)
    assert errs[0] > 0
    assert errs[1] < errs[0]


# ---- the kernel's arithmetic restated in float32 -------------------------------------------
def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _mac(acc, a, b):
    """sic_mac: acc += a b as two fused multiply-adds per component, a's real part first."""
    ar, ai = a
    xr = _fma(ai, -b[1], _fma(ar, b[0], acc[0]))
    xi = _fma(ai, b[0], _fma(ar, b[1], acc[1]))
    return xr, xi


def pic_detect_f32(G, s2, lam, y, sbar, v):
    """pic_detect of pic_kernels.hip in float32 numpy, operation for operation (the fused
    multiply-adds through float64 products): Q = G^H G in float64 rounded to float32, r = lam y +
    Q (y - sbar), A = Q diag(v) + s2 I, elimination of [A | r Q] without pivoting on the pivots'
    real parts, back-substitution for A^-1 r and the diagonal of A^-1 Q. y, sbar [N][n][J], v
    [N][n][J], all float32 / complex64. Returns (z^ complex128, nu float64) [N][n][J]."""
    f = np.float32
    N = G.shape[-1]
    Q = (np.conj(G.astype(np.complex128).transpose(0, 2, 1)) @ G.astype(np.complex128))
    Qr, Qi = Q.real.astype(f), Q.imag.astype(f)
    for t in range(N):
        Qi[:, t, t] = 0.0
        for u in range(t):                       # the lower triangle is the upper one's conjugate
            Qr[:, t, u], Qi[:, t, u] = Qr[:, u, t], -Qi[:, u, t]
    s2, lam = f(s2), f(lam)
    yr, yi = y.real.astype(f), y.imag.astype(f)
    sr, si = sbar.real.astype(f), sbar.imag.astype(f)
    v = v.astype(f)
    shape = yr[0].shape
    q = lambda t, u: (np.broadcast_to(Qr[None, :, t, u], shape), np.broadcast_to(Qi[None, :, t, u], shape))
    d = [(yr[u] - sr[u], yi[u] - si[u]) for u in range(N)]
    A = [[None] * N for _ in range(N)]
    X = [[None] * N for _ in range(N)]
    R = [None] * N
    for t in range(N):
        acc = (lam * yr[t], lam * yi[t])
        for u in range(N):
            acc = _mac(acc, q(t, u), d[u])
        R[t] = acc
        for c in range(N):
            A[t][c] = (q(t, c)[0] * v[c], q(t, c)[1] * v[c])
            X[t][c] = (q(t, c)[0].copy(), q(t, c)[1].copy())
        A[t][t] = (A[t][t][0] + s2, A[t][t][1])
    ip = [None] * N
    for c in range(N):
        ip[c] = f(1.0) / A[c][c][0]
        for rr in range(c + 1, N):
            nf = (-(A[rr][c][0] * ip[c]), -(A[rr][c][1] * ip[c]))
            for k in range(c + 1, N):
                A[rr][k] = _mac(A[rr][k], nf, A[c][k])
            R[rr] = _mac(R[rr], nf, R[c])
            for t in range(N):
                X[rr][t] = _mac(X[rr][t], nf, X[c][t])
    neg = lambda a: (-a[0], -a[1])
    x = [None] * N
    for i in range(N - 1, -1, -1):
        acc = R[i]
        for k in range(i + 1, N):
            acc = _mac(acc, neg(A[i][k]), x[k])
        x[i] = (acc[0] * ip[i], acc[1] * ip[i])
    z = np.zeros((N,) + shape, np.complex128)
    nu = np.zeros((N,) + shape, np.float64)
    for t in range(N):
        c = [None] * N
        for i in range(N - 1, t - 1, -1):
            acc = X[i][t]
            for k in range(i + 1, N):
                acc = _mac(acc, neg(A[i][k]), c[k])
            c[i] = (acc[0] * ip[i], acc[1] * ip[i])
        imu = f(1.0) / c[t][0]
        zr, zi = x[t][0] * imu + sr[t], x[t][1] * imu + si[t]
        assert zr.dtype == f and imu.dtype == f
        z[t] = zr.astype(np.float64) + 1j * zi.astype(np.float64)
        nu[t] = (imu - v[t]).astype(np.float64)
    return z, nu


# the GPU cases' geometries (tests/test_gpu_pic.py): N, QAM order, MMSE
RESTATED = [(2, 4, False), (2, 16, False), (4, 64, True), (4, 256, True), (1, 16, False)]


@pytest.mark.parametrize("N,order,mmse", RESTATED)
def test_float32_restatement_of_the_kernels_arithmetic(N, order, mmse):
    """The kernel's moments and elimination in float32 against the float64 model on the same
    complex64 G and the same prior bytes, 30 dB i.i.d. Rayleigh (2048 carriers x 4 symbols, every
    conditioning the estimate of a flat channel can have and worse), three kinds of priors
    (uniform random int8, all zero, genie +-127) at prior_scale 4 and 0.5. With u = 2^-24,
    kappa the 2-norm condition number of A and mag_t the sum of the magnitudes of the terms of
    r_t over Q[t][t] and of sbar_t (pic.pic_detect), it measures the worst
      |z32 - z64| / (u kappa mag)   and   |nu32 - nu64| / (u kappa (nu + v))
    and asserts them below pic.Z_RATIO_F32 and pic.NU_RATIO_F32, the recorded figures the GPU
    bounds are 8x of. Elimination without pivoting loses nothing to the pivoted float64 solve,
    also at v = 0: A is a column scaling of a Hermitian positive definite matrix.
    Measured worst ratios (z, nu): 2.50, 4.36 (2x2 QPSK), 2.78, 4.55 (2x2 16-QAM), 2.97, 6.12
    (4x4 64-QAM), 4.18, 5.07 (4x4 256-QAM), 2.74, 2.58 (1x1 16-QAM); with the second-moment form
    of the variance (M scale^2 - mean^2) in place of the subtraction-free one the nu ratio is
    41877: the variance is then off by 2^-23 absolute, 2e-3 of nu at 30 dB."""
    rng = np.random.default_rng(760 + N + order)
    J, n = 2048, 4
    G, s2, sent, _, X, _ = _rayleigh(rng, N, J, n, order, 30.0, mmse)
    G = G.astype(np.complex64)
    s2 = float(np.float32(s2))
    lam = s2 if mmse else 0.0
    y = _decode(G.astype(np.complex128), X, lam).astype(np.complex64)
    nb = 2 * soft.qam_bits(order)
    kinds = {"random": rng.integers(-128, 128, (N, n, J, nb)).astype(np.int8),
             "zero": np.zeros((N, n, J, nb), np.int8), "genie": _genie(sent, order)}
    wz = wn = 0.0
    for kind, prior in kinds.items():
        for ps in (4.0, 0.5):
            ref = pic.pic_frame(y, G, s2, lam, prior, ps, order, with_bound=True)
            sb32, v32 = pic.prior_moments_nested(prior, ps, order, dtype=np.float32)
            assert v32.dtype == np.float32
            if N == 1:                           # the kernel takes sbar = 0, v = 1 there
                sb32, v32 = np.zeros_like(sb32), np.ones_like(v32)
            z32, nu32 = pic_detect_f32(G, s2, lam, y, sb32, v32)
            kz = np.abs(z32 - ref["z"]) / (U * ref["cond"] * ref["mag"])
            kn = np.abs(nu32 - ref["nu"]) / (U * ref["cond"] * (ref["nu"] + ref["v"]))
            wz, wn = max(wz, float(kz.max())), max(wn, float(kn.max()))
    print("N %d %d-QAM: worst z ratio %.3f, worst nu ratio %.3f" % (N, order, wz, wn))
    assert wz <= pic.Z_RATIO_F32 and wn <= pic.NU_RATIO_F32


def test_null_handle_and_null_struct_are_argument_errors():
    L = _lib.lib()
    a = _lib.PicSoft(16, 32, 48, 64, 80, 1, 1, 0, _lib.LLR_I8, 1.0, 1.0)
    assert L.mimo_rx_pic_soft(None, C.byref(a), None) == -1
    assert L.mimo_rx_pic_soft(None, None, None) == -1
