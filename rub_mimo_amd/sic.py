"""The written definition of the ordered MMSE-SIC detector (DESIGN.md "SIC detection",
include/mimo_rx.h) as float64 numpy: what mimo_rx_sic_detect, mimo_rx_sic_order and
mimo_rx_sic_mse compute on the GPU (tables in fp64 stored as fp32, symbols in fp32).

Per synced frame and occupied carrier: G the estimate [rx][tx], s2 the frame's noise_var,
Q = G^H G, lam = s2 (MMSE) or 0 (ZF, ZF2 at N = 2), R = Q + lam I. The linear decode delivered
y = (Q + lam I)^-1 G^H X, so R y = G^H X is the matched-filter statistic. Stage k = 0..N-1 with
S the undetected streams and pi_0..pi_(k-1) the detected ones:
  E = (Q[S,S] + s2 I)^-1;  pi_k = argmin_S Re E[t][t] (ties: lowest t);  r = E[pi_k][:]
  beta = 1 - s2 E[pi_k][pi_k]
  T[k][u] = sum_{v in S} r_v R[v][u] / beta        (u = 0..N-1)
  C[k][i] = sum_{v in S} r_v Q[v][pi_i] / beta     (i < k)
  nu_sic[pi_k] = s2 E[pi_k][pi_k] / beta           (= (1 - beta) / beta)
  z_(pi_k) = sum_u T[k][u] y_u - sum_{i<k} C[k][i] s^_(pi_i);  s^_(pi_k) = slice(z_(pi_k))
A carrier whose solve fails at any stage gets zero tables, order 0..N-1 and nu_sic 0.

Soft output (mimo_rx_sic_soft): the same stages, every one still cancelling its hard decision,
and per stage the max-log LLRs of its z,
  LLR_i = llr_scale delta_i(z_(pi_k)) / max(nu_sic[pi_k], 1e-30)
with delta_i the soft output's numerator (soft.llr_delta: min over the levels with bit i = 1
minus min over the levels with bit i = 0, bit 0 the index's most significant bit, values
0..b-1 from Re z and b..2b-1 from Im z, positive = bit 0). z is unbiased, so a non-zero LLR's
sign is the matching bit of the stage's index. A NaN z gives 0, and so does every carrier whose
solve failed: that is not the good carrier with nu_sic = 0 because s2 = 0, which takes the
floor. nu_sic assumes perfect cancellation: error propagation is not in the weight.

Soft feedback (mimo_rx_sic_soft_fb; soft_symbol, sic_apply_soft): the order, T, C and nu_sic
above, but a stage cancels the expected symbols of the earlier stages and carries their
variances in its weight. With l_m the levels (qam_levels), per symbol and stage k:
  z_k = sum_u T[k][u] y_u - sum_{i<k} C[k][i] sbar_i
  nu_k = nu_sic[pi_k] + sum_{i<k} |C[k][i]|^2 v_i
  idx_k = slice(z_k);  LLR_i = llr_scale delta_i(z_k) / max(nu_k, 1e-30)
  per dimension x of z_k: p_m ~ exp(-(x - l_m)^2 / max(nu_k, 1e-30)) (the complex error power
  nu_k is nu_k / 2 per real dimension), mean = sum p_m l_m, variance = sum p_m l_m^2 - mean^2
  floored at 0;  sbar_k = mean(Re) + j mean(Im),  v_k = variance(Re) + variance(Im)
The posterior is evaluated relative to the slicer's level l_c of x: t = x - l_c, o_m = l_m - l_c,
w_m = exp(-max(o_m (o_m - 2 t), 0) / nu_k), mean = l_c + sum w o / sum w, variance =
sum w o^2 / sum w - (sum w o / sum w)^2: the same posterior (l_c is the nearest level, so the
floor only acts on the slicer's rounding at a boundary), with no weight above 1 and the
slicer's own equal to 1, so that nothing overflows or becomes 0/0 for any z or nu. Stage 0, and
all of N = 1, is the soft output above; nu -> 0 gives the hard point and v = 0.
"""
from __future__ import annotations

import numpy as np

from .soft import MSE_FLOOR, llr_delta, qam_bits, qam_levels


def qam_inv_scale(qam_order):
    """The float32 inv_scale = sqrt(2 (L^2 - 1) / 3) of the device's Qam (make_qam)."""
    L = 1 << qam_bits(qam_order)
    return np.float32(np.sqrt(2.0 * (L * L - 1.0) / 3.0))


def qam_demap_f32(z, qam_order):
    """qam_demap (common.hpp) restated in float32, operation for operation: per dimension
    m = clamp(floorf((v * inv_scale + L) * 0.5f), 0, L - 1), 0 for a NaN, and the index
    (gray(mI) << b) | gray(mQ). z complex (rounded to complex64 first); returns uint8."""
    b = qam_bits(qam_order)
    L = 1 << b
    inv = qam_inv_scale(qam_order)
    z = np.asarray(z).astype(np.complex64)

    def level(v):
        with np.errstate(invalid="ignore", over="ignore"):
            t = (v.astype(np.float32) * inv + np.float32(L)) * np.float32(0.5)
            f = np.floor(t)
        f = np.where(np.isnan(t), np.float32(0.0), f)
        return np.clip(f, 0, L - 1).astype(np.uint32)

    mi, mq = level(z.real), level(z.imag)
    return (((mi ^ (mi >> 1)) << b) | (mq ^ (mq >> 1))).astype(np.uint8)


def qam_points(idx, qam_order):
    """qam_point of index arrays: the float32 constellation points as complex128."""
    b = qam_bits(qam_order)
    L = 1 << b
    lv = qam_levels(qam_order)
    idx = np.asarray(idx).astype(np.uint32)

    def gray_dec(g):
        m = g.copy()
        for s in (1, 2, 4, 8):
            m ^= m >> s
        return m

    return lv[gray_dec(idx >> b)] + 1j * lv[gray_dec(idx & (L - 1))]


def _inv_or_none(A):
    try:
        E = np.linalg.inv(A)
    except np.linalg.LinAlgError:
        return None
    return E


def sic_tables(G, noise_var, lam, order=None):
    """Detection order and tables of J carriers. G [J][N][N] ([rx][tx]), noise_var = s2 and lam
    scalars; order [J][N] forces the detection order (else the smallest-MSE rule).
    Returns (order [J][N] uint8, T [J][N][N], C [J][N][N] with C[j][k][i] = 0 for i >= k,
    nu_sic [J][N] indexed by stream), float64 / complex128."""
    G = np.asarray(G, np.complex128)
    J, N = G.shape[0], G.shape[-1]
    s2, lam = float(noise_var), float(lam)
    eye = np.eye(N)
    Q = np.conj(G.transpose(0, 2, 1)) @ G
    R = Q + lam * eye
    forced = None if order is None else np.asarray(order, np.int64).reshape(J, N)
    out_order = np.zeros((J, N), np.int64)
    T = np.zeros((J, N, N), np.complex128)
    Ct = np.zeros((J, N, N), np.complex128)
    nu = np.zeros((J, N), np.float64)
    done = np.zeros((J, N), bool)          # detected streams
    bad = np.zeros(J, bool)
    ar = np.arange(J)
    for k in range(N):
        # (Q[S,S] + s2 I)^-1 as the S block of the inverse of the matrix whose detected rows and
        # columns are the identity's
        A = Q + s2 * eye
        A = np.where(done[:, :, None] | done[:, None, :], eye[None], A)
        E = _inv_or_none(A)
        if E is None:                      # some carrier is singular: one by one
            E = np.zeros_like(A)
            for j in range(J):
                Ej = _inv_or_none(A[j])
                if Ej is None:
                    bad[j] = True
                else:
                    E[j] = Ej
        d = np.real(np.diagonal(E, axis1=1, axis2=2)).copy()
        bad |= ~np.all(np.isfinite(E.reshape(J, -1)), axis=1)
        d[done] = np.inf
        d[bad] = 0.0
        pi = np.argmin(d, axis=1) if forced is None else forced[:, k]
        pi = np.where(bad, 0, pi)
        e = np.real(E[ar, pi, pi])
        beta = 1.0 - s2 * e
        bad |= ~(e > 0.0) | ~(beta > 0.0)
        beta = np.where(bad, 1.0, beta)
        r = np.where(done, 0.0, E[ar, pi, :])                     # [J][N], zero off S
        T[:, k, :] = np.einsum("jv,jvu->ju", r, R) / beta[:, None]
        rq = np.einsum("jv,jvu->ju", r, Q) / beta[:, None]
        for i in range(k):
            Ct[:, k, i] = rq[ar, out_order[:, i]]
        nu[ar, pi] = s2 * e / beta
        out_order[:, k] = pi
        done[ar, pi] = True
    T[bad] = 0.0
    Ct[bad] = 0.0
    nu[bad] = 0.0
    out_order[bad] = np.arange(N)
    return out_order.astype(np.uint8), T, Ct, nu


def sic_stage_mse(G, noise_var, order):
    """For a given (partial or full) order [J][N]: the candidate MSEs s2 E[t][t] / beta_t of
    every stream at every stage, [J][N(stage)][N(stream)], inf for streams already detected.
    What the ordering rule compares (the tests use it to find near-ties)."""
    G = np.asarray(G, np.complex128)
    J, N = G.shape[0], G.shape[-1]
    s2 = float(noise_var)
    eye = np.eye(N)
    Q = np.conj(G.transpose(0, 2, 1)) @ G
    order = np.asarray(order, np.int64).reshape(J, N)
    done = np.zeros((J, N), bool)
    out = np.full((J, N, N), np.inf)
    ar = np.arange(J)
    for k in range(N):
        A = np.where(done[:, :, None] | done[:, None, :], eye[None], Q + s2 * eye)
        d = np.real(np.diagonal(np.linalg.inv(A), axis1=1, axis2=2)).copy()
        d[done] = np.inf
        out[:, k, :] = d
        done[ar, order[:, k]] = True
    return out


def sic_apply(y, order, T, C, qam_order, decided=None, with_mag=False):
    """The symbol pass. y [N][n_sym][J] the linear decode's output by stream; order, T, C as
    sic_tables returns them. Returns (z [N][n_sym][J] complex128, idx [N][n_sym][J] uint8), both
    by stream. With `decided` ([N][n_sym][J] indices by stream) every stage cancels the given
    earlier decisions instead of its own (teacher forcing). with_mag adds the magnitude sum
    sum_u |T[k][u]| |y_u| + sum_{i<k} |C[k][i]| |s^_(pi_i)| of each z, by stream."""
    y = np.asarray(y, np.complex128)
    N, n, J = y.shape
    order = np.asarray(order, np.int64).reshape(J, N)
    T = np.asarray(T, np.complex128)
    C = np.asarray(C, np.complex128)
    z = np.zeros((N, n, J), np.complex128)
    idx = np.zeros((N, n, J), np.uint8)
    mag = np.zeros((N, n, J), np.float64)
    ar = np.arange(J)
    shat = []
    ay = np.abs(y)
    for k in range(N):
        pi = order[:, k]
        zk = np.einsum("ju,unj->nj", T[:, k, :], y)
        mk = np.einsum("ju,unj->nj", np.abs(T[:, k, :]), ay)
        for i in range(k):
            zk = zk - C[:, k, i][None, :] * shat[i]
            mk = mk + np.abs(C[:, k, i])[None, :] * np.abs(shat[i])
        ik = qam_demap_f32(zk, qam_order)
        z[pi, :, ar] = zk.T
        idx[pi, :, ar] = ik.T
        mag[pi, :, ar] = mk.T
        use = ik if decided is None else np.asarray(decided)[pi, :, ar].T
        shat.append(qam_points(use, qam_order))
    return (z, idx, mag) if with_mag else (z, idx)


def failed_carriers(T):
    """The carriers whose solve failed, [J] bool, read off tables T [J][N][N] as sic_tables
    returns them: a failed carrier's tables are all zero, and a good carrier's never are
    (T[k][pi_k] is not 0)."""
    T = np.asarray(T)
    return ~np.any(T.reshape(T.shape[0], -1) != 0, axis=1)


def sic_llr(z, nu_sic, qam_order, llr_scale=1.0, failed=None):
    """Max-log LLRs [..., 2b] of the stage outputs z with their post-SIC error power nu_sic
    (broadcast against z): llr_scale * soft.llr_delta(z) / max(nu_sic, 1e-30), float64.
    Positive = bit 0; value i belongs to bit i of the stage's index counted from its most
    significant bit. A NaN z gives 0; `failed` (bool, broadcast against z) marks the carriers
    whose solve failed: they give 0, whereas a good carrier with nu_sic = 0 takes the floor."""
    shape = np.shape(z)
    nu = np.maximum(np.broadcast_to(np.asarray(nu_sic, np.float64), shape), MSE_FLOOR)
    with np.errstate(invalid="ignore", over="ignore"):
        out = llr_scale * llr_delta(z, qam_order) / nu[..., None]
    out = np.where(np.isnan(out), 0.0, out)
    if failed is not None:
        out = np.where(np.broadcast_to(np.asarray(failed, bool), shape)[..., None], 0.0, out)
    return out


def soft_symbol(z, nu, qam_order):
    """Posterior mean and variance of the symbol behind z = s + e, e ~ CN(0, nu), s uniform on
    the constellation: per dimension p_m ~ exp(-(x - l_m)^2 / max(nu, 1e-30)), evaluated in the
    offset form of the module docstring around the slicer's level (qam_demap_f32). z complex, nu
    broadcast against it. Returns (sbar complex128, v float64 = Re variance + Im variance)."""
    z = np.asarray(z, np.complex128)
    lv = qam_levels(qam_order)
    nu = np.maximum(np.broadcast_to(np.asarray(nu, np.float64), z.shape), MSE_FLOOR)
    pt = qam_points(qam_demap_f32(z, qam_order), qam_order)

    def dim(x, lc):
        o = lv - lc[..., None]                                   # [..., L]
        with np.errstate(invalid="ignore", over="ignore"):
            e = np.fmax(o * (o - 2.0 * (x - lc)[..., None]), 0.0)
            w = np.exp(-e / nu[..., None])
        sw = w.sum(axis=-1)
        m = (w * o).sum(axis=-1) / sw
        return lc + m, np.maximum((w * o * o).sum(axis=-1) / sw - m * m, 0.0)

    mr, vr = dim(z.real, pt.real)
    mi, vi = dim(z.imag, pt.imag)
    return mr + 1j * mi, vr + vi


def sic_apply_soft(y, order, T, C, nu_sic, qam_order, fed_z=None, with_mag=False):
    """The symbol pass with soft feedback. y [N][n_sym][J] the linear decode's output by
    stream; order, T, C, nu_sic ([J][N] by stream) as sic_tables returns them. Returns
    (z [N][n_sym][J] complex128, idx [N][n_sym][J] uint8, nu [N][n_sym][J] float64 the error
    power nu_k that weights the stage's LLRs), all by stream. With `fed_z` ([N][n_sym][J] by
    stream) stage k's sbar_i and v_i are computed from the given earlier z, with the model's own
    nu_i, instead of from its own z (teacher forcing). with_mag adds the magnitude sum
    sum_u |T[k][u]| |y_u| + sum_{i<k} |C[k][i]| |sbar_i| of each z, by stream."""
    y = np.asarray(y, np.complex128)
    N, n, J = y.shape
    order = np.asarray(order, np.int64).reshape(J, N)
    T = np.asarray(T, np.complex128)
    C = np.asarray(C, np.complex128)
    nu_sic = np.asarray(nu_sic, np.float64).reshape(J, N)
    z = np.zeros((N, n, J), np.complex128)
    idx = np.zeros((N, n, J), np.uint8)
    nu = np.zeros((N, n, J), np.float64)
    mag = np.zeros((N, n, J), np.float64)
    ar = np.arange(J)
    sbar, var = [], []
    ay = np.abs(y)
    for k in range(N):
        pi = order[:, k]
        zk = np.einsum("ju,unj->nj", T[:, k, :], y)
        mk = np.einsum("ju,unj->nj", np.abs(T[:, k, :]), ay)
        nk = np.broadcast_to(nu_sic[ar, pi][None, :], (n, J)).copy()
        for i in range(k):
            zk = zk - C[:, k, i][None, :] * sbar[i]
            mk = mk + np.abs(C[:, k, i])[None, :] * np.abs(sbar[i])
            nk = nk + (np.abs(C[:, k, i]) ** 2)[None, :] * var[i]
        z[pi, :, ar] = zk.T
        idx[pi, :, ar] = qam_demap_f32(zk, qam_order).T
        nu[pi, :, ar] = nk.T
        mag[pi, :, ar] = mk.T
        src = zk if fed_z is None else np.asarray(fed_z, np.complex128)[pi, :, ar].T
        sb, vv = soft_symbol(src, nk, qam_order)
        sbar.append(sb)
        var.append(vv)
    return (z, idx, nu, mag) if with_mag else (z, idx, nu)


def llr_gmi(llr, sent_idx, qam_order):
    """Generalised mutual information per bit of LLRs [..., 2b] (positive = bit 0) against the
    transmitted indices sent_idx [...]: 1 - E log2(1 + exp(-LLR)) over the bits sent as 0 and
    1 - E log2(1 + exp(+LLR)) over those sent as 1, bit i counted from the index's most
    significant bit. The rate a bit-interleaved decoder fed these LLRs could reach."""
    nb = 2 * qam_bits(qam_order)
    llr = np.asarray(llr, np.float64)
    sent = np.asarray(sent_idx).astype(np.int64)
    bits = (sent[..., None] >> (nb - 1 - np.arange(nb))) & 1
    return 1.0 - float(np.mean(np.logaddexp(0.0, np.where(bits == 1, llr, -llr)))) / np.log(2.0)
