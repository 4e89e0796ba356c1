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
