"""The written definition of the soft-input MMSE-PIC detector (DESIGN.md "Soft-input MMSE-PIC",
include/mimo_rx.h) as float64 numpy: what mimo_rx_pic_soft computes on the GPU (Q in fp64 stored
as fp32, everything per symbol in fp32).

Per synced frame and occupied carrier: G the estimate [rx][tx], s2 the frame's noise_var,
Q = G^H G, lam = s2 (MMSE) or 0 (ZF, ZF2 at N = 2), R = Q + lam I. The linear decode delivered
y = (Q + lam I)^-1 G^H X, so m = R y = G^H X is the matched-filter statistic. Per written symbol
and stream t:
  lam_i = prior[t][i] / prior_scale (the plain int8 value; positive = bit 0; values 0..b-1
  belong to Re, most significant bit first, values b..2b-1 to Im)
  per dimension over the L levels l_m: P(m) ~ exp(sum_i (bit_i(gray m) ? -lam_i/2 : +lam_i/2)),
  mean = sum P l, variance = max(sum P l^2 - mean^2, 0)
  sbar_t = mean(Re) + j mean(Im),  v_t = variance(Re) + variance(Im)
  A = Q diag(v) + s2 I,  r = m - Q sbar,  mu_t = (A^-1 Q)[t][t]
  z^_t = (A^-1 r)_t / mu_t + sbar_t,  nu_t = 1 / mu_t - v_t
  idx_t = slice(z^_t),  LLR_i = llr_scale delta_i(z^_t) / max(nu_t, 1e-30)
That is the unbiased MMSE estimate of s_t from X - sum_{u != t} g_u sbar_u with the residual
covariance G diag(v, v_t := 1) G^H + s2 I, in the N x N domain: stream t's own priors enter
neither z^_t nor nu_t, so the LLRs are extrinsic. Zero priors give sbar = 0, v = 1 and the
unbiased linear MMSE output of every stream; certain priors give nu_t = s2 / Q[t][t]; at N = 1
the priors cancel. Rows the decode did not write, carriers whose Q is not finite and frames with
noise_var <= 0 are erased: z^ = 0, idx = 0, LLRs 0.
"""
from __future__ import annotations

import numpy as np

from .sic import qam_demap_f32
from .soft import MSE_FLOOR, llr_delta, qam_bits, qam_levels, quantise_i8


def _natural(prior_i8, prior_scale):
    p = np.asarray(prior_i8)
    if p.dtype != np.int8:
        raise TypeError("priors are int8")
    return p.astype(np.float64) / float(prior_scale)


def prior_moments(prior_i8, prior_scale, qam_order, levels=None):
    """The definition: prior [..., 2b] int8 -> (sbar [...] complex128, v [...] float64), the
    softmax over the L levels of each dimension (`levels`: qam_point's fp32 levels unless
    given)."""
    b = qam_bits(qam_order)
    lam = _natural(prior_i8, prior_scale)
    lv = qam_levels(qam_order) if levels is None else np.asarray(levels, np.float64)
    m = np.arange(1 << b)
    gray = m ^ (m >> 1)
    sign = 1.0 - 2.0 * ((gray[:, None] >> (b - 1 - np.arange(b))) & 1)        # [L][b], +1 = bit 0

    def dim(l):
        e = 0.5 * np.einsum("...i,mi->...m", l, sign)
        e -= e.max(axis=-1, keepdims=True)
        P = np.exp(e)
        P /= P.sum(axis=-1, keepdims=True)
        mean = (P * lv).sum(axis=-1)
        return mean, np.maximum((P * lv * lv).sum(axis=-1) - mean * mean, 0.0)

    mr, vr = dim(lam[..., :b])
    mi, vi = dim(lam[..., b:])
    return mr + 1j * mi, vr + vi


def prior_moments_nested(prior_i8, prior_scale, qam_order, dtype=np.float64):
    """The same moments in the factorised form the kernel evaluates, in `dtype` arithmetic and
    the kernel's operation order: the reflected Gray map is
    x = -s_0 (2^(b-1) + s_1 (2^(b-2) + ... + s_(b-1))) scale with s_i = +-1 the bit signs, so
    with e = exp(-|lam_i|), t_i = tanh(lam_i / 2) = copysign((1 - e) / (1 + e), lam_i) and
    c_i = 1 - t_i^2 = 4 e / (1 + e)^2: from m = 1, V = 0 backwards V <- V + c_(i+1) m^2,
    m <- w + t_(i+1) m, w = 2^(b-1-i); mean = -t_0 m scale, variance = (V + c_0 m^2) scale^2
    (no subtraction: a small variance keeps its relative accuracy). Its levels are the exact
    products (2 m - (L - 1)) scale of the fp32 scale, which qam_point rounds to fp32 (a relative
    6e-8): in float64 it equals prior_moments on those exact levels to rounding."""
    f = dtype
    b = qam_bits(qam_order)
    L = 1 << b
    scale = np.float32(1.0 / np.sqrt(2.0 * (L * L - 1.0) / 3.0)).astype(f)
    p = np.asarray(prior_i8)
    if p.dtype != np.int8:
        raise TypeError("priors are int8")
    if f == np.float32:
        lam = p.astype(f) * (f(1.0) / f(prior_scale))
    else:
        lam = p.astype(f) / f(prior_scale)
    with np.errstate(under="ignore"):
        e = np.exp(-np.abs(lam)).astype(f)
        r = f(1.0) / (f(1.0) + e)
        t = np.copysign((f(1.0) - e) * r, lam).astype(f)
        c = ((f(4.0) * e) * r) * r

        def dim(t, c):
            m = np.ones(t.shape[:-1], f)
            V = np.zeros(t.shape[:-1], f)
            for i in range(b - 2, -1, -1):
                w = f(1 << (b - 1 - i))
                V = V + c[..., i + 1] * (m * m)
                m = w + t[..., i + 1] * m
            return -(t[..., 0] * m) * scale, (V + c[..., 0] * (m * m)) * (scale * scale)

        mr, vr = dim(t[..., :b], c[..., :b])
        mi, vi = dim(t[..., b:], c[..., b:])
    return mr + 1j * mi, vr + vi


def pic_detect(y, G_occ, s2, lam, sbar, v, with_bound=False):
    """One pass of the detector. y [N][n][J] the linear decode's output by stream, G_occ
    [J][N][N] ([rx][tx]), s2 and lam scalars, sbar (complex) and v [N][n][J]. Returns
    (z^ [N][n][J] complex128, nu [N][n][J], mu [N][n][J]). with_bound adds the 2-norm condition
    number of A, [n][J], and mag [N][n][J], the sum of the magnitudes of the terms of r_t, in
    units of the symbol (over Q[t][t]), and of sbar_t:
    (sum_u |Q[t][u]| (|y_u| + |sbar_u|) + lam |y_t|) / Q[t][t] + |sbar_t|."""
    y = np.asarray(y, np.complex128)
    N, n, J = y.shape
    G = np.asarray(G_occ, np.complex128)
    s2, lam = float(s2), float(lam)
    Q = np.conj(G.transpose(0, 2, 1)) @ G                                       # [J][N][N]
    sb = np.broadcast_to(np.asarray(sbar, np.complex128), y.shape)
    vv = np.broadcast_to(np.asarray(v, np.float64), y.shape)
    yt = y.transpose(1, 2, 0)                                                   # [n][J][N]
    st = sb.transpose(1, 2, 0)
    vt = vv.transpose(1, 2, 0)
    m = np.einsum("jtu,nju->njt", Q, yt) + lam * yt
    r = m - np.einsum("jtu,nju->njt", Q, st)
    A = Q[None] * vt[:, :, None, :] + s2 * np.eye(N)                            # [n][J][N][N]
    x = np.linalg.solve(A, r[..., None])[..., 0]
    X = np.linalg.solve(A, np.broadcast_to(Q[None], A.shape))
    mu = np.real(np.diagonal(X, axis1=-2, axis2=-1))                            # [n][J][N]
    z = x / mu + st
    nu = 1.0 / mu - vt
    out = (z.transpose(2, 0, 1), nu.transpose(2, 0, 1), mu.transpose(2, 0, 1))
    if with_bound:
        aq = np.abs(Q)
        qtt = np.real(np.diagonal(Q, axis1=1, axis2=2))[None]                   # [1][J][N]
        mag = (np.einsum("jtu,nju->njt", aq, np.abs(yt) + np.abs(st)) + lam * np.abs(yt)) / qtt \
            + np.abs(st)
        out += (np.linalg.cond(A), mag.transpose(2, 0, 1))
    return out


def pic_llr(z, nu, qam_order, llr_scale=1.0, erased=None):
    """Max-log LLRs [..., 2b] of z^ with its error power nu: llr_scale soft.llr_delta(z^) /
    max(nu, 1e-30), float64; a NaN gives 0, and so does what `erased` (bool, broadcast against
    z) marks."""
    shape = np.shape(z)
    nu = np.maximum(np.broadcast_to(np.asarray(nu, np.float64), shape), MSE_FLOOR)
    with np.errstate(invalid="ignore", over="ignore"):
        out = llr_scale * llr_delta(z, qam_order) / nu[..., None]
    out = np.where(np.isnan(out), 0.0, out)
    if erased is not None:
        out = np.where(np.broadcast_to(np.asarray(erased, bool), shape)[..., None], 0.0, out)
    return out


def pic_llr_i8(z, nu, qam_order, llr_scale=1.0, erased=None):
    """MIMO_LLR_I8 of pic_llr."""
    return quantise_i8(pic_llr(z, nu, qam_order, llr_scale, erased))


def pic_frame(y, G_occ, s2, lam, prior_i8, prior_scale, qam_order, llr_scale=1.0,
              with_bound=False):
    """One pass over the written symbols of a frame: y [N][n][J], prior_i8 [N][n][J][2b] int8
    or None (all zero). Returns a dict: z, idx (uint8), nu, mu, llr (float64 [N][n][J][2b]),
    sbar, v, erased [J] (carriers whose Q is not finite, and every carrier when s2 <= 0), and
    with_bound cond [n][J] and mag [N][n][J]. Erased entries are z = 0, idx = 0, LLRs 0."""
    y = np.asarray(y, np.complex128)
    N, n, J = y.shape
    b = qam_bits(qam_order)
    if prior_i8 is None:
        prior_i8 = np.zeros((N, n, J, 2 * b), np.int8)
    if N == 1:
        sbar, v = np.zeros(y.shape, np.complex128), np.ones(y.shape)
    else:
        sbar, v = prior_moments(prior_i8, prior_scale, qam_order)
    G = np.asarray(G_occ, np.complex128)
    Q = np.conj(G.transpose(0, 2, 1)) @ G
    with np.errstate(over="ignore", invalid="ignore"):
        erased = ~np.all(np.isfinite(Q.astype(np.complex64).reshape(J, -1)), axis=1)
    if not (float(s2) > 0.0):
        erased[:] = True
    Gs = np.where(erased[:, None, None], np.eye(N), G)
    res = pic_detect(y, Gs, s2 if s2 > 0 else 1.0, lam, sbar, v, with_bound=with_bound)
    z = np.where(erased[None, None, :], 0.0, res[0])
    idx = np.where(erased[None, None, :], 0, qam_demap_f32(z, qam_order)).astype(np.uint8)
    out = dict(z=z, idx=idx, nu=res[1], mu=res[2], sbar=sbar, v=v, erased=erased,
               llr=pic_llr(z, res[1], qam_order, llr_scale, erased[None, None, :]))
    if with_bound:
        out.update(cond=res[3], mag=res[4])
    return out


# The float32 error of the kernel's arithmetic against this model, measured by
# tests/test_pic_model.py's restatement: the worst |z32 - z64| / (u kappa(A) mag) and
# |nu32 - nu64| / (u kappa(A) (nu + v)), u = 2^-24, rounded up. The GPU tests allow 8 times these.
Z_RATIO_F32 = 4.2      # measured 4.18 (4x4 256-QAM, random priors)
NU_RATIO_F32 = 6.2     # measured 6.13 (4x4 64-QAM, random priors at prior_scale 0.5)
