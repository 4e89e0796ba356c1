"""The written definition of the soft output (DESIGN.md "Soft output", include/mimo_rx.h) as
float64 numpy: what mimo_rx_batch_mse and mimo_rx_soft_demap compute on the GPU in fp32.

Model per occupied subcarrier k (carrier j) of a synced frame: the decode's input is
X = G s + n with E|s_u|^2 = 1 and n ~ CN(0, s2 I), s2 the frame's noise_var, and it delivers
y_t = g_k sum_r W[t][r] X_r.
"""
from __future__ import annotations

import numpy as np

MSE_FLOOR = 1e-30


def qam_bits(qam_order):
    """Bits per dimension b of a square QAM of order L^2 = 4^b."""
    b = 0
    while (1 << (2 * b)) < qam_order:
        b += 1
    if (1 << (2 * b)) != qam_order or b < 1:
        raise ValueError("qam_order must be 4, 16, 64 or 256")
    return b


def qam_levels(qam_order):
    """The L per-dimension levels l_m = (2m - (L-1)) scale of the pipeline's constellation
    (unit mean symbol energy): scale and the product are float32, as qam_point computes them
    on the device and in the oracle; returned as float64."""
    L = 1 << qam_bits(qam_order)
    scale = np.float32(1.0 / np.sqrt(2.0 * (L * L - 1.0) / 3.0))
    return ((2 * np.arange(L) - (L - 1)).astype(np.float32) * scale).astype(np.float64)


def mse_terms(G, W, gain, noise_var, occ):
    """The two terms of the post-detection MSE, each [N][M_occ] float64: the noise enhancement
    g^2 s2 sum_r |W[t][r]|^2 and the residual interference plus bias
    sum_u |g sum_r W[t][r] G[r][u] - delta_tu|^2 (arguments as mse_reference)."""
    occ = np.asarray(occ, np.int64)
    G = np.asarray(G, np.complex128)[occ]
    W = np.asarray(W, np.complex128)[occ]
    g = np.asarray(gain, np.float64).reshape(-1)
    N = G.shape[-1]
    noise = g ** 2 * float(noise_var) * np.sum(np.abs(W) ** 2, axis=2).T      # [t][j]
    C = g[:, None, None] * (W @ G) - np.eye(N)                                # [j][t][u]
    return noise, np.sum(np.abs(C) ** 2, axis=2).T


def mse_reference(G, W, gain, noise_var, occ):
    """Post-detection MSE nu[t][j], the predicted E|y_t - s_t|^2.

    G [M][N][N] ([sc][rx][tx]), W [M][N][N] ([sc][out][rx]), gain [M_occ], occ the M_occ
    occupied subcarrier indices in carrier order. Returns [N][M_occ] float64:
      nu[t][j] = g^2 s2 sum_r |W[t][r]|^2 + sum_u |g sum_r W[t][r] G[r][u] - delta_tu|^2
    """
    noise, isi = mse_terms(G, W, gain, noise_var, occ)
    return noise + isi


def _dim_delta(x, qam_order):
    """min over levels with bit i = 1 minus min over levels with bit i = 0 of (x - l_m)^2,
    bit 0 the most significant bit of gray(m): [..., b]."""
    b = qam_bits(qam_order)
    lv = qam_levels(qam_order)
    m = np.arange(1 << b)
    gray = m ^ (m >> 1)
    d2 = (np.asarray(x, np.float64)[..., None] - lv) ** 2                     # [..., L]
    out = np.empty(d2.shape[:-1] + (b,), np.float64)
    for i in range(b):
        one = ((gray >> (b - 1 - i)) & 1) == 1
        out[..., i] = d2[..., one].min(axis=-1) - d2[..., ~one].min(axis=-1)
    return out


def llr_delta(y, qam_order):
    """The LLR numerators of complex y, [..., 2b]: bits 0..b-1 from Re y, b..2b-1 from Im y."""
    y = np.asarray(y, np.complex128)
    return np.concatenate([_dim_delta(y.real, qam_order), _dim_delta(y.imag, qam_order)], axis=-1)


def llr_reference(y, nu, qam_order, llr_scale=1.0):
    """Max-log LLRs [..., 2b] of equalised symbols y with post-detection MSE nu (broadcast
    against y): llr_scale * delta / max(nu, 1e-30). Positive = bit 0; bit i is bit i of the
    index (gray(mI) << b) | gray(mQ) counted from its most significant bit. NaN y gives 0."""
    nu = np.maximum(np.broadcast_to(np.asarray(nu, np.float64), np.shape(y)), MSE_FLOOR)
    with np.errstate(invalid="ignore"):
        out = llr_scale * llr_delta(y, qam_order) / nu[..., None]
    return np.where(np.isnan(out), 0.0, out)


def quantise_i8(llr):
    """MIMO_LLR_I8 of LLR values: round half to even, clamp to [-127, 127], int8."""
    v = np.rint(np.nan_to_num(np.asarray(llr), nan=0.0, posinf=127.0, neginf=-127.0))
    return np.clip(v, -127, 127).astype(np.int8)
