"""The written definition of the layered tree-search detector (LORD; DESIGN.md "Layered tree
search", include/mimo_rx.h) as float64 numpy: what mimo_rx_lord_soft computes on the GPU (Q and
the factors U in fp64 stored as fp32, everything per symbol in fp32).

Per synced frame and occupied carrier: G the estimate [rx][tx], s2 the frame's noise_var,
Q = G^H G (stored as fp32), lam = s2 (MMSE) or 0 (ZF, ZF2 at N = 2), m = (Q + lam I) y the
matched-filter statistic recovered from the decode's y. The metric of a symbol vector s is
D(s) = s^H Q s - 2 Re(s^H m) = |X - G s|^2 up to a constant. Per target stream t:
  order    the other streams by decreasing Q[u][u] (the stored fp32 values, ties to the lower
           index) are o_0, o_1, ...; p = (o_(N-2), ..., o_0, t): the target is last, o_0 is
           detected first
  factor   U upper triangular, real positive diagonal, U^H U = P (Q + r I) P^T, r = s2
           whatever the detector (r = 0 at N = 2), stored as fp32
  chain    yt = U^-H (P m); for each of the L^2 values c of s_t in index order: s_(N-1) = c, and
           for k = N-2 .. 0: e_k = (yt_k - sum_{j>k} U_kj s_j) / U_kk, s_k = qam_point(slice(e_k))
  metric   D_c = sum_k |yt_k - sum_{j>=k} U_kj s_j|^2 - r sum_k |s_k|^2 = D(s) + |yt|^2
  LLR_i    llr_scale (min_{c: bit_i(c) = 1} D_c - min_{c: bit_i(c) = 0} D_c) / s2
  idx      the c with the smallest D_c, the lowest c on a tie
At N = 1 there is no chain: D_c = Q |c|^2 - 2 Re(c* m). At N = 2 the one sliced stream is the
exact minimiser, so the output is the max-log ML detector's. Rows the decode did not write,
carriers whose Q or U is not finite and frames with noise_var <= 0 or not finite are erased:
LLRs 0, idx 0.
"""
from __future__ import annotations

import numpy as np

from .sic import qam_demap_f32, qam_points
from .soft import qam_bits, qam_levels, quantise_i8

U32 = 2.0 ** -24


def _f32(a):
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return a.astype(np.complex64).astype(np.complex128)
    return a.astype(np.float32).astype(np.float64)


def lord_reg(N, s2):
    """The regularisation of the factor: s2 on a chain of two or more sliced streams, none at
    N = 2, where the one sliced stream must be the exact minimiser of D."""
    return float(s2) if N > 2 else 0.0


def lord_tables(G_occ, s2, fp32_tables=True):
    """The per-carrier tables of one frame. G_occ [J][N][N] ([rx][tx]). Returns (Q [J][N][N]
    complex128 holding the stored fp32 values, perm [J][N][N] int64 with perm[j][t] the
    permutation p of target t, U [J][N][N][N] complex128 holding the stored fp32 factors by
    target, erased [J]). Erased carriers (and all of them when s2 is not finite and positive)
    carry the tables of Q = I. fp32_tables=False keeps Q and U in float64 (the definition without
    its storage format, for the exactness tests)."""
    G = np.asarray(G_occ, np.complex128)
    J, N, _ = G.shape
    s2 = float(s2)
    with np.errstate(over="ignore", invalid="ignore"):
        Q64 = np.conj(G.transpose(0, 2, 1)) @ G
        Q = Q64.astype(np.complex64)
        if not fp32_tables:
            Q = Q64.copy()
        erased = ~np.all(np.isfinite(Q.reshape(J, -1)), axis=1)
    if not (s2 > 0.0 and np.isfinite(s2)):
        erased[:] = True
        s2 = 1.0
    Q = np.where(erased[:, None, None], np.eye(N), Q.astype(np.complex128))
    ar = np.arange(N)
    Q[:, ar, ar] = Q[:, ar, ar].real
    qd = Q[:, ar, ar].real                                                     # [J][N]
    perm = np.zeros((J, N, N), np.int64)
    for t in range(N):
        others = np.array([u for u in range(N) if u != t], np.int64)
        if N > 1:
            o = others[np.argsort(-qd[:, others], axis=1, kind="stable")]      # [J][N-1], o_0 first
            perm[:, t, :N - 1] = o[:, ::-1]
        perm[:, t, N - 1] = t
    U = np.zeros((J, N, N, N), np.complex128)
    A = Q + lord_reg(N, s2) * np.eye(N)
    for t in range(N):
        p = perm[:, t]
        Ap = np.take_along_axis(np.take_along_axis(A, p[:, :, None], 1), p[:, None, :], 2)
        with np.errstate(all="ignore"):
            try:
                Lc = np.linalg.cholesky(Ap)
            except np.linalg.LinAlgError:
                Lc = np.full(Ap.shape, np.nan, np.complex128)
                for j in range(J):
                    try:
                        Lc[j] = np.linalg.cholesky(Ap[j])
                    except np.linalg.LinAlgError:
                        pass
            Ut = np.conj(Lc.transpose(0, 2, 1))
            U[:, t] = _f32(Ut) if fp32_tables else Ut
    bad = ~np.all(np.isfinite(U.reshape(J, -1)), axis=1) | \
        ~np.all(U[:, :, ar, ar].real.reshape(J, -1) > 0, axis=1)
    if bad.any():
        erased = erased | bad
        Ui = np.sqrt(1.0 + lord_reg(N, s2)) * np.eye(N)
        U[bad] = _f32(Ui)
        Q[bad] = np.eye(N)
        perm[bad] = lord_tables(np.eye(N)[None], s2)[1][0]
    return Q, perm, U, erased


def _boundary(x, scale, L):
    """Per real dimension: the distance of x to the nearest decision boundary of the slicer and
    the two level indices (lo, lo + 1) on either side of that boundary."""
    xs = x / scale
    j = np.clip(np.rint(xs / 2.0), -(L // 2 - 1), L // 2 - 1)
    return np.abs(xs - 2.0 * j) * scale, (j + (L // 2 - 1)).astype(np.int64)


def _chain(yt, Ut, s, r, k0, pts, lv, qam, tau):
    """Steps k = k0 .. 0 of the chain on s, r (lists by position, arrays [n][J][C]); yt [n][J][N],
    Ut [J][N][N]. With tau ([N][n][J], or None) it returns per step the fragile flags of both
    dimensions and the alternative point across the nearest boundary."""
    N = Ut.shape[-1]
    L = len(lv)
    scale = float(lv[-1]) / (L - 1)
    frag = {}
    code = 0
    for k in range(k0, -1, -1):
        a = yt[:, :, k, None] + 0.0 * s[N - 1]
        for j in range(k + 1, N):
            a = a - Ut[None, :, k, j, None] * s[j]
        ukk = Ut[None, :, k, k, None].real
        e = a / ukk
        idx = qam_demap_f32(e, qam)
        s[k] = pts[idx]
        code = code | (_levels(idx, L) << (16 * k))
        r[k] = a - ukk * s[k]
        if tau is not None:
            out = []
            for x, main in ((e.real, s[k].real), (e.imag, s[k].imag)):
                d, lo = _boundary(x, scale, L)
                alt = np.where(main <= lv[lo], lv[np.minimum(lo + 1, L - 1)], lv[lo])
                out.append((d < tau[k][:, :, None], alt))
            frag[k] = out
    return frag, code


def _levels(idx, L):
    """The level pair of an index, mI | mQ << 8 (int64)."""
    b = L.bit_length() - 1
    g = np.asarray(idx).astype(np.int64)
    gi, gq = g >> b, g & (L - 1)
    for sft in (1, 2, 4):
        gi, gq = gi ^ (gi >> sft), gq ^ (gq >> sft)
    return gi | (gq << 8)


def _metric(s, r, s2):
    return sum(np.abs(x) ** 2 for x in r) - s2 * sum(np.abs(x) ** 2 for x in s)


def lord_detect(y, Q, perm, U, s2, lam, qam_order, with_bound=False, ratio=None):
    """The chains of every target. y [N][n][J]; Q, perm, U from lord_tables. Returns a dict: D
    [N][n][J][C] the metrics by target and candidate index, code [N][n][J][C] the chain's sliced
    levels (mI | mQ << 8, 16 bits per position); with_bound adds cond [J] (the 2-norm
    condition number of Q + r I), mag [N][n][J], tol [N][n][J] (8 ratio u cond mag),
    ambiguous [N][n][J] and ambiguous_two, the part of it that the first rule below flags.
    `ratio` defaults to D_RATIO_F32.

    mag, the magnitude sum of the metric's terms, bounds every candidate's:
    sum_k (|yt_k| + sum_{j>=k} |U_kj| c_max)^2 + r N c_max^2, c_max the corner point's modulus.
    For e_k it is (|yt_k| + sum_{j>k} |U_kj| c_max) / U_kk, and tau_k = 8 ratio u cond of that.

    A slicing is fragile when e_k lies within tau_k of a decision boundary in either dimension. A
    candidate with one fragile slicing gets both branches evaluated. An entry (stream, symbol,
    carrier) is ambiguous when a candidate has two or more fragile slicings (the other branch's
    own fragile slicings count), or when a fragile candidate's smaller branch metric lies within
    tol of, or below, one of the per-bit minima that candidate competes for. At N <= 2 the mask
    is empty: the one slicing at N = 2 picks the exact minimiser of a continuous function."""
    y = np.asarray(y, np.complex128)
    N, n, J = y.shape
    s2, lam = lord_reg(N, s2), float(lam)       # (s2 enters the chains as the regularisation)
    b = qam_bits(qam_order)
    C = 1 << (2 * b)
    lv = qam_levels(qam_order)
    pts = qam_points(np.arange(C), qam_order)                                   # [C]
    cmax = float(np.abs(pts).max())
    yj = y.transpose(1, 2, 0)                                                   # [n][J][N]
    m = np.einsum("jtu,nju->njt", Q, yj) + lam * yj
    D = np.zeros((N, n, J, C))
    codes = np.zeros((N, n, J, C), np.int64)
    out = {}
    if with_bound:
        ratio = D_RATIO_F32 if ratio is None else ratio
        cond = np.linalg.cond(Q + s2 * np.eye(N))
        mag = np.zeros((N, n, J))
        amb = np.zeros((N, n, J), bool)
        amb2 = np.zeros((N, n, J), bool)
    cc = np.broadcast_to(pts, (n, J, C))
    for t in range(N):
        if N == 1:
            q = Q[None, :, 0, 0, None].real
            D[0] = q * np.abs(cc) ** 2 - 2.0 * np.real(np.conj(cc) * m[:, :, 0, None])
            if with_bound:
                mag[0] = Q[None, :, 0, 0].real * cmax ** 2 + 2.0 * cmax * np.abs(m[:, :, 0])
            continue
        Ut = U[:, t]                                                            # [J][N][N]
        pm = np.take_along_axis(m, np.broadcast_to(perm[None, :, t, :], m.shape), 2)
        yt = np.zeros_like(pm)
        for k in range(N):                                                      # U^H yt = P m
            acc = pm[:, :, k]
            for j in range(k):
                acc = acc - np.conj(Ut[None, :, j, k]) * yt[:, :, j]
            yt[:, :, k] = acc / Ut[None, :, k, k].real
        aU = np.abs(Ut)
        tau = None
        if with_bound:
            me = np.zeros((N, n, J))
            for k in range(N):
                me[k] = np.abs(yt[:, :, k]) + cmax * aU[None, :, k, k + 1:].sum(-1)
                mag[t] += (me[k] + cmax * aU[None, :, k, k]) ** 2
            mag[t] += s2 * N * cmax ** 2
            tau = 8.0 * ratio * U32 * cond[None, None, :] * me / aU[:, np.arange(N), np.arange(N)].T[:, None, :]
        s, r = [None] * N, [None] * N
        s[N - 1] = cc
        r[N - 1] = yt[:, :, N - 1, None] - Ut[None, :, N - 1, N - 1, None].real * cc
        frag, codes[t] = _chain(yt, Ut, s, r, N - 2, pts, lv, qam_order, tau)
        D[t] = _metric(s, r, s2)
        if with_bound and N > 2:
            # N = 2: the one slicing picks the exact minimiser of a continuous function, so
            # either branch of a fragile slicing has the same metric to rounding: never ambiguous
            nfrag = sum(frag[k][d][0].astype(np.int64) for k in range(N - 1) for d in (0, 1))
            small = np.full(D[t].shape, np.inf)
            two = nfrag >= 2
            for k in range(N - 2, -1, -1):
                for dim in (0, 1):
                    fl, alt = frag[k][dim]
                    sa, ra = list(s), list(r)
                    sa[k] = alt + 1j * s[k].imag if dim == 0 else s[k].real + 1j * alt
                    ra[k] = r[k] + Ut[None, :, k, k, None].real * (s[k] - sa[k])
                    f2, _ = _chain(yt, Ut, sa, ra, k - 1, pts, lv, qam_order, tau)
                    more = False
                    for i in f2:
                        more = more | f2[i][0][0] | f2[i][1][0]
                    two = two | (fl & (nfrag == 1) & more)
                    small = np.where(fl & (nfrag == 1), np.minimum(small, _metric(sa, ra, s2)), small)
            tolD = 8.0 * ratio * U32 * cond[None, :] * mag[t]                   # [n][J]
            bits = (np.arange(C)[:, None] >> (2 * b - 1 - np.arange(2 * b))) & 1   # [C][2b]
            thr = np.full(D[t].shape, -np.inf)
            for i in range(2 * b):
                for v in (0, 1):
                    sel = bits[:, i] == v
                    mn = D[t][:, :, sel].min(-1)
                    thr[:, :, sel] = np.maximum(thr[:, :, sel], mn[:, :, None])
            near = (nfrag == 1) & (small <= thr + tolD[:, :, None])
            amb[t] = (two | near).any(-1)
            amb2[t] = two.any(-1)
    out["D"] = D
    out["code"] = codes
    if with_bound:
        tol = 8.0 * ratio * U32 * cond[None, None, :] * mag
        out.update(cond=cond, mag=mag, tol=tol, ambiguous=amb, ambiguous_two=amb2)
    return out


def delta_of(D, qam_order):
    """The LLR numerators [..., 2b] of metrics D [..., C]: min over the candidates with bit i = 1
    minus min over those with bit i = 0, bit 0 the index's most significant."""
    nb = 2 * qam_bits(qam_order)
    C = 1 << nb
    bits = (np.arange(C)[:, None] >> (nb - 1 - np.arange(nb))) & 1
    out = np.empty(D.shape[:-1] + (nb,))
    for i in range(nb):
        out[..., i] = D[..., bits[:, i] == 1].min(-1) - D[..., bits[:, i] == 0].min(-1)
    return out


def lord_frame(y, G_occ, s2, lam, qam_order, llr_scale=1.0, with_bound=False, fp32_tables=True):
    """One pass over the written symbols of a frame: y [N][n][J] the linear decode's output by
    stream, G_occ [J][N][N]. Returns a dict: llr (float64 [N][n][J][2b]), delta (the LLR
    numerators min1 - min0), idx (uint8), D and code [N][n][J][C] (lord_detect), gap [N][n][J]
    (second-best minus best D), the tables Q, perm, U (lord_tables), erased [J]; with_bound adds
    cond [J], mag, tol and ambiguous [N][n][J] (lord_detect). Erased entries are idx = 0, LLRs 0.
    fp32_tables=False keeps the tables in float64."""
    y = np.asarray(y, np.complex128)
    N, n, J = y.shape
    Q, perm, U, erased = lord_tables(G_occ, s2, fp32_tables)
    ok = float(s2) > 0.0 and np.isfinite(float(s2))
    s2e = float(s2) if ok else 1.0
    with np.errstate(invalid="ignore", over="ignore"):
        yy = np.where(erased[None, None, :], 0.0, y)
        res = lord_detect(yy, Q, perm, U, s2e, float(lam) if ok else 0.0, qam_order, with_bound)
        D = res["D"]
        delta = delta_of(D, qam_order)
        llr = float(llr_scale) * delta / s2e
    er = erased[None, None, :]
    llr = np.where(np.isnan(llr) | er[..., None], 0.0, llr)
    srt = np.sort(D, axis=-1)
    out = dict(llr=llr, delta=np.where(er[..., None], 0.0, delta),
               idx=np.where(er, 0, np.argmin(D, axis=-1)).astype(np.uint8), D=D,
               gap=srt[..., 1] - srt[..., 0], erased=erased, perm=perm, U=U, Q=Q,
               code=res["code"])
    if with_bound:
        out.update(cond=res["cond"], mag=res["mag"], tol=res["tol"],
                   ambiguous=res["ambiguous"] & ~er)
    return out


def lord_llr_i8(llr):
    """MIMO_LLR_I8 of lord_frame's llr."""
    return quantise_i8(llr)


# The float32 error of the kernel's arithmetic against this model, measured by
# tests/test_lord_model.py's restatement: the worst |dD32 - dD64| / (u cond mag), u = 2^-24, dD
# the difference of the two minima behind an LLR, rounded up. The GPU tests allow 8 times it.
D_RATIO_F32 = 1.5      # measured 1.44 (1x1 16-QAM); 0.79 at 2x2 QPSK, 0.046 at 4x4 64-QAM
