"""The written definition of the channel code over the int8 LLR rows (DESIGN.md "Viterbi
decoder", include/mimo_rx.h) as integer numpy, and the ctypes wrapper of the mimo_fec_* calls.
What mimo_fec_encode computes on the host and mimo_fec_decode on the GPU (fec_kernels.hip),
bit for bit: everything is integer arithmetic, so there are no tolerances.

Encoder: the 802.11 mother code, K = 7, generators 133 / 171 octal. Info bits u_0..u_(n_info-1),
then six zero tail bits: T = n_info + 6 trellis steps, u_t = 0 for t < 0, and the trellis
starts and ends in the all-zero state.
  A_t = u_t ^ u_(t-2) ^ u_(t-3) ^ u_(t-5) ^ u_(t-6)        (133)
  B_t = u_t ^ u_(t-1) ^ u_(t-2) ^ u_(t-3) ^ u_(t-6)        (171)
Rates (the 802.11 puncturing patterns): R12 sends every A_t and B_t; R23 has period 2 and keeps
A in steps {1,1}, B in {1,0}; R34 has period 3 and keeps A in {1,1,0}, B in {1,0,1} (sent order
A1 B1 A2 B3). Sent order: for t = 0..T-1, A_t if kept, then B_t if kept: coded bits
k = 0..n_tx-1. A codeword is one row of n_c values; T is the largest step count with
n_tx(T) <= n_c. Coded bit k sits at row position perm[k] (perm None: k); positions no coded bit
refers to are ignored by the decoder and 0 from the encoder.

Decoder: maximum likelihood over the terminated trellis, full traceback from state 0. State
s = u_(t-1) | u_(t-2) << 1 | ... | u_(t-6) << 5, so state s at step t is entered with u_t = s & 1
from p0 = s >> 1 (u_(t-6) = 0) or p1 = p0 | 32 (u_(t-6) = 1). LLRs are positive for bit 0; a
punctured bit has LLR 0. The metric of a transition with outputs (a, b) is
(a ? -L_A : L_A) + (b ? -L_B : L_B) on the plain int8 values (-128 is -128). Path metrics start
at 0 in state 0 and at -2^30 elsewhere, are never normalised (the largest reachable magnitude is
2 * 128 * 24576), the larger one survives and a tie keeps p0. Outputs per row: the n_info bits
packed MSB first (bit k at byte k >> 3, mask 0x80 >> (k & 7)), zero up to the pitch, and the
final metric of state 0. An all-zero row decodes to zero bits and metric 0.

Soft-output decoder (mimo_fec_siso, DESIGN.md "Soft-output decoder"): max-log-MAP over the same
trellis, branch metric g_t(p->s) and rows. alpha_0 and beta_T are 0 in state 0 and NEG = -2^29
elsewhere (not -2^30: for T < 12 a state can be unreachable from both ends, and alpha + g + beta
must stay in int32); alpha_(t+1)(s) = max over the two predecessors of alpha_t(p) + g_t(p->s),
beta_t(p) = max over the two successors of g_t(p->s) + beta_(t+1)(s); nothing is normalised. For
x in {u_t, A_t, B_t}: M(v) = max over the transitions with x = v of alpha_t(p) + g_t(p->s) +
beta_(t+1)(s) and Lambda = M(0) - M(1). d_out receives clamp(Lambda, +-127) (APP) or
clamp(Lambda - L_in, +-127) (EXT) at the row position of every kept coded bit and nothing
elsewhere; info bit k is Lambda_k^u < 0 (a tie gives 0), the info LLR clamp(Lambda_k^u, +-127),
the metric alpha_T(0), which is the Viterbi metric.

Encoder on the device (mimo_fec_encode_rows, DESIGN.md "Coded transmit"): encode_rows is what it
writes, from info bits in the packed format above (unpack_bits; whatever lies past bit n_info is
ignored): the rows of encode (ENC_BITS), or those rows through rows_to_idx (ENC_QAM):
idx[j] = sum over i < 2b of row[2b j + i] << (2b - 1 - i), the inverse of the order in which the
soft passes write a carrier's 2b LLRs.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

R12, R23, R34 = 0, 1, 2
RATES = (R12, R23, R34)
TAIL = 6
N_STATES = 64
MAX_NC = 32768
M_INIT = -(1 << 30)
NEG_SISO = -(1 << 29)
SISO_APP, SISO_EXT = 0, 1
# kept (1) / punctured (0) per step of the period, for A and for B
KEEP = {R12: ((1,), (1,)), R23: ((1, 1), (1, 0)), R34: ((1, 1, 0), (1, 0, 1))}
D_FREE = {R12: 10, R23: 6, R34: 5}


def n_tx(rate, T):
    """Coded bits sent for T trellis steps."""
    ka, kb = KEEP[rate]
    P = len(ka)
    per = sum(ka) + sum(kb)
    r = T % P
    return (T // P) * per + sum(ka[:r]) + sum(kb[:r])


def geometry(rate, n_c):
    """(T, n_info, n_tx) of a row of n_c values: T the largest step count with n_tx(T) <= n_c.
    ValueError where mimo_fec_create returns MIMO_ERR_ARG (bad rate, T < 7, n_c > 32768)."""
    if rate not in KEEP:
        raise ValueError("rate")
    if n_c > MAX_NC:
        raise ValueError("n_c > %d" % MAX_NC)
    T = 0
    while n_tx(rate, T + 1) <= n_c:      # n_tx grows with every step
        T += 1
    if T < TAIL + 1:
        raise ValueError("row too short: T = %d < 7" % T)
    return T, T - TAIL, n_tx(rate, T)


def coded_index(rate, T):
    """kA[T], kB[T]: the coded-bit index of A_t and of B_t in the sent order, -1 where
    punctured."""
    ka, kb = KEEP[rate]
    P = len(ka)
    t = np.arange(T)
    keepa = np.array(ka, bool)[t % P]
    keepb = np.array(kb, bool)[t % P]
    both = np.stack([keepa, keepb], 1).reshape(-1)
    k = np.cumsum(both) - 1
    k = np.where(both, k, -1).reshape(T, 2)
    return k[:, 0].astype(np.int64), k[:, 1].astype(np.int64)


def positions(rate, n_c, perm=None):
    """posA[T], posB[T]: the row position of A_t and B_t (through perm), -1 where punctured.
    ValueError for a perm whose entries are not distinct values below n_c."""
    T, _, ntx = geometry(rate, n_c)
    kA, kB = coded_index(rate, T)
    if perm is None:
        return kA, kB
    perm = np.asarray(perm).astype(np.int64)
    if perm.shape != (ntx,) or np.any(perm < 0) or np.any(perm >= n_c) or \
            len(np.unique(perm)) != ntx:
        raise ValueError("perm")
    return (np.where(kA >= 0, perm[np.maximum(kA, 0)], -1),
            np.where(kB >= 0, perm[np.maximum(kB, 0)], -1))


def encode(rate, n_c, info, perm=None):
    """info [..., n_info] of 0/1 -> rows [..., n_c] of 0/1 at row positions (after perm),
    unreferenced positions 0."""
    T, n_info, _ = geometry(rate, n_c)
    info = np.asarray(info).astype(np.uint8)
    assert info.shape[-1] == n_info
    lead = info.shape[:-1]
    z = np.zeros(lead + (TAIL,), np.uint8)
    u = np.concatenate([z, info, z], -1)                 # u[..., t + 6] = u_t
    at = lambda d: u[..., TAIL - d:TAIL - d + T]         # u_(t-d)
    A = at(0) ^ at(2) ^ at(3) ^ at(5) ^ at(6)
    B = at(0) ^ at(1) ^ at(2) ^ at(3) ^ at(6)
    pA, pB = positions(rate, n_c, perm)
    row = np.zeros(lead + (n_c,), np.uint8)
    row[..., pA[pA >= 0]] = A[..., pA >= 0]
    row[..., pB[pB >= 0]] = B[..., pB >= 0]
    return row


def depuncture(rate, n_c, llr, perm=None):
    """llr [..., n_c] int8 -> (L_A, L_B) [..., T] int64, 0 where punctured."""
    llr = np.asarray(llr)
    assert llr.dtype == np.int8 and llr.shape[-1] == n_c
    pA, pB = positions(rate, n_c, perm)
    v = llr.astype(np.int64)
    LA = np.where(pA >= 0, v[..., np.maximum(pA, 0)], 0)
    LB = np.where(pB >= 0, v[..., np.maximum(pB, 0)], 0)
    return LA, LB


def _trellis():
    s = np.arange(N_STATES)
    u = s & 1
    out = []
    for p in (s >> 1, (s >> 1) | 32):
        b = lambda k: (p >> k) & 1                       # bit k of p is u_(t-1-k)
        a_ = u ^ b(1) ^ b(2) ^ b(4) ^ b(5)
        b_ = u ^ b(0) ^ b(1) ^ b(2) ^ b(5)
        out.append((p, 1 - 2 * a_.astype(np.int64), 1 - 2 * b_.astype(np.int64)))
    return out


def viterbi(LA, LB):
    """(L_A, L_B) [rows][T] integers -> (bits [rows][T - 6] uint8, metric [rows] int64): the
    decoder of the module docstring in int64, vectorised over rows and states."""
    LA = np.asarray(LA).astype(np.int64)
    LB = np.asarray(LB).astype(np.int64)
    rows, T = LA.shape
    (p0, sa0, sb0), (p1, sa1, sb1) = _trellis()
    m = np.full((rows, N_STATES), M_INIT, np.int64)
    m[:, 0] = 0
    dec = np.empty((T, rows, N_STATES), bool)
    for t in range(T):
        la, lb = LA[:, t, None], LB[:, t, None]
        m0 = m[:, p0] + (sa0 * la + sb0 * lb)
        m1 = m[:, p1] + (sa1 * la + sb1 * lb)
        d = m1 > m0                                      # a tie keeps p0
        dec[t] = d
        m = np.where(d, m1, m0)
    bits = np.empty((rows, T), np.uint8)
    s = np.zeros(rows, np.int64)
    ar = np.arange(rows)
    for t in range(T - 1, -1, -1):
        bits[:, t] = s & 1
        s = (s >> 1) | (dec[t, ar, s].astype(np.int64) << 5)
    assert np.all(s == 0) and not bits[:, T - TAIL:].any()
    return bits[:, :T - TAIL], m[:, 0].copy()


def min_pitch(n_info):
    """The smallest bits_pitch: ceil(n_info / 8) rounded up to a multiple of 4."""
    return ((n_info + 7) // 8 + 3) // 4 * 4


def pack_bits(bits, pitch=None):
    """bits [rows][n_info] of 0/1 -> [rows][pitch] uint8, MSB first, zero padded."""
    rows, n = bits.shape
    pitch = min_pitch(n) if pitch is None else pitch
    out = np.zeros((rows, pitch), np.uint8)
    out[:, :(n + 7) // 8] = np.packbits(bits.astype(np.uint8), axis=1, bitorder="big")
    return out


def unpack_bits(packed, n_info):
    """[rows][pitch] uint8 in the d_bits format -> bits [rows][n_info] of 0/1; whatever the
    rows hold past bit n_info is dropped."""
    packed = np.ascontiguousarray(packed, np.uint8)
    return np.unpackbits(packed, axis=1, bitorder="big")[:, :n_info]


def decode(rate, n_c, llr, perm=None, bits_pitch=None):
    """llr [rows][n_c] int8 -> (packed bits [rows][bits_pitch] uint8, metric [rows] int32):
    what mimo_fec_decode writes."""
    bits, metric = viterbi(*depuncture(rate, n_c, llr, perm))
    return pack_bits(bits, bits_pitch), metric.astype(np.int32)


def _i32(x):
    assert x.min() >= -(1 << 31) and x.max() < (1 << 31)
    return x


def siso(LA, LB):
    """(L_A, L_B) [rows][T] integers -> (Lu, LAo, LBo [rows][T] int64, metric [rows] int64): the
    unclamped max-log-MAP Lambda of u_t, A_t and B_t of the module docstring and alpha_T(0), in
    int64 with every intermediate asserted to lie in int32; vectorised over rows and states."""
    LA = np.asarray(LA).astype(np.int64)
    LB = np.asarray(LB).astype(np.int64)
    rows, T = LA.shape
    (p0, sa0, sb0), (p1, sa1, sb1) = _trellis()          # the two transitions into state s
    s = np.arange(N_STATES)
    low = np.int64(-(1 << 62))                           # "no such transition" in a masked max
    # per bit x and value v: which of the 2 * 64 transitions (into s from p0, into s from p1)
    sel = {"u": [np.concatenate([s & 1, s & 1]) == v for v in (0, 1)],
           "a": [np.concatenate([sa0, sa1]) == 1 - 2 * v for v in (0, 1)],
           "b": [np.concatenate([sb0, sb1]) == 1 - 2 * v for v in (0, 1)]}
    al = np.empty((T + 1, rows, N_STATES), np.int64)
    al[0] = NEG_SISO
    al[0][:, 0] = 0
    for t in range(T):
        la, lb = LA[:, t, None], LB[:, t, None]
        al[t + 1] = _i32(np.maximum(al[t][:, p0] + (sa0 * la + sb0 * lb),
                                    al[t][:, p1] + (sa1 * la + sb1 * lb)))
    be = np.full((rows, N_STATES), NEG_SISO, np.int64)
    be[:, 0] = 0
    out = {k: np.empty((rows, T), np.int64) for k in sel}
    for t in range(T - 1, -1, -1):
        la, lb = LA[:, t, None], LB[:, t, None]
        c0 = (sa0 * la + sb0 * lb) + be                  # g + beta_(t+1)(s), from p0 and from p1
        c1 = (sa1 * la + sb1 * lb) + be
        e = _i32(np.concatenate([al[t][:, p0] + c0, al[t][:, p1] + c1], 1))
        for k, (m0, m1) in sel.items():
            out[k][:, t] = _i32(np.where(m0, e, low).max(1) - np.where(m1, e, low).max(1))
        # state p < 32 is p0 of s = 2p and 2p + 1, state p >= 32 is their p1
        be = _i32(np.concatenate([np.maximum(c0[:, 0::2], c0[:, 1::2]),
                                  np.maximum(c1[:, 0::2], c1[:, 1::2])], 1))
    return out["u"], out["a"], out["b"], al[T][:, 0].copy()


def decode_siso(rate, n_c, llr, perm=None, mode=SISO_APP, bits_pitch=None, info_pitch=None,
                fill=0):
    """llr [rows][n_c] int8 -> (out [rows][n_c] int8, packed bits [rows][bits_pitch] uint8,
    info LLRs [rows][info_pitch] int8, metric [rows] int32): what mimo_fec_siso writes. `fill` is
    what d_out held before the call: positions no kept coded bit refers to keep it."""
    assert mode in (SISO_APP, SISO_EXT)
    T, n_info, _ = geometry(rate, n_c)
    LA, LB = depuncture(rate, n_c, llr, perm)
    Lu, LAo, LBo, metric = siso(LA, LB)
    if mode == SISO_EXT:
        LAo, LBo = _i32(LAo - LA), _i32(LBo - LB)
    pA, pB = positions(rate, n_c, perm)
    out = np.full(np.asarray(llr).shape, fill, np.int8)
    out[:, pA[pA >= 0]] = np.clip(LAo[:, pA >= 0], -127, 127)
    out[:, pB[pB >= 0]] = np.clip(LBo[:, pB >= 0], -127, 127)
    info_pitch = min_info_pitch(n_info) if info_pitch is None else info_pitch
    info = np.zeros((LA.shape[0], info_pitch), np.int8)
    info[:, :n_info] = np.clip(Lu[:, :n_info], -127, 127)
    bits = pack_bits((Lu[:, :n_info] < 0).astype(np.uint8), bits_pitch)
    return out, bits, info, metric.astype(np.int32)


def min_info_pitch(n_info):
    """The smallest info_pitch: n_info rounded up to a multiple of 4."""
    return (n_info + 3) // 4 * 4


def qam_indices(row, n_bits):
    """Coded rows [..., n_c] of 0/1 -> QAM indices [..., n_c / n_bits]: value i of a symbol is
    bit i of its index counted from the most significant bit (the soft passes' LLR order)."""
    row = np.asarray(row).astype(np.uint32)
    g = row.reshape(row.shape[:-1] + (row.shape[-1] // n_bits, n_bits))
    w = 1 << np.arange(n_bits - 1, -1, -1, dtype=np.uint32)
    return (g * w).sum(-1).astype(np.uint8)


def rows_to_idx(row, b):
    """Coded rows [..., n_c] of 0/1 -> QAM indices [..., n_c / (2 b)] uint8, b bits per dimension:
    idx[j] = sum over i < 2b of row[2b j + i] << (2b - 1 - i), what MIMO_FEC_ENC_QAM writes. Row
    position i of carrier j is bit 2b - 1 - i of the index (gray(mI) << b) | gray(mQ): values
    0..b-1 are Re, MSB first, then Im, the order of a carrier's 2b LLRs."""
    if b not in (1, 2, 3, 4) or np.shape(row)[-1] % (2 * b):
        raise ValueError("b must be 1..4 and n_c a multiple of 2 b")
    return qam_indices(row, 2 * b)


def idx_to_rows(idx, b):
    """QAM indices [..., n] -> coded rows [..., n 2b] of 0/1: the inverse of rows_to_idx (bits of
    the index above 2b are dropped)."""
    if b not in (1, 2, 3, 4):
        raise ValueError("b must be 1..4")
    idx = np.asarray(idx).astype(np.uint32)
    sh = np.arange(2 * b - 1, -1, -1, dtype=np.uint32)
    bits = (idx[..., None] >> sh) & 1
    return bits.reshape(idx.shape[:-1] + (idx.shape[-1] * 2 * b,)).astype(np.uint8)


def idx_to_points(idx, b):
    """QAM indices -> the constellation points qam_point gives them (complex128): the index is
    (gray(mI) << b) | gray(mQ) and level m is soft.qam_levels(4^b)[m]."""
    from . import soft
    idx = np.asarray(idx).astype(np.int64) & ((1 << (2 * b)) - 1)
    m = np.arange(1 << b)
    level_of_gray = np.empty(1 << b, np.int64)
    level_of_gray[m ^ (m >> 1)] = m
    lv = soft.qam_levels(1 << (2 * b))
    return lv[level_of_gray[idx >> b]] + 1j * lv[level_of_gray[idx & ((1 << b) - 1)]]


ENC_BITS, ENC_QAM = 0, 1


def encode_rows(rate, n_c, packed, perm=None, form=ENC_BITS, qam_bits=0):
    """packed [rows][pitch] uint8 info bits in the d_bits format -> what mimo_fec_encode_rows
    writes: [rows][n_c] 0/1 bytes (ENC_BITS) or [rows][n_c / (2 b)] QAM indices (ENC_QAM)."""
    _, n_info, _ = geometry(rate, n_c)
    row = encode(rate, n_c, unpack_bits(packed, n_info), perm)
    if form == ENC_BITS:
        if qam_bits:
            raise ValueError("qam_bits must be 0 with ENC_BITS")
        return row
    if form != ENC_QAM:
        raise ValueError("form")
    return rows_to_idx(row, qam_bits)


class Fec:
    """One code geometry (mimo_fec_create): rate R12 / R23 / R34, rows of n_c values, an
    optional permutation of n_tx distinct row positions. encode and geometry run on the host;
    decode, siso and encode_rows run on the GPU."""

    def __init__(self, rate, n_c, perm=None):
        self._h = None
        p = None if perm is None else np.ascontiguousarray(perm, np.uint16)
        cfg = _lib.FecConfig(rate, n_c, None if p is None else p.ctypes.data)
        h = C.c_void_p()
        _lib.check(_lib.lib().mimo_fec_create(C.byref(cfg), C.byref(h)), "mimo_fec_create")
        self._h = h
        self.rate, self.n_c = rate, n_c
        self.steps, self.n_info, self.n_tx = self.geometry()

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.lib().mimo_fec_destroy(self._h)
                self._h = None
        except Exception:       # (interpreter shutdown: the module globals may be gone)
            pass

    def geometry(self):
        t, i, n = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _lib.check(_lib.lib().mimo_fec_geometry(self._h, C.byref(t), C.byref(i), C.byref(n)),
                   "mimo_fec_geometry")
        return t.value, i.value, n.value

    def encode(self, info):
        """info [n_info] of 0/1 -> row [n_c] of 0/1 (mimo_fec_encode, host)."""
        info = np.ascontiguousarray(info, np.uint8)
        assert info.shape == (self.n_info,)
        row = np.empty(self.n_c, np.uint8)
        _lib.check(_lib.lib().mimo_fec_encode(self._h, info.ctypes.data, row.ctypes.data),
                   "mimo_fec_encode")
        return row

    def min_pitch(self):
        return min_pitch(self.n_info)

    def decode(self, llr, n_rows, bits, bits_pitch=None, metric=None, stream=None):
        """Decode n_rows rows of n_c int8 LLRs on the device (mimo_fec_decode): bits receives
        [n_rows][bits_pitch] uint8, metric (optional) [n_rows] int32. llr, bits and metric are
        torch tensors, DeviceBuffers or addresses. Asynchronous on `stream`."""
        from .receiver import _ptr
        a = _lib.FecDecodeArgs(_ptr(llr), _ptr(bits), _ptr(metric), n_rows,
                               self.min_pitch() if bits_pitch is None else bits_pitch)
        _lib.check(_lib.lib().mimo_fec_decode(self._h, C.byref(a), stream), "mimo_fec_decode")

    def encode_rows(self, info, n_rows, out, form=ENC_BITS, qam_bits=0, bits_pitch=None,
                    stream=None):
        """Encode n_rows rows of packed info bits on the device (mimo_fec_encode_rows): info
        [n_rows][bits_pitch] uint8 in the d_bits format; out receives [n_rows][n_c] 0/1 bytes
        (ENC_BITS) or [n_rows][n_c / (2 qam_bits)] QAM indices (ENC_QAM). Tensors, DeviceBuffers
        or addresses. Asynchronous on `stream`."""
        from .receiver import _ptr
        a = _lib.FecEncodeArgs(_ptr(info), _ptr(out), n_rows,
                               self.min_pitch() if bits_pitch is None else bits_pitch, form,
                               qam_bits)
        _lib.check(_lib.lib().mimo_fec_encode_rows(self._h, C.byref(a), stream),
                   "mimo_fec_encode_rows")

    def min_info_pitch(self):
        return min_info_pitch(self.n_info)

    def siso(self, llr, n_rows, out=None, bits=None, info_llr=None, metric=None, mode=SISO_APP,
             bits_pitch=None, info_pitch=None, stream=None):
        """Max-log-MAP decode of n_rows rows of n_c int8 LLRs on the device (mimo_fec_siso): out
        (optional) receives the APP or extrinsic int8 LLRs of the kept coded bits at their row
        positions, bits (optional) [n_rows][bits_pitch] uint8, info_llr (optional)
        [n_rows][info_pitch] int8, metric (optional) [n_rows] int32. At least one of out, bits and
        info_llr. Tensors, DeviceBuffers or addresses. Asynchronous on `stream`."""
        from .receiver import _ptr
        a = _lib.FecSisoArgs(_ptr(llr), _ptr(out), _ptr(bits), _ptr(info_llr), _ptr(metric),
                             n_rows, self.min_pitch() if bits_pitch is None else bits_pitch,
                             self.min_info_pitch() if info_pitch is None else info_pitch, mode)
        _lib.check(_lib.lib().mimo_fec_siso(self._h, C.byref(a), stream), "mimo_fec_siso")

    @staticmethod
    def qam_indices(row, n_bits):
        return qam_indices(row, n_bits)
