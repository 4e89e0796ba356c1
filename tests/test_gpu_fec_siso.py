"""GPU tests of the soft-output (max-log-MAP) decoder (mimo_fec_siso; fec_siso_kernel in
fec_siso_kernels.hip) against the written definition in rub_mimo_amd/fec.py (decode_siso).
Integer arithmetic throughout: d_out (with the sentinels at the positions the call must not
write), bits, info LLRs, metric, padding and guard bytes are compared bitwise, there are no
tolerances.

Geometries around the 64-step chunk edge (T = 63, 64, 65, 32, 96), rows so short that a
hypothesis has no path (T = 7) or that alpha and beta are both still NEG-based (T = 11, and
T = 12 beside it), a row with an unused position, every T mod 3 of the rate-3/4 pattern, a C3 row
(T = 6144), the largest row (T = 24576), one row alone, and more rows than the persistent grid
has waves. Inputs per row, cycling: uniform int8 over the full range, uniform in [-8, 8] (so
that unsaturated values are compared), int8 with half the values 0 (many ties), an encoded row at
magnitude 20 with a few hard errors, all -128, all +127, all 0. Identity, random and sparse
permutations on the small geometries. Then the decoder behind mimo_rx_soft_demap on the
three-frame capture of postpass_support.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from postpass_support import N_FRAMES, NOISE_FRAME, _n_out, _sctype, _synth_capture
from rub_mimo_amd import _lib, fec, soft
from rub_mimo_amd.receiver import Receiver, RxParams

pytestmark = pytest.mark.gpu

GUARD = 64
N_FLIP = {fec.R12: 4, fec.R23: 2, fec.R34: 2}
N_KINDS = 7
S_OUT, S_BITS, S_INFO, S_METRIC = 0x5C, 0xA5, 0xC3, 0x5A      # what the outputs hold before a call

# rate, n_c, rows, all three perms
GEOMS = {
    "r12_T63": (fec.R12, 126, 5, True),
    "r12_T64_37rows": (fec.R12, 128, 37, True),
    "r12_T65": (fec.R12, 130, 5, True),
    "r12_T32": (fec.R12, 64, 5, True),
    "r12_T96": (fec.R12, 192, 5, True),
    "r12_T7": (fec.R12, 14, 3, True),
    "r12_T11": (fec.R12, 22, 5, True),
    "r12_T12": (fec.R12, 24, 5, True),
    "r23_one_unused": (fec.R23, 100, 9, True),
    "r34_Tmod3_0": (fec.R34, 100, 9, True),
    "r34_Tmod3_1": (fec.R34, 98, 9, True),
    "r34_Tmod3_2": (fec.R34, 99, 9, True),
    "r12_c3_row": (fec.R12, 12288, 8, False),
    "r34_largest": (fec.R34, 32768, 2, False),
    "r12_one_row": (fec.R12, 128, 1, False),
    "r23_T20_9001rows": (fec.R23, 30, 9001, False),
}
PERMS = ["identity", "random", "sparse"]
CASES = [(n, k) for n, g in GEOMS.items() for k in (PERMS if g[3] else PERMS[:1])]
MODES = {"app": fec.SISO_APP, "ext": fec.SISO_EXT}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need an MI355X")


def _perm(kind, rng, n_c, ntx):
    if kind == "identity":
        return None
    if kind == "random":
        return rng.permutation(n_c)[:ntx].astype(np.uint16)
    return np.sort(rng.choice(n_c, ntx, replace=False)).astype(np.uint16)


def _inputs(rng, rate, n_c, rows, perm):
    """rows x n_c int8, the seven kinds cycling over the rows; the coded row of the encoded rows
    (None elsewhere)."""
    T, n_info, ntx = fec.geometry(rate, n_c)
    used = np.arange(ntx) if perm is None else perm.astype(np.int64)
    llr = np.empty((rows, n_c), np.int8)
    coded = [None] * rows
    for r in range(rows):
        k = r % N_KINDS
        if k == 0:
            llr[r] = rng.integers(-128, 128, n_c)
        elif k == 1:
            llr[r] = rng.integers(-8, 9, n_c)
        elif k == 2:
            v = rng.integers(-128, 128, n_c)
            llr[r] = np.where(rng.integers(0, 2, n_c) == 1, v, 0)
        elif k == 3:
            coded[r] = fec.encode(rate, n_c, rng.integers(0, 2, n_info).astype(np.uint8), perm)
            v = 20 * (1 - 2 * coded[r].astype(np.int64))
            at = used[rng.choice(ntx, N_FLIP[rate], replace=False)]
            v[at] = -v[at]
            llr[r] = v
        else:
            llr[r] = (-128, 127, 0)[k - 4]
    return llr, coded


class _Dev:
    """Device copies of the LLR rows and sentinel-filled outputs with guard bytes on both
    sides."""

    def __init__(self, llr, bits_pitch, info_pitch):
        self.rows, self.n_c = llr.shape
        self.bp, self.ip = bits_pitch, info_pitch
        self.llr = _lib.DeviceBuffer(llr.nbytes)
        self.llr.upload(llr)
        self.buf = {"out": (_lib.DeviceBuffer(2 * GUARD + llr.nbytes), S_OUT),
                    "bits": (_lib.DeviceBuffer(2 * GUARD + self.rows * bits_pitch), S_BITS),
                    "info": (_lib.DeviceBuffer(2 * GUARD + self.rows * info_pitch), S_INFO),
                    "metric": (_lib.DeviceBuffer(2 * GUARD + 4 * self.rows), S_METRIC)}
        self.fill()

    def fill(self):
        for b, s in self.buf.values():
            b.upload(np.full(b.nbytes, s, np.uint8))

    def _get(self, name):
        b, s = self.buf[name]
        v = b.download(np.uint8, b.nbytes)
        assert np.all(v[:GUARD] == s) and np.all(v[-GUARD:] == s), name
        return v[GUARD:-GUARD].copy()

    def results(self):
        _lib.check(_lib.lib().mimo_stream_sync(None), "sync")
        return (self._get("out").view(np.int8).reshape(self.rows, self.n_c),
                self._get("bits").reshape(self.rows, self.bp),
                self._get("info").view(np.int8).reshape(self.rows, self.ip),
                self._get("metric").view(np.int32))

    def siso(self, f, mode=fec.SISO_APP, without=(), rows=None):
        self.fill()
        p = {k: (None if k in without else b.addr + GUARD) for k, (b, _) in self.buf.items()}
        f.siso(self.llr, self.rows if rows is None else rows, p["out"], p["bits"], p["info"],
               p["metric"], mode, self.bp, self.ip)
        return self.results()

    def viterbi(self, f):
        self.fill()
        f.decode(self.llr, self.rows, self.buf["bits"][0].addr + GUARD, self.bp,
                 self.buf["metric"][0].addr + GUARD)
        _, bits, _, metric = self.results()
        return bits, metric


@functools.lru_cache(maxsize=None)
def _inputs_case(name, kind):
    """The case's handle arguments and inputs; computed once and shared (no test modifies
    them)."""
    rate, n_c, rows, _ = GEOMS[name]
    rng = np.random.default_rng(1000 * list(GEOMS).index(name) + PERMS.index(kind))
    T, n_info, ntx = fec.geometry(rate, n_c)
    perm = _perm(kind, rng, n_c, ntx)
    llr, coded = _inputs(rng, rate, n_c, rows, perm)
    return rate, n_c, rows, perm, llr, coded


@functools.lru_cache(maxsize=None)
def _model_case(name, kind, mode):
    """The model's outputs of the case with d_out pre-filled with the sentinel."""
    rate, n_c, rows, perm, llr, _ = _inputs_case(name, kind)
    return fec.decode_siso(rate, n_c, llr, perm, MODES[mode], fill=np.int8(S_OUT))


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name,kind", CASES)
def test_siso_is_bitwise_the_model(name, kind, mode):
    """d_out (sentinels at the unreferenced positions included), bits, info LLRs, their padding
    and the metric equal the model's; the guard bytes stay; a second identical call gives
    identical bytes. At least half of the coded values compared on the [-8, 8] rows are
    unsaturated (asserted on the model alone)."""
    rate, n_c, rows, perm, llr, coded = _inputs_case(name, kind)
    want = _model_case(name, kind, mode)
    T, n_info, ntx = fec.geometry(rate, n_c)
    used = np.arange(ntx) if perm is None else perm.astype(np.int64)
    small = np.arange(rows) % N_KINDS == 1
    if small.any():
        inside = np.abs(want[0][small][:, used].astype(np.int64)) < 127
        assert 2 * inside.sum() >= inside.size, (inside.sum(), inside.size)
    unused = np.setdiff1d(np.arange(n_c), used)
    assert np.all(want[0][:, unused] == np.int8(S_OUT))
    f = fec.Fec(rate, n_c, perm)
    d = _Dev(llr, f.min_pitch(), f.min_info_pitch())
    got = d.siso(f, MODES[mode])
    for g, w, what in zip(got, want, ("d_out", "d_bits", "d_info_llr", "d_metric")):
        assert np.array_equal(g, w), what
    assert _same(d.siso(f, MODES[mode]), got)
    if mode == "app":
        for r, c in enumerate(coded):
            # few errors: the APP hard decision is the sent codeword at every used position
            if c is not None and T >= 12:
                assert np.array_equal(got[0][r, used] < 0, c[used] == 1)


@pytest.mark.parametrize("name,kind", [c for c in CASES if GEOMS[c[0]][2] < 100])
def test_optional_outputs_pitches_and_viterbi_on_the_same_handle(name, kind):
    """Each optional output NULL in turn: its buffer keeps the sentinel and the others are the
    model's; larger pitches only add zero bytes; mimo_fec_decode on the same handle before and
    after is bitwise its model, its metric is d_metric and its bits are d_bits in every row whose
    info LLRs have no 0."""
    rate, n_c, rows, perm, llr, _ = _inputs_case(name, kind)
    want = _model_case(name, kind, "app")
    T, n_info, ntx = fec.geometry(rate, n_c)
    f = fec.Fec(rate, n_c, perm)
    d = _Dev(llr, f.min_pitch(), f.min_info_pitch())
    vit = fec.decode(rate, n_c, llr, perm)
    assert _same(d.viterbi(f), vit)
    sent = (S_OUT, S_BITS, S_INFO, S_METRIC)
    for i, off in enumerate(("out", "bits", "info", "metric")):
        got = d.siso(f, without=(off,))
        for j, (g, w) in enumerate(zip(got, want)):
            if i == j:
                assert np.all(g.view(np.uint8) == sent[j]), off
            else:
                assert np.array_equal(g, w), (off, j)
    got = d.siso(f, without=("bits", "info"))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[3])
    got_v = d.viterbi(f)
    assert _same(got_v, vit)
    assert np.array_equal(got_v[1], want[3])
    sure = np.all(want[2][:, :n_info] != 0, axis=1)
    assert np.array_equal(got_v[0][sure], want[1][sure])
    wide = _Dev(llr, f.min_pitch() + 12, f.min_info_pitch() + 68)
    assert _same(wide.siso(f), fec.decode_siso(rate, n_c, llr, perm, fec.SISO_APP,
                                               f.min_pitch() + 12, f.min_info_pitch() + 68,
                                               fill=np.int8(S_OUT)))


def test_viterbi_cross_check_has_rows_of_both_kinds():
    """The cross-check above compares bits on some rows and leaves rows with ties out (a
    condition on the inputs, met by the model alone)."""
    want = _model_case("r12_T64_37rows", "identity", "app")
    sure = np.all(want[2][:, :58] != 0, axis=1)
    assert sure.sum() >= 10 and (~sure).sum() >= 5


def test_more_rows_after_fewer_on_one_handle():
    """The workspace is sized by the grid at the first call: a later call with more rows (and
    then one with fewer again) gives the model's bytes."""
    rate, n_c = fec.R34, 260
    rng = np.random.default_rng(3)
    llr, _ = _inputs(rng, rate, n_c, 50, None)
    want = fec.decode_siso(rate, n_c, llr, fill=np.int8(S_OUT))
    f = fec.Fec(rate, n_c)
    for rows in (2, 50, 7):
        d = _Dev(llr[:rows], f.min_pitch(), f.min_info_pitch())
        assert _same(d.siso(f), [w[:rows] for w in want]), rows
    d = _Dev(llr, f.min_pitch(), f.min_info_pitch())
    got = d.siso(f, rows=3)                             # fewer rows than the buffers hold
    for g, w, s in zip(got, want, (S_OUT, S_BITS, S_INFO, S_METRIC)):
        assert np.array_equal(g[:3], w[:3]) and np.all(g[3:].view(np.uint8) == s)


def _rc(f, llr, out, bits, info, metric, n_rows, bp, ip, mode=0):
    a = _lib.FecSisoArgs(llr, out, bits, info, metric, n_rows, bp, ip, mode)
    return _lib.lib().mimo_fec_siso(f._h, C.byref(a), None)


def test_argument_errors():
    f = fec.Fec(fec.R12, 128)                  # n_info 58: bits_pitch >= 8, info_pitch >= 60
    llr = _lib.DeviceBuffer(8 * 128 + 16)
    llr.zero()
    out = _lib.DeviceBuffer(4 * 128 + 16)
    bits = _lib.DeviceBuffer(4 * 16 + 16)
    info = _lib.DeviceBuffer(4 * 64 + 16)
    met = _lib.DeviceBuffer(4 * 4 + 16)
    l, o, b, i, m = llr.addr, out.addr, bits.addr, info.addr, met.addr
    assert _rc(f, l, o, b, i, m, 4, 8, 60) == 0
    assert _rc(f, l, o, b, i, m, 4, 8, 60, 1) == 0
    assert _rc(f, l, o, b, i, None, 4, 16, 64) == 0
    assert _rc(f, l, o, None, None, None, 4, 0, 0) == 0          # pitches of absent outputs
    assert _rc(f, l, None, b, None, m, 4, 8, 0) == 0
    assert _rc(f, l, None, None, i, m, 4, 0, 60) == 0
    assert _rc(f, l, None, None, None, m, 4, 8, 60) == -1        # nothing to write
    assert b"null" in _lib.lib().mimo_last_error()
    assert _rc(f, None, o, b, i, m, 4, 8, 60) == -1
    assert _rc(f, l, o, b, i, m, 4, 8, 60, 2) == -1              # no such mode
    assert _rc(f, l, l, b, i, m, 4, 8, 60) == -1                 # d_out is d_llr
    assert b"overlap" in _lib.lib().mimo_last_error()
    assert _rc(f, l, l + 4 * 128 - 16, b, i, m, 4, 8, 60) == -1  # d_out starts in d_llr's last row
    assert _rc(f, l + 256, l, b, i, m, 4, 8, 60) == -1           # d_out ends in d_llr
    assert _rc(f, l, l + 4 * 128, b, i, m, 4, 8, 60) == 0        # adjacent is allowed
    assert _rc(f, l + 8, o, b, i, m, 4, 8, 60) == -1             # misaligned d_llr
    assert _rc(f, l, o + 8, b, i, m, 4, 8, 60) == -1             # misaligned d_out
    assert _rc(f, l, o, b + 4, i, m, 4, 8, 60) == -1             # misaligned d_bits
    assert _rc(f, l, o, b, i + 4, m, 4, 8, 60) == -1             # misaligned d_info_llr
    assert _rc(f, l, o, b, i, m + 2, 4, 8, 60) == -1             # misaligned d_metric
    assert _rc(f, l, o, b, i, m, 0, 8, 60) == -1                 # no rows
    assert _rc(f, l, o, b, i, m, 4, 4, 60) == -1                 # pitch below ceil(n_info / 8)
    assert _rc(f, l, o, b, i, m, 4, 10, 60) == -1                # pitch no multiple of 4
    assert b"bits_pitch" in _lib.lib().mimo_last_error()
    assert _rc(f, l, o, b, i, m, 4, 8, 56) == -1                 # info_pitch below n_info
    assert _rc(f, l, o, b, i, m, 4, 8, 62) == -1                 # info_pitch no multiple of 4
    assert b"info_pitch" in _lib.lib().mimo_last_error()
    assert _lib.lib().mimo_fec_siso(f._h, None, None) == -1
    a = _lib.FecSisoArgs(l, o, b, i, m, 4, 8, 60, 0)
    assert _lib.lib().mimo_fec_siso(None, C.byref(a), None) == -1
    _lib.check(_lib.lib().mimo_stream_sync(None), "sync")


# ---- end to end: the decoder behind mimo_rx_soft_demap on the three-frame capture ----
# 2x2 ZF 16-QAM, rate 1/2, seed 81, int8 at llr_scale 4 (test_gpu_fec.py's qam16_zf_2x2 case)
@functools.lru_cache(maxsize=None)
def _e2e():
    M, cp, N, nac, pid, qam, det, seed, rate = 256, 32, 2, 4, 10, 16, _lib.DET_ZF, 81, fec.R12
    p = _sctype(M, "all")
    F, mo = N_FRAMES, pid
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=det, keep_identity_bias=False, qam_order=qam, p=p))
    mocc = rx.M_occ
    nsym = F * N * mo * mocc
    nb = 2 * soft.qam_bits(qam)
    n_c, rows = mocc * nb, F * N * mo
    tx = _lib.DeviceBuffer(nsym)
    iq, L = _synth_capture(M, cp, N, nac, pid, qam, p, seed=seed, tx=tx)
    osym, oidx = _lib.DeviceBuffer(nsym * 8), _lib.DeviceBuffer(nsym)
    rx.process(iq, L, L, F, max_out=mo, out_sym=osym, out_idx=oidx)
    res = rx.results()
    written = np.zeros((F, N, mo), bool)
    for fr, r in enumerate(res):
        written[fr, :, :_n_out(r, mo)] = True
    written = written.reshape(rows)
    sent = tx.download(np.uint8, nsym).reshape(rows, mocc)
    x = ((sent[..., None] >> np.arange(nb - 1, -1, -1)) & 1).astype(np.uint8).reshape(rows, n_c)
    f = fec.Fec(rate, n_c)
    T, n_info, ntx = f.geometry()
    rng = np.random.default_rng(seed)
    info = rng.integers(0, 2, (rows, n_info)).astype(np.uint8)
    c = fec.encode(rate, n_c, info)
    llr = _lib.DeviceBuffer(nsym * nb)
    rx.soft_demap(osym, llr, max_out=mo, fmt=_lib.LLR_I8, llr_scale=4.0)
    rx.results()                                        # (synchronises)
    raw = llr.download(np.int8, nsym * nb).reshape(rows, n_c)
    assert not np.any(raw == -128)                      # so the negation is exact
    v = np.where((x ^ c) == 1, -raw, raw).astype(np.int8)
    d = _Dev(v, f.min_pitch(), f.min_info_pitch())
    got = d.siso(f)
    want = fec.decode_siso(rate, n_c, v, fill=np.int8(S_OUT))
    return dict(res=res, written=written, c=c, v=v, got=got, want=want, rate=rate, ntx=ntx,
                T=T, rows_f=N * mo)


def test_end_to_end_behind_soft_demap():
    """The result is bitwise the model's on the same LLR bytes. The noise frame's rows give
    all-zero outputs and metric 0. Every written row whose LLR signs agree with the codeword at
    all used positions and which has fewer than d_free zero LLRs there (test_gpu_fec.py's
    criterion: that codeword is then the unique maximum) has APP signs equal to the codeword at
    every used position where the APP is non-zero; such rows exist."""
    e = _e2e()
    assert e["res"][NOISE_FRAME]["status"] != _lib.FRAME_OK
    assert sum(r["status"] == _lib.FRAME_OK for r in e["res"]) == N_FRAMES - 1
    for g, w, what in zip(e["got"], e["want"], ("d_out", "d_bits", "d_info_llr", "d_metric")):
        assert np.array_equal(g, w), what
    ntx, w = e["ntx"], e["written"]
    out, bits, illr, metric = e["got"]
    assert e["T"] >= 12
    noise = slice(NOISE_FRAME * e["rows_f"], (NOISE_FRAME + 1) * e["rows_f"])
    assert not w[noise].any() and not e["v"][noise].any()
    for o in (out[noise, :ntx], bits[noise], illr[noise], metric[noise]):
        assert not o.any()
    v, c = e["v"][:, :ntx].astype(np.int64), e["c"][:, :ntx]
    clean = w & np.all((v == 0) | ((v < 0) == (c == 1)), axis=1) & \
        ((v == 0).sum(axis=1) < fec.D_FREE[e["rate"]])
    assert clean.sum() > 0
    app = out[clean][:, :ntx].astype(np.int64)
    assert np.all((app == 0) | ((app < 0) == (c[clean] == 1)))
