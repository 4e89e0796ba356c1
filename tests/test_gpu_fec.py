"""GPU tests of the K = 7 Viterbi decoder (mimo_fec_decode; fec_viterbi_kernel in
fec_kernels.hip) against the written definition in rub_mimo_amd/fec.py. Integer arithmetic
throughout: bits, padding and metric are compared bitwise, there are no tolerances.

Geometries around the 64-step chunk edge (T = 63, 64, 65), the smallest row (T = 7), every
T mod 3 of the rate-3/4 pattern, a row with an unused position, a C3 row (T = 6144), the largest
row (T = 24576), one row alone, and more rows than the persistent grid has waves. Inputs per
row, cycling: uniform int8 over the full range, int8 with half the values 0 (ties at most steps),
an encoded row at magnitude 20 with hard errors below half the free distance, all -128, all +127,
all 0. Identity, random and sparse permutations. Then the decoder behind mimo_rx_soft_demap and
mimo_rx_sic_soft_fb on the three-frame capture of postpass_support.py."""
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

# rate, n_c, rows
GEOMS = {
    "r12_T63": (fec.R12, 126, 5),
    "r12_T64_37rows": (fec.R12, 128, 37),
    "r12_T65": (fec.R12, 130, 5),
    "r12_T7": (fec.R12, 14, 3),
    "r23_one_unused": (fec.R23, 100, 9),
    "r34_Tmod3_0": (fec.R34, 100, 9),
    "r34_Tmod3_1": (fec.R34, 98, 9),
    "r34_Tmod3_2": (fec.R34, 99, 9),
    "r12_T32": (fec.R12, 64, 5),
    "r12_T96": (fec.R12, 192, 5),
    "r12_c3_row": (fec.R12, 12288, 8),
    "r34_largest": (fec.R34, 32768, 4),
    "r12_one_row": (fec.R12, 128, 1),
    "r23_T20_9001rows": (fec.R23, 30, 9001),
}
PERMS = ["identity", "random", "sparse"]


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
    """rows x n_c int8, the six kinds cycling over the rows; the info bits of the encoded
    rows (None elsewhere)."""
    T, n_info, ntx = fec.geometry(rate, n_c)
    used = np.arange(ntx) if perm is None else perm.astype(np.int64)
    llr = np.empty((rows, n_c), np.int8)
    info = [None] * rows
    for r in range(rows):
        k = r % 6
        if k == 0:
            llr[r] = rng.integers(-128, 128, n_c)
        elif k == 1:
            v = rng.integers(-128, 128, n_c)
            llr[r] = np.where(rng.integers(0, 2, n_c) == 1, v, 0)
        elif k == 2:
            info[r] = rng.integers(0, 2, n_info).astype(np.uint8)
            row = fec.encode(rate, n_c, info[r], perm)
            v = 20 * (1 - 2 * row.astype(np.int64))
            at = used[rng.choice(ntx, N_FLIP[rate], replace=False)]
            v[at] = -v[at]
            llr[r] = v
        else:
            llr[r] = (-128, 127, 0)[k - 3]
    return llr, info


class _Dev:
    """Device copies of the LLR rows and garbage-filled outputs with guard bytes on both
    sides."""

    def __init__(self, llr, pitch):
        self.rows, self.pitch = llr.shape[0], pitch
        self.llr = _lib.DeviceBuffer(llr.nbytes)
        self.llr.upload(llr)
        self.bits = _lib.DeviceBuffer(2 * GUARD + self.rows * pitch)
        self.metric = _lib.DeviceBuffer(2 * GUARD + 4 * self.rows)
        self.garbage()

    def garbage(self):
        self.bits.upload(np.full(self.bits.nbytes, 0xA5, np.uint8))
        self.metric.upload(np.full(self.metric.nbytes, 0x5A, np.uint8))

    def decode(self, f, with_metric=True, rows=None):
        f.decode(self.llr, self.rows if rows is None else rows, self.bits.addr + GUARD,
                 self.pitch, self.metric.addr + GUARD if with_metric else None)
        _lib.check(_lib.lib().mimo_stream_sync(None), "sync")
        b = self.bits.download(np.uint8, self.bits.nbytes)
        m = self.metric.download(np.uint8, self.metric.nbytes)
        assert np.all(b[:GUARD] == 0xA5) and np.all(b[-GUARD:] == 0xA5)
        assert np.all(m[:GUARD] == 0x5A) and np.all(m[-GUARD:] == 0x5A)
        return (b[GUARD:-GUARD].reshape(self.rows, self.pitch).copy(),
                m[GUARD:-GUARD].copy().view(np.int32))


@functools.lru_cache(maxsize=None)
def _model_case(name, kind):
    """The case's handle arguments, inputs and the model's outputs; computed once and shared
    (no test modifies them)."""
    rate, n_c, rows = GEOMS[name]
    rng = np.random.default_rng(1000 * list(GEOMS).index(name) + PERMS.index(kind))
    T, n_info, ntx = fec.geometry(rate, n_c)
    perm = _perm(kind, rng, n_c, ntx)
    llr, info = _inputs(rng, rate, n_c, rows, perm)
    bits, metric = fec.viterbi(*fec.depuncture(rate, n_c, llr, perm))
    for r, u in enumerate(info):
        if u is not None:                   # fewer errors than d_free / 2: the sent bits
            assert np.array_equal(bits[r], u)
            assert metric[r] == 20 * ntx - 2 * 20 * N_FLIP[rate]
    return rate, n_c, rows, perm, llr, bits, metric.astype(np.int32)


@pytest.mark.parametrize("kind", PERMS)
@pytest.mark.parametrize("name", list(GEOMS))
def test_decode_is_bitwise_the_model(name, kind):
    """Bits, padding and metric equal the model's; the guard bytes stay; a second identical
    call gives identical bytes; with d_metric NULL the bits are the same and the metric buffer
    keeps its garbage; a larger bits_pitch only adds zero bytes."""
    rate, n_c, rows, perm, llr, bits, metric = _model_case(name, kind)
    f = fec.Fec(rate, n_c, perm)
    assert f.geometry() == fec.geometry(rate, n_c)
    pitch = f.min_pitch()
    want = fec.pack_bits(bits, pitch)
    d = _Dev(llr, pitch)
    got_b, got_m = d.decode(f)
    assert np.array_equal(got_m, metric)
    assert np.array_equal(got_b, want)
    assert rows < 6 or len(np.unique(got_b)) > 2
    d.garbage()
    again_b, again_m = d.decode(f)
    assert np.array_equal(again_b, got_b) and np.array_equal(again_m, got_m)
    d.garbage()
    nm_b, nm_m = d.decode(f, with_metric=False)
    assert np.array_equal(nm_b, want) and np.all(nm_m.view(np.uint8) == 0x5A)
    wide = _Dev(llr, pitch + 12)
    wide_b, wide_m = wide.decode(f)
    assert np.array_equal(wide_b, fec.pack_bits(bits, pitch + 12))
    assert np.array_equal(wide_m, metric)


@pytest.mark.parametrize("rate,n_c", [(fec.R12, 131), (fec.R23, 100), (fec.R34, 101)])
def test_unused_positions_are_ignored(rate, n_c):
    """A table that leaves a position unused (n_tx < n_c): whatever that position holds, the
    output is the model's."""
    rng = np.random.default_rng(n_c)
    T, n_info, ntx = fec.geometry(rate, n_c)
    assert ntx < n_c
    perm = np.delete(np.arange(n_c), n_c // 2)[:ntx].astype(np.uint16)
    unused = np.setdiff1d(np.arange(n_c), perm)                  # mid-row, not merely its end
    assert len(unused) == n_c - ntx and unused[0] == n_c // 2
    llr, _ = _inputs(rng, rate, n_c, 6, perm)
    f = fec.Fec(rate, n_c, perm)
    outs = []
    for g in (-128, 0, 127, 55):
        llr[:, unused] = g
        d = _Dev(llr, f.min_pitch())
        outs.append(d.decode(f))
    bits, metric = fec.decode(rate, n_c, llr, perm)
    for b, m in outs:
        assert np.array_equal(b, bits) and np.array_equal(m, metric)


def test_more_rows_after_fewer_on_one_handle():
    """The workspace is sized by the grid at the first decode: a later call with more rows
    (and then one with fewer again) gives the model's bytes."""
    rate, n_c = fec.R34, 260
    rng = np.random.default_rng(3)
    llr, _ = _inputs(rng, rate, n_c, 50, None)
    bits, metric = fec.decode(rate, n_c, llr)
    f = fec.Fec(rate, n_c)
    for rows in (2, 50, 7):
        d = _Dev(llr[:rows], f.min_pitch())
        b, m = d.decode(f)
        assert np.array_equal(b, bits[:rows]) and np.array_equal(m, metric[:rows]), rows


def _rc(f, llr, bits, metric, n_rows, pitch):
    a = _lib.FecDecodeArgs(llr, bits, metric, n_rows, pitch)
    return _lib.lib().mimo_fec_decode(f._h, C.byref(a), None)


def test_argument_errors():
    f = fec.Fec(fec.R12, 128)                          # n_info 58: 8 bytes, pitch >= 8
    llr = _lib.DeviceBuffer(4 * 128 + 16)
    llr.zero()
    bits = _lib.DeviceBuffer(4 * 16 + 16)
    met = _lib.DeviceBuffer(4 * 4 + 16)
    l, b, m = llr.addr, bits.addr, met.addr
    assert _rc(f, l, b, m, 4, 8) == 0
    assert _rc(f, l, b, None, 4, 8) == 0
    assert _rc(f, l, b, m, 4, 16) == 0
    assert _rc(f, None, b, m, 4, 8) == -1
    assert _rc(f, l, None, m, 4, 8) == -1
    assert _rc(f, l + 8, b, m, 4, 8) == -1             # misaligned d_llr
    assert _rc(f, l, b + 4, m, 4, 8) == -1             # misaligned d_bits
    assert _rc(f, l, b, m + 2, 4, 8) == -1             # misaligned d_metric
    assert _rc(f, l, b, m, 0, 8) == -1                 # no rows
    assert _rc(f, l, b, m, 4, 4) == -1                 # pitch below ceil(n_info / 8)
    assert _rc(f, l, b, m, 4, 10) == -1                # pitch no multiple of 4
    assert b"bits_pitch" in _lib.lib().mimo_last_error()
    assert _lib.lib().mimo_fec_decode(f._h, None, None) == -1
    a = _lib.FecDecodeArgs(l, b, m, 4, 8)
    assert _lib.lib().mimo_fec_decode(None, C.byref(a), None) == -1
    _lib.check(_lib.lib().mimo_stream_sync(None), "sync")


# ---- end to end: the decoder behind the soft passes on the three-frame capture ----
# M, cp, N, nac, pid, qam, detector, sctype, synthesiser seed, code rate. The seeds were chosen on
# the CPU (oracle synth_frame + FrameSyncRef at 30 dB, soft.mse_reference / llr_reference and
# sic.sic_tables / sic_apply_soft in float64, int8 at llr_scale 4) so that the model alone meets
# the condition on the inputs below: clean rows of frames 0 and 2 were 30 / 40 for both passes
# (qam16_zf_2x2, seed 81) and 45 / 64 (soft_demap) and 64 / 64 (sic_soft_fb) (qam64_mmse_4x4,
# seed 8).
E2E = {
    "qam16_zf_2x2": (256, 32, 2, 4, 10, 16, _lib.DET_ZF, "all", 81, fec.R12),
    "qam64_mmse_4x4": (128, 32, 4, 8, 8, 64, _lib.DET_MMSE, None, 8, fec.R34),
}


@functools.lru_cache(maxsize=None)
def _e2e(name):
    """One batch of the case; per soft pass the int8 LLRs at llr_scale 4 with the signs flipped
    where transmitted bit ^ codeword bit is 1 (the code is linear: the decoder then sees the
    codeword of the chosen info bits through the same channel), the decoder's output on them
    and the model's on the same bytes."""
    M, cp, N, nac, pid, qam, det, sct, seed, rate = E2E[name]
    p = _sctype(M, sct)
    F, mo = N_FRAMES, pid
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=det, keep_identity_bias=False, qam_order=qam, p=p))
    mocc = rx.M_occ
    nsym = F * N * mo * mocc
    nb = 2 * soft.qam_bits(qam)
    n_c, rows = mocc * nb, F * N * mo
    tx = _lib.DeviceBuffer(nsym)
    iq, L = _synth_capture(M, cp, N, nac, pid, qam, p, seed=seed, tx=tx)
    osym, oidx, zidx = (_lib.DeviceBuffer(nsym * 8), _lib.DeviceBuffer(nsym),
                        _lib.DeviceBuffer(nsym))
    rx.process(iq, L, L, F, max_out=mo, out_sym=osym, out_idx=oidx)
    res = rx.results()
    written = np.zeros((F, N, mo), bool)
    for f, r in enumerate(res):
        written[f, :, :_n_out(r, mo)] = True
    written = written.reshape(rows)
    sent = tx.download(np.uint8, nsym).reshape(rows, mocc)
    x = ((sent[..., None] >> np.arange(nb - 1, -1, -1)) & 1).astype(np.uint8).reshape(rows, n_c)
    f = fec.Fec(rate, n_c)
    T, n_info, ntx = f.geometry()
    rng = np.random.default_rng(seed)
    info = rng.integers(0, 2, (rows, n_info)).astype(np.uint8)
    c = fec.encode(rate, n_c, info)
    llr = _lib.DeviceBuffer(nsym * nb)
    out = {}
    for pname in ("soft_demap", "sic_soft_fb"):
        if pname == "soft_demap":
            rx.soft_demap(osym, llr, max_out=mo, fmt=_lib.LLR_I8, llr_scale=4.0)
            idx = oidx
        else:
            rx.sic_soft_fb(osym, llr, None, zidx, max_out=mo, fmt=_lib.LLR_I8, llr_scale=4.0)
            idx = zidx
        rx.results()                                    # (synchronises)
        raw = llr.download(np.int8, nsym * nb).reshape(rows, n_c)
        assert not np.any(raw == -128)                  # so the negation is exact
        v = np.where((x ^ c) == 1, -raw, raw).astype(np.int8)
        hard = idx.download(np.uint8, nsym).reshape(rows, mocc)
        d = _Dev(v, f.min_pitch())
        bits, metric = d.decode(f)
        mb, mm = fec.viterbi(*fec.depuncture(rate, n_c, v))
        out[pname] = dict(v=v, bits=bits, metric=metric, model_bits=mb, model_metric=mm,
                          uncoded=int(np.unpackbits((hard ^ sent)[written]).sum()))
    return dict(res=res, written=written, info=info, c=c, out=out, rate=rate, ntx=ntx,
                n_info=n_info, mo=mo, N=N, pitch=f.min_pitch())


@pytest.mark.parametrize("pname", ["soft_demap", "sic_soft_fb"])
@pytest.mark.parametrize("name", list(E2E))
def test_end_to_end_behind_the_soft_passes(name, pname):
    """The decoder's output is bitwise the model's on the same LLR bytes. Every written row
    whose LLR signs agree with the codeword at all used positions and which has fewer than
    d_free zero LLRs there decodes to exactly the chosen info bits (that codeword is then the
    unique maximum); such rows are at least half of the written rows (a condition on the
    inputs, met by the CPU models alone, see E2E). Rows of the noise frame decode to zeros with
    metric 0. The coded and uncoded error counts are printed, not asserted."""
    e = _e2e(name)
    o = e["out"][pname]
    assert e["res"][NOISE_FRAME]["status"] != _lib.FRAME_OK
    assert sum(r["status"] == _lib.FRAME_OK for r in e["res"]) == N_FRAMES - 1
    assert np.array_equal(o["bits"], fec.pack_bits(o["model_bits"], e["pitch"]))
    assert np.array_equal(o["metric"], o["model_metric"].astype(np.int32))
    ntx, w = e["ntx"], e["written"]
    v, c = o["v"][:, :ntx].astype(np.int64), e["c"][:, :ntx]
    clean = w & np.all((v == 0) | ((v < 0) == (c == 1)), axis=1) & \
        ((v == 0).sum(axis=1) < fec.D_FREE[e["rate"]])
    dec = np.unpackbits(o["bits"], axis=1)[:, :e["n_info"]]
    assert np.array_equal(dec[clean], e["info"][clean])
    assert np.array_equal(o["metric"][clean], np.abs(v[clean]).sum(axis=1))
    assert 2 * clean.sum() >= w.sum() > 0, (clean.sum(), w.sum())
    rows_f = e["N"] * e["mo"]
    noise = slice(NOISE_FRAME * rows_f, (NOISE_FRAME + 1) * rows_f)
    assert not w[noise].any() and not o["bits"][noise].any() and not o["metric"][noise].any()
    assert not o["bits"][~w].any() and not o["metric"][~w].any()
    coded = int((dec[w] != e["info"][w]).sum())
    print("%s %s: %d of %d written rows clean; info-bit errors %d of %d coded, %d of %d uncoded"
          % (name, pname, clean.sum(), w.sum(), coded, w.sum() * e["n_info"], o["uncoded"],
             w.sum() * v.shape[1]))
