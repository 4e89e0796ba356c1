"""GPU tests of the decode and weight kernels element by element, per kernel family.

Every symbol-parity assertion elsewhere reduces a frame to one error-vector ratio, which a
large local error passes (one value off by half the 64-QAM spacing among 8 M, or one carrier
0.4 % wrong on every symbol). Here every kept (symbol, stream, carrier) of every decode kernel
family, at the smallest shape that reaches it, is compared with the float64 decode of
tests/decode_support.py in units of float32 rounding at that element (DEC_UNITS, set from the
C oracle's own error in tests/test_decode_model.py and never from a GPU kernel); the indices
with the hard decision of the delivered value and of the reference, each mismatch judged on its
own; the error counts and EVM sums with recounts; and the rows the decode must not write with a
sentinel. The weight kernels are compared per entry with a float64 solve on frequency-selective
channels (decode_support.select_fir), where the pivot order of the Gauss-Jordan changes from
carrier to carrier. No oracle runs here: the reference is numpy.

Kernel families (decode_kernels.hip decode_launch_na, decode_stream.hip stream_geometry_ok,
decode_split.hip decode_split_accepts); mimo_rx_get_decode_path tells the three launch paths
apart, the kernel within MIMO_DECODE_SYMBOL follows from the geometry:
  decode_stream_kernel      N 2 at M 1024/2048/4096, N 4 at M 1024/2048, every carrier occupied
  split decode              N 8 at M 512..4096, every carrier occupied, max_out >= M / 64
  decode_reg_kernel         N 2/4 at M 512..4096 wherever the two above refuse
  decode_persistent_kernel  M 256, every carrier occupied
  decode_kernel             everything else
"""
import numpy as np
import pytest

import decode_support as ds
from rub_mimo_amd import _lib
from rub_mimo_amd import framing as fr
from rub_mimo_amd.receiver import Receiver, RxParams, Synthesizer, SynthParams

pytestmark = pytest.mark.gpu

STREAM, SPLIT, SYMBOL = _lib.DECODE_STREAM, _lib.DECODE_SPLIT, _lib.DECODE_SYMBOL
ZF2, ZF, MMSE, SISO = _lib.DET_ZF2, _lib.DET_ZF, _lib.DET_MMSE, _lib.DET_SISO
GUARD = 4096                   # sentinel bytes before and after each output buffer
SYM_FILL, IDX_FILL = 0xFF, 0xA5
EVM_RTOL = 1e-5


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need an MI355X")


def _sctype(M, kind):
    if kind == "liquid":
        return fr.ofdmframe_init_liquid_sctype(M)
    return None


class _Guarded:
    """A device output buffer pre-filled with a sentinel byte, with a guard region of the same
    byte on either side."""

    def __init__(self, nbytes, fill):
        import torch
        self.n, self.fill = nbytes, fill
        self.t = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device="cuda")
        self.addr = self.t.data_ptr() + GUARD

    def host(self):
        h = self.t.cpu().numpy()
        assert np.all(h[:GUARD] == self.fill), "bytes written before the output buffer"
        assert np.all(h[GUARD + self.n:] == self.fill), "bytes written past the output buffer"
        return h[GUARD:GUARD + self.n]


def _qam_points(idx, qam):
    L, b, s = ds._qam(qam)
    out = []
    for g in (np.asarray(idx, np.int64) >> b, np.asarray(idx, np.int64) & (L - 1)):
        m = g.copy()
        for sh in (1, 2, 4):
            m ^= m >> sh
        out.append((2 * m - (L - 1)) / s)
    return out[0] + 1j * out[1]


NAC = 2                        # (the decode does not depend on the number of access codes)


def run_case(M, cp, N, pid, qam, det, seed, path, F=3, sct=None, ref_mode=2, outs="both",
             layout=_lib.LAYOUT_STREAM_MAJOR, sc16=False, noise_frame=None, siso=None, K=1,
             nac=NAC, max_out=None, base=None):
    """Synthesise F captures on the device (K > 1: each a stream of two back-to-back frames in
    K slots), decode them with sentinel-filled outputs and check every element. Returns what a
    dependent case (another output set of the same batch) compares with."""
    import torch
    p = _sctype(M, sct)
    sp = SynthParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid=pid,
                     qam_order=qam, seed=seed, snr_db=30.0, p=p)
    S = Synthesizer(sp)
    P = RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid, detector=det,
                 qam_order=qam, p=p, siso_tx=siso[0] if siso else 0,
                 siso_rx=siso[1] if siso else 0)
    rxo = Receiver(P)
    mocc = rxo.M_occ
    occ_p = rxo.p
    mo = pid if max_out is None else max_out
    slots = F * K
    tx = torch.zeros((slots, N, pid, mocc), dtype=torch.uint8, device="cuda")
    rs = None
    if K > 1:
        lens, L = S.stream_layout(F, 2)
        iq = torch.zeros((F, N, L), dtype=torch.complex64, device="cuda")
        starts, _ = S.generate_streams(iq, L, F, 2, K, tx_idx=tx)
        rs = torch.from_numpy(starts.view(np.int64).copy()).cuda()
        assert ref_mode == 1
    else:
        L = max(S.frame_len(i) for i in range(F))
        iq = torch.zeros((F, N, L), dtype=torch.complex64, device="cuda")
        S.generate(iq, L, L, F, tx_idx=tx)
    torch.cuda.synchronize()
    if noise_frame is not None:
        rng = np.random.default_rng(seed)
        nz = 0.01 * (rng.standard_normal((N, L)) + 1j * rng.standard_normal((N, L)))
        iq[noise_frame] = torch.from_numpy(nz.astype(np.complex64)).cuda()
    src, scale = iq, None
    if sc16:
        amax = float(torch.view_as_real(iq).abs().max()) * 1.01
        src = (torch.view_as_real(iq) * (32767.0 / amax)).round_().clamp_(-32768, 32767) \
            .to(torch.int16).contiguous()
        scale = amax / 32767.0
        host = (src.cpu().numpy().astype(np.float32) * np.float32(scale))
        host = host[..., 0] + 1j * host[..., 1]
    else:
        host = iq.cpu().numpy()
    txh = tx.cpu().numpy()                                         # [slot][N][pid][mocc]
    sym_major = layout == _lib.LAYOUT_SYMBOL_MAJOR
    refi = None
    if ref_mode == 1:
        refi = torch.from_numpy(np.ascontiguousarray(
            txh[:, :, :mo].transpose(0, 2, 1, 3) if sym_major else txh[:, :, :mo])).cuda()
    want_sym, want_idx = outs in ("both", "sym"), outs in ("both", "idx")
    osym = _Guarded(slots * N * mo * mocc * 8, SYM_FILL) if want_sym else None
    oidx = _Guarded(slots * N * mo * mocc, IDX_FILL) if want_idx else None
    rxo.process(src, L, L, F, max_out=mo, out_sym=osym.addr if osym else None,
                out_idx=oidx.addr if oidx else None, ref_mode=ref_mode, ref_idx=refi,
                ref_seed=seed, frame_id0=0, frames_per_capture=K, ref_starts=rs, sc16=sc16,
                sc16_scale=scale, out_layout=layout)
    res = rxo.results(slots)
    assert rxo.decode_path() == path, (rxo.decode_path(), path)
    ci, _ = rxo.corr(slots)
    W, G = rxo.W(slots), rxo.G(slots)
    gain = rxo.gain(slots)
    shape = (slots, mo, N, mocc) if sym_major else (slots, N, mo, mocc)
    order = (0, 1, 2, 3) if sym_major else (0, 2, 1, 3)            # -> [slot][sym][N][mocc]
    yg = ig = None
    if want_sym:
        ybytes = osym.host().reshape(shape + (8,)).transpose(order + (4,))
        yg = np.ascontiguousarray(ybytes).view(np.complex64)[..., 0]
        ywritten = ~np.all(ybytes == SYM_FILL, axis=(2, 3, 4))     # [slot][sym]
    if want_idx:
        ig = oidx.host().reshape(shape).transpose(order)
        iwritten = ~np.all(ig == IDX_FILL, axis=(2, 3))
    chk = ds.ElementCheck(qam)
    ok = [f for f in range(slots) if res[f]["status"] == _lib.FRAME_OK]
    assert len(ok) >= max(1, (F if noise_frame is None else F - 1) - 1), \
        [r["status"] for r in res]
    if noise_frame is not None:
        assert res[noise_frame]["status"] == _lib.FRAME_NO_SYNC
        assert any(f > noise_frame for f in ok) and any(f < noise_frame for f in ok)
    if K > 1:
        assert any(res[f]["origin"] > 0 for f in ok), "no second frame of a capture decoded"
    kept = {}
    for f in range(slots):
        r = res[f]
        n = min(r["n_sym"], mo) if r["status"] == _lib.FRAME_OK else 0
        # rows of symbols >= min(n_sym, max_out) and of frames that did not sync stay unwritten
        if want_sym:
            assert not ywritten[f, n:].any() and ywritten[f, :n].all(), (f, n, ywritten[f])
        if want_idx:
            assert not iwritten[f, n:].any() and iwritten[f, :n].all(), (f, n, iwritten[f])
        if n == 0:
            continue
        if K == 1:
            assert n == mo                                     # (PID + 2 callbacks, PID kept)
        y64, u = ds.decode_reference(host[r["capture"]], W[f], gain[f], ci[f], r["sync_index"],
                                     occ_p, cp, nac, n, origin=r["origin"], siso=siso, G=G[f])
        label = "frame %d:" % f
        y = yg[f, :n] if want_sym else None
        chk.frame(y64, u, y=y, idx=ig[f, :n] if want_idx else None, label=label)
        # reference points of the EVM: the transmitted indices, or the decisions themselves
        ysum = y if want_sym else base[f]["y"]
        if ref_mode == 0:
            refidx = ig[f, :n] if want_idx else ds.demap64(ysum, qam)
        else:
            refidx = txh[r["ref_frame"] if K > 1 else f][:, :n].transpose(1, 0, 2)
        s = _qam_points(refidx, qam)
        num = np.sum(np.abs(ysum.astype(np.complex128) - s) ** 2, axis=(0, 2))
        den = np.sum(np.abs(s) ** 2, axis=(0, 2))
        assert np.allclose(r["evm_num"], num, rtol=EVM_RTOL, atol=0), (f, r["evm_num"], num)
        assert np.allclose(r["evm_den"], den, rtol=EVM_RTOL, atol=0), (f, r["evm_den"], den)
        if ref_mode != 0:
            if want_idx:
                err = np.sum(ig[f, :n] != refidx, axis=(0, 2))
            else:
                err = base[f]["errors"]
            assert np.array_equal(r["errors"], err), (f, r["errors"], err)
        kept[f] = dict(y=ysum, errors=r["errors"])
    max_e = chk.finish()
    print("max e %.2f over %d elements, %d excused" % (max_e, chk.total, chk.excused))
    return kept


# ------------------------------------------------------------------------------------
# decode_stream_kernel<LOG2M, NA>: PID 13 and three frames, so that the persistent
# workgroups' symbol ranges straddle frames
STREAM_CASES = {
    "m1024_n2": (1024, 76, 2, 13, 16, ZF2, 301),
    "m1024_n4": (1024, 76, 4, 13, 64, MMSE, 302),
    "m2048_n2": (2048, 152, 2, 13, 4, ZF, 303),
    "m2048_n4": (2048, 152, 4, 13, 256, ZF, 304),
    "m4096_n2": (4096, 304, 2, 13, 64, MMSE, 305),
}


@pytest.mark.parametrize("name", list(STREAM_CASES))
def test_stream_decode_elements(name):
    """One case carries a noise-only frame in the middle of the batch."""
    run_case(*STREAM_CASES[name], STREAM, noise_frame=1 if name == "m2048_n4" else None)


def test_stream_decode_every_reference_mode_and_output_set():
    """decode_stream_kernel<10, 2, R, OUTS>: every ref_mode with symbols and indices, indices
    only, symbols only and neither (EVM only); the sums of the runs without symbols are taken
    over the symbols of the run that delivered both."""
    for ref_mode in (0, 1, 2):
        base = run_case(*STREAM_CASES["m1024_n2"], STREAM, ref_mode=ref_mode)
        for outs in ("sym", "idx", "none"):
            run_case(*STREAM_CASES["m1024_n2"], STREAM, ref_mode=ref_mode, outs=outs, base=base)


@pytest.mark.parametrize("name", ["m1024_n4", "m2048_n2"])
def test_stream_decode_elements_sc16_input(name):
    """The sc16 wire format read in place (ref_mode 1, both outputs: what the streaming decode
    takes without widening); the reference decodes float(i16) * scale."""
    run_case(*STREAM_CASES[name], STREAM, ref_mode=1, sc16=True)


def test_stream_decode_elements_symbol_major():
    run_case(*STREAM_CASES["m2048_n4"], STREAM, ref_mode=1, layout=_lib.LAYOUT_SYMBOL_MAJOR)


def test_stream_decode_elements_back_to_back_frames():
    """Two back-to-back frames per capture (frames_per_capture 3): the second frame's symbols
    start from its own origin."""
    run_case(*STREAM_CASES["m1024_n2"], STREAM, F=2, K=3, ref_mode=1)


# ------------------------------------------------------------------------------------
# split decode (N = 8): PID = M / 64 + 1, the smallest max_out it accepts and one more;
# M 2048 and 4096 take the persistent spectra form
SPLIT_CASES = {
    "m512": (512, 38, 8, 9, 64, MMSE, 311),
    "m1024": (1024, 76, 8, 17, 256, ZF, 312),
    "m2048": (2048, 152, 8, 33, 16, MMSE, 313),
    "m4096": (4096, 304, 8, 65, 4, ZF, 314),
}


@pytest.mark.parametrize("name", list(SPLIT_CASES))
def test_split_decode_elements(name):
    run_case(*SPLIT_CASES[name], SPLIT, F=2, ref_mode=1 if name == "m1024" else 2)


# ------------------------------------------------------------------------------------
# decode_reg_kernel: N 2/4 at M 512..4096 where the streaming decode refuses the geometry
REG_CASES = {
    "m512_n2": ((512, 38, 2, 6, 16, ZF2, 321), {}),
    "m512_n4": ((512, 38, 4, 6, 64, MMSE, 322), {"ref_mode": 1}),
    "m4096_n4": ((4096, 304, 4, 5, 256, ZF, 323), {"F": 2}),
    "m1024_n2_liquid": ((1024, 76, 2, 6, 4, ZF, 324), {"sct": "liquid", "noise_frame": 1}),
    "m2048_n4_liquid": ((2048, 152, 4, 5, 16, MMSE, 325), {"sct": "liquid", "ref_mode": 0}),
    "m1024_n2_siso": ((1024, 76, 2, 6, 64, SISO, 326), {"siso": (1, 0)}),
}


@pytest.mark.parametrize("name", list(REG_CASES))
def test_reg_decode_elements(name):
    geo, kw = REG_CASES[name]
    run_case(*geo, SYMBOL, **kw)


# ------------------------------------------------------------------------------------
# decode_persistent_kernel<8, NA, TP, R>: M 256 with every carrier occupied
@pytest.mark.parametrize("N,qam,det,ref_mode", [(1, 4, ZF, 0), (2, 16, ZF2, 1), (4, 64, MMSE, 2),
                                                 (8, 256, ZF, 1), (2, 256, MMSE, 2),
                                                 (4, 4, ZF, 0)])
def test_persistent_decode_elements(N, qam, det, ref_mode):
    run_case(256, 32, N, 7, qam, det, 330 + N + ref_mode, SYMBOL, ref_mode=ref_mode,
             noise_frame=1 if N == 4 and ref_mode == 2 else None)


# ------------------------------------------------------------------------------------
# decode_kernel: every other geometry
KERNEL_CASES = {
    "m64_n2": ((64, 16, 2, 10, 16, ZF2, 341), {}),
    "m128_n4": ((128, 16, 4, 7, 64, MMSE, 342), {"ref_mode": 1}),
    "m256_n8_liquid": ((256, 32, 8, 5, 256, ZF, 343), {"sct": "liquid", "ref_mode": 0}),
    "m1024_n1": ((1024, 76, 1, 5, 4, ZF, 344), {}),
    # PID 12 < M / 64: below the split decode's threshold
    "m4096_n8": ((4096, 304, 8, 12, 64, MMSE, 345), {"F": 2}),
}


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_symbol_decode_elements(name):
    geo, kw = KERNEL_CASES[name]
    run_case(*geo, SYMBOL, **kw)


# ------------------------------------------------------------------------------------
# weights per carrier on frequency-selective channels
W_F = 3
PIVOT_FLOOR = {8: 8, 4: 3}      # tests/test_decode_model.py measures them on the CPU
DET_NAME = {ZF2: "zf2", ZF: "zf", MMSE: "mmse"}


@pytest.mark.parametrize("N,det,sct", [
    (1, ZF, None), (1, MMSE, "liquid"), (2, ZF, "liquid"), (2, MMSE, None), (2, ZF2, None),
    (2, ZF2, "liquid"), (4, ZF, None), (4, MMSE, "liquid"), (4, MMSE, None),
    (8, ZF, None), (8, MMSE, None), (8, ZF, "liquid"), (8, MMSE, "liquid")])
def test_weights_per_carrier_on_selective_channels(N, det, sct):
    """weights_kernel<1/2/4> and weights_row_kernel<8> against a float64 solve of the handle's
    own G (and the frame's noise_var), carrier by carrier, on captures filtered by select_fir
    (3 taps, seed 7 + frame): the pivot order differs from carrier to carrier, and the test
    counts on the host that it does."""
    import torch
    M, cp, pid, qam, seed = 256, 32, 4, 16, 73
    nac = 4 if N <= 2 else 2
    p = _sctype(M, sct)
    S = Synthesizer(SynthParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid=pid,
                                qam_order=qam, seed=seed, snr_db=30.0, p=p))
    L = max(S.frame_len(i) for i in range(W_F))
    iq = torch.zeros((W_F, N, L), dtype=torch.complex64, device="cuda")
    S.generate(iq, L, L, W_F)
    torch.cuda.synchronize()
    host = iq.cpu().numpy()
    sel = np.stack([ds.select_fir(host[f], 3, 7 + f) for f in range(W_F)])
    iq = torch.from_numpy(sel).cuda()
    rxo = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                            detector=det, qam_order=qam, p=p))
    rxo.process(iq, L, L, W_F, max_out=pid)
    res = rxo.results()
    G, W, gain = rxo.G(), rxo.W(), rxo.gain()
    occ = ds.occupied(rxo.p)
    null = np.setdiff1d(np.arange(M), occ)
    ok = [f for f in range(W_F) if res[f]["status"] == _lib.FRAME_OK]
    assert len(ok) >= 2, [r["status"] for r in res]
    eps = ds.EPS24
    seqs, skipped, total = set(), 0, 0
    for f in ok:
        s2 = float(res[f]["noise_var"])
        Go = G[f][occ].astype(np.complex128)
        W64, g64, cond = ds.weights_reference(Go, s2, DET_NAME[det])
        Wf = W[f][occ].astype(np.complex128)
        assert np.all(W[f][null] == 0), f
        if det == ZF2:
            # det = g00 g11 - g01 g10 in float32: a complex product a b without contraction is
            # off by at most 2 sqrt(2) eps |a| |b| (each component: two products and one
            # difference), the difference of the two by eps |det| more, so |d det| < 4 eps S
            # with S = |g00 g11| + |g01 g10| >= |det|. An entry conj(det) g carries
            # |d det| |g| plus its own product's 2 sqrt(2) eps |det| |g|: within 8 eps S max|g|.
            # gain = 1 / |det|^2: twice det's relative error, the squares, their sum and the
            # division: within (8 eps S / |det| + 4 eps) relative.
            a = np.abs(Go)
            Ssum = a[:, 0, 0] * a[:, 1, 1] + a[:, 0, 1] * a[:, 1, 0]
            bound = 8 * eps * Ssum * a.max(axis=(1, 2))
            assert np.all(np.abs(Wf - W64) <= bound[:, None, None]), \
                (f, (np.abs(Wf - W64) / bound[:, None, None]).max())
            rel = 8 * eps * Ssum * np.sqrt(g64) + 4 * eps          # (sqrt(gain) = 1 / |det|)
            assert np.all(np.abs(gain[f] - g64) <= rel * g64), \
                (f, (np.abs(gain[f] - g64) / (rel * g64)).max())
            continue
        assert np.all(gain[f] == 1.0), f
        # the kernels solve in double: one float32 rounding of the result (2^-24 relative per
        # component) plus a double-solve error far below it for cond(G) < 1e6
        good = cond < 1e6
        skipped += int((~good).sum())
        total += len(occ)
        peak = np.abs(W64).max(axis=(1, 2))
        d = np.abs(Wf - W64).max(axis=(1, 2))
        bad = good & (d > 2.0 ** -23 * peak)
        assert not bad.any(), (f, "carriers", occ[bad][:8], (d / peak)[bad][:8])
        seqs |= {tuple(r) for r in ds.pivot_sequences(ds.solve_matrix(Go, s2, DET_NAME[det]))}
    if det != ZF2:
        assert skipped <= 0.01 * total, (skipped, total)
        print("pivot sequences %d, skipped %d of %d" % (len(seqs), skipped, total))
        if N in PIVOT_FLOOR:
            assert len(seqs) >= PIVOT_FLOOR[N], len(seqs)


def test_batch_gain_argument_errors():
    rxo = Receiver(RxParams(M=64, cp_len=16, num_streams=2, num_access_codes=4, pid_max=4,
                            detector=ZF2, qam_order=4))
    buf = np.zeros(64, np.float32)
    assert _lib.lib().mimo_rx_batch_gain(rxo._h, None, 1) == -1
    assert _lib.lib().mimo_rx_batch_gain(rxo._h, buf.ctypes.data, 1) == -1   # no batch yet
    assert _lib.lib().mimo_rx_batch_gain(rxo._h, buf.ctypes.data, 0) == 0
