"""GPU tests of the soft output (mimo_rx_soft_demap, mimo_rx_batch_mse; soft_kernels.hip)
against the written definition in rub_mimo_amd/soft.py, evaluated in float64 on the GPU's own
downloaded symbols and MSE. Shapes are the smallest that reach every kernel instantiation
(N = 1, 2, 4, 8; 1..4 bits per dimension; both formats), both output layouts, a guard-band
allocation whose symbol count is no multiple of 4, and the streaming decode's geometry."""
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest

from postpass_support import (LAYOUTS, N_FRAMES, NOISE_FRAME, _n_out, _res_bytes, _sctype,
                              _synth_capture)
from rub_mimo_amd import _lib, soft
from rub_mimo_amd.receiver import Receiver, RxParams

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "m[0-9]*.npz")))
GOLDEN = [g for g in GOLDEN if "_stream" not in os.path.basename(g)]
SCALES = (1.0, 0.05)

# M, cp, N, nac, pid, qam, detector, sctype, synthesiser seed (one whose three frames all sync:
# a frame's hashed lead offset decides that, in the oracle as on the GPU)
CASES = {
    "qpsk_zf2": (64, 16, 2, 4, 10, 4, _lib.DET_ZF2, None, 79),
    "qam16_zf_allocc": (256, 32, 2, 4, 10, 16, _lib.DET_ZF, "all", 76),
    "qam64_mmse_4x4": (128, 32, 4, 8, 8, 64, _lib.DET_MMSE, None, 77),
    "qam256_mmse_8x8": (256, 32, 8, 4, 6, 256, _lib.DET_MMSE, None, 79),
    "qpsk_zf_guard": (64, 16, 2, 4, 10, 4, _lib.DET_ZF, "liquid", 79),
    "qam64_mmse_stream": (2048, 152, 4, 20, 4, 64, _lib.DET_MMSE, None, 70),
}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need an MI355X")


def _soft_rc(rx, sym, llr, n_frames, max_out, layout=0, fmt=_lib.LLR_I8, scale=1.0):
    a = _lib.SoftDemap(sym, llr, n_frames, max_out, layout, fmt, scale)
    return _lib.lib().mimo_rx_soft_demap(rx._h, C.byref(a), None)


@functools.lru_cache(maxsize=None)
def run_case(name, layout):
    """One batch of the case in `layout` and its soft outputs, computed once and shared (the
    returned arrays are not modified by the tests)."""
    M, cp, N, nac, pid, qam, det, sct, seed = CASES[name]
    p = _sctype(M, sct)
    iq, L = _synth_capture(M, cp, N, nac, pid, qam, p, seed=seed)
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=det, keep_identity_bias=True, qam_order=qam, p=p))
    mocc, mo, F = rx.M_occ, pid + 3, N_FRAMES
    nsym = F * N * mo * mocc
    nb = 2 * soft.qam_bits(qam)
    osym = _lib.DeviceBuffer(nsym * 8)
    oidx = _lib.DeviceBuffer(nsym)
    osym.zero()
    oidx.zero()
    rx.process(iq, L, L, F, max_out=mo, out_sym=osym, out_idx=oidx, out_layout=layout)
    res = rx.results()
    shape = (F, mo, N, mocc) if layout == _lib.LAYOUT_SYMBOL_MAJOR else (F, N, mo, mocc)
    before = (osym.download(np.uint32, nsym * 2), oidx.download(np.uint8, nsym), res)
    f32, i8 = {}, {}
    lf = _lib.DeviceBuffer(nsym * nb * 4)
    li = _lib.DeviceBuffer(nsym * nb)
    for sc in SCALES:
        # garbage first: every value, erasures included, must be written by the call
        lf.upload(np.full(nsym * nb, 7.5, np.float32))
        li.upload(np.full(nsym * nb, 77, np.int8))
        rx.soft_demap(osym, lf, max_out=mo, out_layout=layout, fmt=_lib.LLR_F32, llr_scale=sc)
        rx.soft_demap(osym, li, max_out=mo, out_layout=layout, fmt=_lib.LLR_I8, llr_scale=sc)
        nu = rx.mse()                        # (synchronises)
        f32[sc] = lf.download(np.float32, nsym * nb).reshape(shape + (nb,))
        i8[sc] = li.download(np.int8, nsym * nb).reshape(shape + (nb,))
    # a second call on the same batch
    rx.soft_demap(osym, li, max_out=mo, out_layout=layout, fmt=_lib.LLR_I8, llr_scale=SCALES[1])
    res2 = rx.results()
    again = li.download(np.int8, nsym * nb).reshape(shape + (nb,))
    after = (osym.download(np.uint32, nsym * 2), oidx.download(np.uint8, nsym), res2)
    y = before[0].view(np.complex64).reshape(shape)
    d = before[1].reshape(shape)
    if layout == _lib.LAYOUT_SYMBOL_MAJOR:   # -> [F][N][mo][M_occ] views for the checks
        tr = lambda a: a.swapaxes(1, 2)
        y, d, again = tr(y), tr(d), tr(again)
        f32 = {k: tr(v) for k, v in f32.items()}
        i8 = {k: tr(v) for k, v in i8.items()}
    return dict(y=y, d=d, res=res, nu=nu, f32=f32, i8=i8, again=again, before=before,
                after=after, qam=qam, mo=mo, mocc=mocc, N=N)


@pytest.mark.parametrize("layout", LAYOUTS, ids=["stream_major", "symbol_major"])
@pytest.mark.parametrize("name", list(CASES))
def test_llr_matches_definition(name, layout):
    """fp32 LLRs at llr_scale 1 against llr_reference on the GPU's own symbols and MSE.
    Per element |LLR nu - delta_ref| <= 1e-5 (A^2 + |delta_ref|), A = max(|x|, l_max): the
    kernel does a handful of fp32 operations (a subtraction, a square, a difference of two
    squares, one division and one product) on terms of size A^2, each with relative error
    6e-8, so 1e-5 leaves about 10x margin."""
    c = run_case(name, layout)
    qam, mo, b = c["qam"], c["mo"], soft.qam_bits(c["qam"])
    lmax = soft.qam_levels(qam)[-1]
    llr = c["f32"][1.0]
    assert c["res"][NOISE_FRAME]["status"] != _lib.FRAME_OK
    print("%s layout %d: frame status %s" % (name, layout, [r["status"] for r in c["res"]]))
    assert sum(r["status"] == _lib.FRAME_OK for r in c["res"]) == N_FRAMES - 1
    worst = 0.0
    for f, r in enumerate(c["res"]):
        n = _n_out(r, mo)
        assert n < mo                         # rows past n_sym exist
        assert np.all(llr[f, :, n:] == 0.0)   # erasures, exactly
        assert np.all(c["nu"][f] == 0.0) == (n == 0)
        if n == 0:
            continue
        y = c["y"][f, :, :n].astype(np.complex128)
        nu = c["nu"][f].astype(np.float64)[:, None, :]
        assert np.all(nu > 0)
        ref = soft.llr_delta(y, qam)
        got = llr[f, :, :n].astype(np.float64) * nu[..., None]
        A = np.concatenate([np.repeat(np.maximum(np.abs(y.real), lmax)[..., None], b, -1),
                            np.repeat(np.maximum(np.abs(y.imag), lmax)[..., None], b, -1)], -1)
        err = np.abs(got - ref) / (A ** 2 + np.abs(ref))
        worst = max(worst, float(err.max()))
        assert np.all(np.abs(got - ref) <= 1e-5 * (A ** 2 + np.abs(ref))), (f, err.max())
        # sign rule: a non-zero LLR's sign is the matching bit of out_idx (positive = 0)
        idx = c["d"][f, :, :n].astype(np.int64)
        for i in range(2 * b):
            bit = (idx >> (2 * b - 1 - i)) & 1
            v = llr[f, :, :n, :][..., i]
            nz = v != 0
            assert np.array_equal(v[nz] < 0, bit[nz] == 1), (f, i)
    print("%s layout %d: worst |LLR nu - ref| / (A^2 + |ref|) = %.3g" % (name, layout, worst))


@pytest.mark.parametrize("layout", LAYOUTS, ids=["stream_major", "symbol_major"])
@pytest.mark.parametrize("name", list(CASES))
def test_int8_is_the_quantised_fp32(name, layout):
    c = run_case(name, layout)
    allv = []
    for sc in SCALES:
        want = soft.quantise_i8(c["f32"][sc])
        assert np.array_equal(c["i8"][sc], want), sc
        allv.append(c["i8"][sc].ravel())
    allv = np.concatenate(allv).astype(np.int32)
    print("%s layout %d: int8 LLRs +127 %d, -127 %d, interior non-zero %d" % (
        name, layout, np.sum(allv == 127), np.sum(allv == -127),
        np.sum((np.abs(allv) < 127) & (allv != 0))))
    assert np.any(allv == 127) and np.any(allv == -127)
    assert np.any((np.abs(allv) < 127) & (allv != 0))
    assert not np.any(allv == -128)


@pytest.mark.parametrize("layout", LAYOUTS, ids=["stream_major", "symbol_major"])
@pytest.mark.parametrize("name", ["qpsk_zf_guard", "qam64_mmse_stream"])
def test_soft_demap_repeats_and_leaves_the_batch_alone(name, layout):
    c = run_case(name, layout)
    assert np.array_equal(c["again"], c["i8"][SCALES[1]])
    assert np.array_equal(c["before"][0], c["after"][0])      # out_sym, bitwise
    assert np.array_equal(c["before"][1], c["after"][1])      # out_idx
    assert _res_bytes(c["before"][2]) == _res_bytes(c["after"][2])


def _golden_batch(g, F=2):
    M, cp, N, nac, pid, qam = (int(g[k]) for k in ("M", "cp", "N", "nac", "pid", "qam"))
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=int(g["detector"]),
                           keep_identity_bias=bool(g["keep_identity_bias"]),
                           siso_tx=int(g["siso_tx"]), siso_rx=int(g["siso_rx"]), qam_order=qam,
                           p=g["p"]))
    host = np.ascontiguousarray(np.broadcast_to(g["rx"], (F,) + g["rx"].shape))
    buf = _lib.DeviceBuffer(host.nbytes)
    buf.upload(host)
    L = g["rx"].shape[1]
    out = _lib.DeviceBuffer(F * N * pid * rx.M_occ * 8)
    rx.process(buf, L, L, F, max_out=pid, out_sym=out)
    res = rx.results()
    assert all(r["status"] == _lib.FRAME_OK for r in res)
    return rx, out, F, pid


@pytest.mark.parametrize("path", [p for p in GOLDEN if "siso" not in p],
                         ids=lambda p: os.path.basename(p))
def test_mse_matches_oracle_estimates(path):
    """mimo_rx_batch_mse on the fixture's capture against mse_reference of the fixture's own
    (oracle) G, W, gain and noise_var: G and W are pinned to 1e-4 of their peaks by the parity
    tests and nu is quadratic in them, hence 1e-3 of nu's peak."""
    g = dict(np.load(path, allow_pickle=False))
    rx, _, F, _ = _golden_batch(g)
    occ = np.flatnonzero(g["p"] != 0)
    want = soft.mse_reference(g["G"], g["W"], g["gain"], float(g["noise_var"]), occ)
    got = rx.mse()
    assert got.shape == (F,) + want.shape and got.dtype == np.float32
    for f in range(F):
        assert np.abs(got[f] - want).max() <= 1e-3 * want.max(), f


def test_siso_is_unsupported():
    g = dict(np.load([p for p in GOLDEN if "siso" in p][0], allow_pickle=False))
    rx, out, F, pid = _golden_batch(g)
    llr = _lib.DeviceBuffer(F * int(g["N"]) * pid * rx.M_occ * 2)
    assert _soft_rc(rx, out.addr, llr.addr, F, pid) == -6
    nu = np.zeros((F, int(g["N"]), rx.M_occ), np.float32)
    assert _lib.lib().mimo_rx_batch_mse(rx._h, nu.ctypes.data, F) == -6


@pytest.mark.parametrize("N,det", [(4, _lib.DET_MMSE), (2, _lib.DET_ZF)], ids=["mmse4", "zf2x2"])
def test_mse_has_the_units_of_the_measured_error(N, det):
    """The measured error power per symbol, evm_num / (n_out M_occ) against the transmitted
    indices, over the mean predicted MSE lies in [0.5, 2]: about 1 + N/nac is expected (the
    channel-estimate error is not in the model); a dn^2 or M_occ slip would be >= 64x.
    Measured: 4x4 MMSE 1.20-1.27 (1 + N/nac = 1.25), 2x2 ZF 1.10-1.16 (1.125). The seed is one
    whose frames' own noise estimates agree: the prediction inherits FrameInfo::noise_var, and a
    frame whose training residual overestimates it (seed 75 frame 2: 6x) reads 0.41-0.61
    ("Units check")."""
    M, cp, nac, pid, qam = 256, 32, 16, 12, 16
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=det, keep_identity_bias=False, qam_order=qam))
    mocc = rx.M_occ
    tx = _lib.DeviceBuffer(N_FRAMES * N * pid * mocc)
    iq, L = _synth_capture(M, cp, N, nac, pid, qam, None, seed=76, noise_frame=None,
                            tx=tx)
    out = _lib.DeviceBuffer(N_FRAMES * N * pid * mocc * 8)
    rx.process(iq, L, L, N_FRAMES, max_out=pid, out_sym=out, ref_mode=1, ref_idx=tx)
    res = rx.results()
    nu = rx.mse().astype(np.float64)
    assert all(r["status"] == _lib.FRAME_OK for r in res)
    for f, r in enumerate(res):
        n = _n_out(r, pid)
        ratio = r["evm_num"] / (n * mocc) / nu[f].mean(axis=1)
        print("N %d frame %d: measured / predicted MSE per stream %s" % (N, f, np.round(ratio, 3)))
        assert np.all((ratio >= 0.5) & (ratio <= 2.0)), (f, ratio)


def test_state_and_argument_errors():
    M, cp, N, nac, pid, qam = 64, 16, 2, 4, 10, 4
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=_lib.DET_ZF2, qam_order=qam))
    F, mocc = N_FRAMES, rx.M_occ
    osym = _lib.DeviceBuffer(F * N * pid * mocc * 8)
    llr = _lib.DeviceBuffer(F * N * pid * mocc * 2 + 16)
    assert _soft_rc(rx, osym.addr, llr.addr, F, pid) == -3          # no batch yet
    nu = np.zeros((F, N, mocc), np.float32)
    assert _lib.lib().mimo_rx_batch_mse(rx._h, nu.ctypes.data, F) == -3
    iq, L = _synth_capture(M, cp, N, nac, pid, qam, None, seed=75, noise_frame=None)
    rx.process(iq, L, L, F, max_out=pid, out_sym=osym)
    rx.results()
    assert _soft_rc(rx, osym.addr, llr.addr, F, pid) == 0
    assert _soft_rc(rx, osym.addr, llr.addr, F - 1, pid) == -1      # not the batch's frames
    assert _soft_rc(rx, osym.addr, llr.addr, F, pid - 1) == -1      # not its max_out
    assert _soft_rc(rx, osym.addr, llr.addr + 8, F, pid) == -1      # misaligned d_llr
    assert _soft_rc(rx, osym.addr + 8, llr.addr, F, pid) == -1      # misaligned d_sym
    assert _soft_rc(rx, osym.addr, llr.addr, F, pid, scale=0.0) == -1
    assert _soft_rc(rx, osym.addr, llr.addr, F, pid, scale=float("nan")) == -1
    assert _soft_rc(rx, osym.addr, llr.addr, F, pid, fmt=2) == -1
    assert _soft_rc(rx, osym.addr, llr.addr, F, pid, layout=2) == -1
    assert _soft_rc(rx, None, llr.addr, F, pid) == -1
    rx.results()
