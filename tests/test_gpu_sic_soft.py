"""GPU tests of the soft-output SIC pass (mimo_rx_sic_soft; sic_pass_kernel's soft instances,
B > 0, in sic_kernels.hip) against mimo_rx_sic_detect, the same kernel body at B = 0, on the
same batch (z and idx bitwise) and against the written
definition in rub_mimo_amd/sic.py (sic_llr), evaluated in float64 on the call's own z and the
handle's nu_sic. test_gpu_sic.py's cases (every N with a receiver, every QAM order, both
layouts, a guard-band allocation whose rows are no multiple of 16 bytes, the streaming
geometry), plus one whose max_out crosses the kernel's 32-symbol block."""
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest

from postpass_support import (N_FRAMES, NOISE_FRAME, _case_params, _n_out, _res_bytes, _sctype,
                              _synth_capture)
from rub_mimo_amd import _lib, sic, soft
from rub_mimo_amd.receiver import Receiver, RxParams

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "m[0-9]*.npz")))
FORMATS = [_lib.LLR_F32, _lib.LLR_I8]
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
    "qam16_zf_1x1": (64, 16, 1, 4, 10, 16, _lib.DET_ZF, None, 79),
    # max_out = pid + 3 = 37: two 32-symbol blocks, the second partial (5 symbols: a partial
    # iteration of 8) on rows of 2 M_occ bytes, no multiple of 16
    "qpsk_zf_guard_2blocks": (64, 16, 2, 4, 34, 4, _lib.DET_ZF, "liquid", 79),
}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need an MI355X")


def _soft_rc(rx, sym, llr, osym, oidx, n_frames, max_out, layout=0, fmt=_lib.LLR_I8, scale=1.0):
    a = _lib.SicSoft(sym, llr, osym, oidx, n_frames, max_out, layout, fmt, scale)
    return _lib.lib().mimo_rx_sic_soft(rx._h, C.byref(a), None)


class _Out:
    """The pass's three output buffers of one batch shape, pre-filled with garbage: every
    value, erasures included, must be written by the call."""

    def __init__(self, nsym, nb):
        self.nsym, self.nb = nsym, nb
        self.zs = _lib.DeviceBuffer(nsym * 8)
        self.zi = _lib.DeviceBuffer(nsym)
        self.lf = _lib.DeviceBuffer(nsym * nb * 4)
        self.li = _lib.DeviceBuffer(nsym * nb)

    def garbage(self):
        self.zs.upload(np.full(2 * self.nsym, 7.5, np.float32))
        self.zi.upload(np.full(self.nsym, 77, np.uint8))
        self.lf.upload(np.full(self.nsym * self.nb, 7.5, np.float32))
        self.li.upload(np.full(self.nsym * self.nb, 77, np.int8))

    def llr_buf(self, fmt):
        return self.lf if fmt == _lib.LLR_F32 else self.li

    def z(self):
        return self.zs.download(np.uint32, 2 * self.nsym)

    def idx(self):
        return self.zi.download(np.uint8, self.nsym)

    def llr(self, fmt):
        if fmt == _lib.LLR_F32:
            return self.lf.download(np.float32, self.nsym * self.nb)
        return self.li.download(np.int8, self.nsym * self.nb)


@functools.lru_cache(maxsize=None)
def run_case(name, layout):
    """One batch of the case in `layout`, mimo_rx_sic_detect's outputs and mimo_rx_sic_soft's in
    both formats at both scales, computed once and shared (the tests modify none of it)."""
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
    before = (osym.download(np.uint32, nsym * 2), oidx.download(np.uint8, nsym), res)
    order0, nu0 = rx.sic_order(), rx.sic_mse()
    o = _Out(nsym, nb)
    kw = dict(max_out=mo, out_layout=layout)
    o.garbage()
    rx.sic_detect(osym, o.zs, o.zi, **kw)
    rx.results()                                      # (synchronises)
    det_out = (o.z(), o.idx())
    zs, idxs, llr = {}, {}, {}
    for sc in SCALES:
        for fmt in FORMATS:
            o.garbage()
            rx.sic_soft(osym, o.llr_buf(fmt), o.zs, o.zi, fmt=fmt, llr_scale=sc, **kw)
            rx.results()
            zs[fmt, sc], idxs[fmt, sc], llr[fmt, sc] = o.z(), o.idx(), o.llr(fmt)
    # LLRs only: both optional outputs NULL
    o.garbage()
    rx.sic_soft(osym, o.li, None, None, fmt=_lib.LLR_I8, llr_scale=SCALES[1], **kw)
    rx.results()
    llr_only = (o.llr(_lib.LLR_I8), o.z(), o.idx(), o.llr(_lib.LLR_F32))
    # a repeat of the first call
    o.garbage()
    rx.sic_soft(osym, o.lf, o.zs, o.zi, fmt=_lib.LLR_F32, llr_scale=SCALES[0], **kw)
    res2 = rx.results()
    again = (o.z(), o.idx(), o.llr(_lib.LLR_F32))
    after = (osym.download(np.uint32, nsym * 2), oidx.download(np.uint8, nsym), res2)
    order1, nu1 = rx.sic_order(), rx.sic_mse()
    shape = (F, mo, N, mocc) if layout == _lib.LAYOUT_SYMBOL_MAJOR else (F, N, mo, mocc)
    view = (lambda a, *t: a.reshape(shape + t).swapaxes(1, 2)) \
        if layout == _lib.LAYOUT_SYMBOL_MAJOR else (lambda a, *t: a.reshape(shape + t))
    return dict(res=res, before=before, after=after, order=(order0, order1), nu=(nu0, nu1),
                det=det_out, zs=zs, idxs=idxs, raw_llr=llr, llr_only=llr_only, again=again,
                z=view(zs[_lib.LLR_F32, 1.0].view(np.complex64)),      # -> [F][N][mo][M_occ]
                idx=view(idxs[_lib.LLR_F32, 1.0]),
                llr={k: view(v, nb) for k, v in llr.items()},          # -> [F][N][mo][M_occ][2b]
                qam=qam, mo=mo, mocc=mocc, N=N, nb=nb)


@_case_params(CASES)
def test_z_and_idx_are_bitwise_those_of_sic_detect(name, layout):
    c = run_case(name, layout)
    assert c["res"][NOISE_FRAME]["status"] != _lib.FRAME_OK
    assert sum(r["status"] == _lib.FRAME_OK for r in c["res"]) == N_FRAMES - 1
    for key in c["zs"]:
        assert np.array_equal(c["zs"][key], c["det"][0]), key
        assert np.array_equal(c["idxs"][key], c["det"][1]), key
    assert len(np.unique(c["det"][1])) > 1


def _delta_check(z, llr, nu, qam):
    """Check 2 on one frame: z, llr [N][n][M_occ](, [2b]) of the rows the decode wrote, nu
    [N][M_occ] > 0. Returns the worst |LLR nu - delta_ref| / (A^2 + |delta_ref|)."""
    b = soft.qam_bits(qam)
    lmax = soft.qam_levels(qam)[-1]
    zz = z.astype(np.complex128)
    ref = soft.llr_delta(zz, qam)
    got = llr.astype(np.float64) * nu.astype(np.float64)[:, None, :, None]
    A = np.concatenate([np.repeat(np.maximum(np.abs(zz.real), lmax)[..., None], b, -1),
                        np.repeat(np.maximum(np.abs(zz.imag), lmax)[..., None], b, -1)], -1)
    ratio = np.abs(got - ref) / (A ** 2 + np.abs(ref))
    worst = float(ratio.max())
    assert np.all(np.abs(got - ref) <= 1e-5 * (A ** 2 + np.abs(ref))), worst
    return worst


@_case_params(CASES)
def test_fp32_llrs_match_the_definition(name, layout):
    """fp32 LLRs at llr_scale 1 against the definition on the call's own z and the handle's
    nu_sic. Per element |LLR nu_sic - delta_ref(z)| <= 1e-5 (A^2 + |delta_ref|), A = max(|x|,
    l_max): test_llr_matches_definition's bound, for the same handful of fp32 operations (a
    subtraction, a square, a difference of two squares, one division and one product) on terms
    of size A^2, each 6e-8, so about 10x margin. No exclusions. Measured worst ratio: 2.5e-7."""
    c = run_case(name, layout)
    llr = c["llr"][_lib.LLR_F32, 1.0]
    worst = 0.0
    for f, r in enumerate(c["res"]):
        n = _n_out(r, c["mo"])
        if n == 0:
            continue
        nu = c["nu"][1][f]
        assert np.all(nu > 0)
        worst = max(worst, _delta_check(c["z"][f, :, :n], llr[f, :, :n], nu, c["qam"]))
    print("%s layout %d: worst |LLR nu_sic - ref| / (A^2 + |ref|) = %.3g" % (name, layout, worst))


@_case_params(CASES)
def test_int8_is_the_quantised_fp32(name, layout):
    c = run_case(name, layout)
    allv = []
    for sc in SCALES:
        want = soft.quantise_i8(c["raw_llr"][_lib.LLR_F32, sc])
        assert np.array_equal(c["raw_llr"][_lib.LLR_I8, sc], want), sc
        allv.append(c["raw_llr"][_lib.LLR_I8, sc])
    allv = np.concatenate(allv).astype(np.int32)
    print("%s layout %d: int8 LLRs +127 %d, -127 %d, interior non-zero %d" % (
        name, layout, np.sum(allv == 127), np.sum(allv == -127),
        np.sum((np.abs(allv) < 127) & (allv != 0))))
    assert np.any(allv == 127) and np.any(allv == -127)
    assert np.any((np.abs(allv) < 127) & (allv != 0))
    assert not np.any(allv == -128)


@_case_params(CASES)
def test_erasures_are_zero_over_the_garbage(name, layout):
    c = run_case(name, layout)
    erased = 0
    for f, r in enumerate(c["res"]):
        n = _n_out(r, c["mo"])
        assert n < c["mo"]                            # erased rows exist in every frame
        for key, llr in c["llr"].items():
            assert np.all(llr[f, :, n:] == 0), (f, key)
            if n:
                assert np.any(llr[f, :, :n] != 0), (f, key)
        assert np.all(c["z"][f, :, n:].view(np.uint32) == 0) and np.all(c["idx"][f, :, n:] == 0)
        erased += c["idx"][f, :, n:].size
    assert erased > 0 and _n_out(c["res"][NOISE_FRAME], c["mo"]) == 0


@_case_params(CASES)
def test_sign_of_a_nonzero_llr_is_the_bit_of_the_calls_idx(name, layout):
    c = run_case(name, layout)
    nb = c["nb"]
    for f, r in enumerate(c["res"]):
        n = _n_out(r, c["mo"])
        idx = c["idx"][f, :, :n].astype(np.int64)
        for key, llr in c["llr"].items():
            for i in range(nb):
                bit = (idx >> (nb - 1 - i)) & 1
                v = llr[f, :, :n, :, i]
                nz = v != 0
                assert np.array_equal(v[nz] < 0, bit[nz] == 1), (f, key, i)


@_case_params(CASES)
def test_llr_only_call_repeats_and_side_effects(name, layout):
    """With both optional outputs NULL the LLRs are the same and the other buffers keep their
    garbage; a repeat call is bitwise equal; d_sym, the batch's d_out_idx, results(),
    sic_order() and sic_mse() are unchanged by the calls."""
    c = run_case(name, layout)
    only, z_g, idx_g, lf_g = c["llr_only"]
    assert np.array_equal(only, c["raw_llr"][_lib.LLR_I8, SCALES[1]])
    assert np.all(z_g.view(np.float32) == 7.5) and np.all(idx_g == 77) and np.all(lf_g == 7.5)
    assert np.array_equal(c["again"][0], c["zs"][_lib.LLR_F32, SCALES[0]])
    assert np.array_equal(c["again"][1], c["idxs"][_lib.LLR_F32, SCALES[0]])
    assert np.array_equal(c["again"][2].view(np.uint32),
                          c["raw_llr"][_lib.LLR_F32, SCALES[0]].view(np.uint32))
    assert np.array_equal(c["before"][0], c["after"][0])      # d_sym, bitwise
    assert np.array_equal(c["before"][1], c["after"][1])      # the batch's d_out_idx
    assert _res_bytes(c["before"][2]) == _res_bytes(c["after"][2])
    assert np.array_equal(c["order"][0], c["order"][1])
    assert np.array_equal(c["nu"][0].view(np.uint32), c["nu"][1].view(np.uint32))


def _check_pass(rx, res, osym, nsym, shape, qam, mo):
    """Checks 1 and 2 on the last batch of rx (stream-major `shape` [F][N][mo][M_occ]).
    Returns the number of frames whose LLRs were checked."""
    nb = 2 * soft.qam_bits(qam)
    o = _Out(nsym, nb)
    o.garbage()
    rx.sic_detect(osym, o.zs, o.zi, max_out=mo)
    rx.results()
    det = (o.z(), o.idx())
    o.garbage()
    rx.sic_soft(osym, o.lf, o.zs, o.zi, max_out=mo, fmt=_lib.LLR_F32)
    rx.results()
    assert np.array_equal(o.z(), det[0]) and np.array_equal(o.idx(), det[1])
    z = det[0].view(np.complex64).reshape(shape)
    llr = o.llr(_lib.LLR_F32).reshape(shape + (nb,))
    nu = rx.sic_mse(len(res))
    done = 0
    for f, r in enumerate(res):
        n = _n_out(r, mo)
        assert np.all(llr[f, :, n:] == 0)
        if n == 0:
            continue
        assert np.all(nu[f] > 0)
        _delta_check(z[f, :, :n], llr[f, :, :n], nu[f], qam)
        done += 1
    return done


@pytest.mark.parametrize("mode", ["cfo_correct", "split_stages"])
def test_pass_follows_a_cfo_corrected_and_a_split_batch(mode):
    """Checks 1 and 2 after a batch with the opt-in CFO correction, and after a batch run as
    its front half then its decode half (MIMO_STAGES_FRONT, MIMO_STAGES_DECODE)."""
    M, cp, N, nac, pid, qam, det, sct, seed = CASES["qam64_mmse_4x4"]
    iq, L = _synth_capture(M, cp, N, nac, pid, qam, None, seed=seed)
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=det, qam_order=qam, cfo_correct=(mode == "cfo_correct")))
    mocc, mo, F = rx.M_occ, pid + 3, N_FRAMES
    nsym = F * N * mo * mocc
    osym, oidx = _lib.DeviceBuffer(nsym * 8), _lib.DeviceBuffer(nsym)
    osym.zero()
    kw = dict(max_out=mo, out_sym=osym, out_idx=oidx)
    if mode == "split_stages":
        rx.process(iq, L, L, F, stages=_lib.STAGES_FRONT, **kw)
        rx.process(iq, L, L, F, stages=_lib.STAGES_DECODE, **kw)
    else:
        rx.process(iq, L, L, F, **kw)
    res = rx.results()
    assert _check_pass(rx, res, osym, nsym, (F, N, mo, mocc), qam, mo) == N_FRAMES - 1


def test_pass_follows_a_batch_of_back_to_back_frames():
    """frames_per_capture > 1: the frame slots of one capture that holds the golden stream's
    frames back to back, the slot after the last frame erased."""
    g = dict(np.load([p for p in GOLDEN if p.endswith("_stream.npz")][0], allow_pickle=False))
    M, cp, N, nac, pid, qam = (int(g[k]) for k in ("M", "cp", "N", "nac", "pid", "qam"))
    K = int(g["n_ok"]) + 1
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=int(g["detector"]), qam_order=qam, p=g["p"]))
    cap = np.ascontiguousarray(g["rx"])
    L = cap.shape[1]
    iq = _lib.DeviceBuffer(cap.nbytes)
    iq.upload(cap)
    mocc = rx.M_occ
    nsym = K * N * pid * mocc
    osym = _lib.DeviceBuffer(nsym * 8)
    osym.zero()
    rx.process(iq, L, L, 1, max_out=pid, out_sym=osym, frames_per_capture=K)
    res = rx.results(K)
    assert [r["status"] == _lib.FRAME_OK for r in res] == [True] * (K - 1) + [False]
    assert _check_pass(rx, res, osym, nsym, (K, N, pid, mocc), qam, pid) == K - 1


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
    rx.results()
    return rx, out, F, pid, N


def test_state_and_argument_errors():
    """Every error code of mimo_rx_sic_soft in one handle's lifetime, then the two unsupported
    detectors."""
    M, cp, N, nac, pid, qam = 64, 16, 2, 4, 10, 4
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=_lib.DET_ZF2, qam_order=qam))
    F, mocc = N_FRAMES, rx.M_occ
    nsym = F * N * pid * mocc
    osym = _lib.DeviceBuffer(nsym * 8)
    zs = _lib.DeviceBuffer(nsym * 8 + 16)
    zi = _lib.DeviceBuffer(nsym + 16)
    llr = _lib.DeviceBuffer(nsym * 2 * 4 + 16)
    s, l, z, i = osym.addr, llr.addr, zs.addr, zi.addr
    assert _soft_rc(rx, s, l, z, i, F, pid) == -3                     # no batch yet
    iq, L = _synth_capture(M, cp, N, nac, pid, qam, None, seed=75, noise_frame=None)
    rx.process(iq, L, L, F, max_out=pid, out_sym=osym)
    rx.results()
    assert _soft_rc(rx, s, l, z, i, F, pid) == 0
    assert _soft_rc(rx, s, l, z, None, F, pid) == 0
    assert _soft_rc(rx, s, l, None, i, F, pid) == 0
    assert _soft_rc(rx, s, l, None, None, F, pid) == 0                # LLRs alone
    assert _soft_rc(rx, s, l, z, i, F, pid, fmt=_lib.LLR_F32, scale=0.05) == 0
    assert _soft_rc(rx, s, l, z, i, F - 1, pid) == -1                 # not the batch's frames
    assert _soft_rc(rx, s, l, z, i, F, pid - 1) == -1                 # not its max_out
    assert _soft_rc(rx, s, l, z, i, F, pid, layout=1) == -1           # not its layout
    assert _soft_rc(rx, s, l, z, i, F, pid, layout=2) == -1           # no layout at all
    assert _soft_rc(rx, s + 8, l, z, i, F, pid) == -1                 # misaligned d_sym
    assert _soft_rc(rx, s, l + 8, z, i, F, pid) == -1                 # misaligned d_llr
    assert _soft_rc(rx, s, l, z + 8, i, F, pid) == -1                 # misaligned d_out_sym
    assert _soft_rc(rx, s, l, z, i + 4, F, pid) == -1                 # misaligned d_out_idx
    assert _soft_rc(rx, s, l, s, i, F, pid) == -1                     # z over d_sym
    assert _soft_rc(rx, s, l, s + 16, i, F, pid) == -1                # overlapping it
    assert _soft_rc(rx, s, l, z, i, F, pid, scale=0.0) == -1
    assert _soft_rc(rx, s, l, z, i, F, pid, scale=-1.0) == -1
    assert _soft_rc(rx, s, l, z, i, F, pid, scale=float("nan")) == -1
    assert _soft_rc(rx, s, l, z, i, F, pid, scale=float("inf")) == -1
    assert _soft_rc(rx, s, l, z, i, F, pid, fmt=2) == -1
    assert _soft_rc(rx, None, l, z, i, F, pid) == -1
    assert _soft_rc(rx, s, None, z, i, F, pid) == -1                  # d_llr is required
    assert _lib.lib().mimo_rx_sic_soft(rx._h, None, None) == -1
    rx.results()
    # SISO
    g = dict(np.load([p for p in GOLDEN if "siso" in p][0], allow_pickle=False))
    rs, out, Fs, pids, Ns = _golden_batch(g)
    l2 = _lib.DeviceBuffer(Fs * Ns * pids * rs.M_occ * 8)
    assert _soft_rc(rs, out.addr, l2.addr, None, None, Fs, pids) == -6
    # ZF2 at N = 4 (identity weights) never reaches the pass: mimo_rx_create refuses it, as the
    # reference's invert() is 2x2 only; the pass keeps its own MIMO_ERR_UNSUPPORTED behind that
    with pytest.raises(_lib.MimoError, match="2x2 only"):
        Receiver(RxParams(M=128, cp_len=32, num_streams=4, num_access_codes=8, pid_max=8,
                          detector=_lib.DET_ZF2, qam_order=64))


@pytest.mark.parametrize("N,det", [(4, _lib.DET_MMSE), (2, _lib.DET_ZF)], ids=["mmse4", "zf2x2"])
def test_weight_has_the_units_of_the_measured_error_by_stage(N, det):
    """The geometry of test_mse_has_the_units_of_the_measured_error. Per detection stage (the
    streams gathered through sic_order), the measured mean |z - s_tx|^2 against the transmitted
    symbols over the mean nu_sic of that stage. Stage 0 cancels nothing: its ratio lies in
    [0.5, 2], about 1 + N/nac = 1.25 / 1.125 expected (the channel-estimate error is not in the
    model). Later stages must be >= 0.5: nu_sic assumes perfect cancellation, so error
    propagation can only raise them. Measured: 4x4 MMSE 1.24-1.25 at stage 0 and 1.20-1.28 at
    stages 1-3, 2x2 ZF 1.10-1.15 at stage 0 and 1.10-1.15 at stage 1 (at 30 dB and 16-QAM wrong
    decisions are too rare to show)."""
    M, cp, nac, pid, qam = 256, 32, 16, 12, 16
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=det, keep_identity_bias=False, qam_order=qam))
    mocc, F = rx.M_occ, N_FRAMES
    nsym = F * N * pid * mocc
    tx = _lib.DeviceBuffer(nsym)
    iq, L = _synth_capture(M, cp, N, nac, pid, qam, None, seed=76, noise_frame=None, tx=tx)
    out = _lib.DeviceBuffer(nsym * 8)
    rx.process(iq, L, L, F, max_out=pid, out_sym=out, ref_mode=1, ref_idx=tx)
    res = rx.results()
    assert all(r["status"] == _lib.FRAME_OK for r in res)
    o = _Out(nsym, 2 * soft.qam_bits(qam))
    o.garbage()
    rx.sic_soft(out, o.li, o.zs, None, max_out=pid)
    rx.results()
    shape = (F, N, pid, mocc)
    z = o.z().view(np.complex64).reshape(shape).astype(np.complex128)
    sent = sic.qam_points(tx.download(np.uint8, nsym).reshape(shape), qam)
    order, nu = rx.sic_order().astype(np.int64), rx.sic_mse().astype(np.float64)
    ar = np.arange(mocc)
    for f, r in enumerate(res):
        assert _n_out(r, pid) == pid
        err = np.abs(z[f] - sent[f]) ** 2                         # [N][pid][M_occ]
        ratio = np.empty(N)
        for k in range(N):
            pi = order[f, :, k]
            ratio[k] = err[pi, :, ar].mean() / nu[f, pi, ar].mean()
        print("N %d frame %d: measured / predicted error power per stage %s" % (
            N, f, np.round(ratio, 3)))
        assert 0.5 <= ratio[0] <= 2.0, (f, ratio)
        assert np.all(ratio[1:] >= 0.5), (f, ratio)
