"""GPU tests of the ordered MMSE-SIC detector (mimo_rx_sic_detect, mimo_rx_sic_order,
mimo_rx_sic_mse; sic_tables_kernel and sic_pass_kernel's hard-output instances, B = 0, in
sic_kernels.hip) against the written definition in rub_mimo_amd/sic.py,
evaluated in float64 on the GPU's own downloaded G, noise variance and equalised symbols.
The geometries, seeds and 30 dB of test_gpu_soft.py (every kernel instantiation N = 2, 4, 8,
both output layouts, a row length that is no multiple of 4, the streaming decode's geometry),
plus one N = 1 case. N = 3 has kernel instances (as the soft output's MSE kernel has) but no
receiver: mimo_rx_create takes 1, 2, 4 or 8 streams, which test_three_streams_have_no_receiver
pins, so three streams are covered by the model's CPU tests only."""
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest

from postpass_support import (N_FRAMES, NOISE_FRAME, _case_params, _n_out, _res_bytes, _sctype,
                              _synth_capture)
from rub_mimo_amd import _lib, sic
from rub_mimo_amd.receiver import Receiver, RxParams

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "m[0-9]*.npz")))

# M, cp, N, nac, pid, qam, detector, sctype, synthesiser seed (one whose three frames all sync)
CASES = {
    "qpsk_zf2": (64, 16, 2, 4, 10, 4, _lib.DET_ZF2, None, 79),
    "qam16_zf_allocc": (256, 32, 2, 4, 10, 16, _lib.DET_ZF, "all", 76),
    "qam64_mmse_4x4": (128, 32, 4, 8, 8, 64, _lib.DET_MMSE, None, 77),
    "qam256_mmse_8x8": (256, 32, 8, 4, 6, 256, _lib.DET_MMSE, None, 79),
    "qpsk_zf_guard": (64, 16, 2, 4, 10, 4, _lib.DET_ZF, "liquid", 79),
    "qam64_mmse_stream": (2048, 152, 4, 20, 4, 64, _lib.DET_MMSE, None, 70),
    "qam16_zf_1x1": (64, 16, 1, 4, 10, 16, _lib.DET_ZF, None, 79),
}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need an MI355X")


def _sic_rc(rx, sym, osym, oidx, n_frames, max_out, layout=0):
    a = _lib.SicDetect(sym, osym, oidx, n_frames, max_out, layout)
    return _lib.lib().mimo_rx_sic_detect(rx._h, C.byref(a), None)


def _garbage(zs, zi, nsym):
    zs.upload(np.full(2 * nsym, 7.5, np.float32))
    zi.upload(np.full(nsym, 77, np.uint8))


@functools.lru_cache(maxsize=None)
def run_case(name, layout):
    """One batch of the case in `layout`, its SIC outputs and the model's tables for the GPU's
    own G and noise variance, computed once and shared (the tests modify none of it)."""
    M, cp, N, nac, pid, qam, det, sct, seed = CASES[name]
    p = _sctype(M, sct)
    iq, L = _synth_capture(M, cp, N, nac, pid, qam, p, seed=seed)
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=det, keep_identity_bias=True, qam_order=qam, p=p))
    mocc, mo, F = rx.M_occ, pid + 3, N_FRAMES
    nsym = F * N * mo * mocc
    osym = _lib.DeviceBuffer(nsym * 8)
    oidx = _lib.DeviceBuffer(nsym)
    osym.zero()
    oidx.zero()
    rx.process(iq, L, L, F, max_out=mo, out_sym=osym, out_idx=oidx, out_layout=layout)
    res = rx.results()
    shape = (F, mo, N, mocc) if layout == _lib.LAYOUT_SYMBOL_MAJOR else (F, N, mo, mocc)
    before = (osym.download(np.uint32, nsym * 2), oidx.download(np.uint8, nsym), res)
    # the getters work before any detect call
    order0, nu0 = rx.sic_order(), rx.sic_mse()
    zs = _lib.DeviceBuffer(nsym * 8)
    zi = _lib.DeviceBuffer(nsym)
    # garbage first: every value, erasures included, must be written by the call
    _garbage(zs, zi, nsym)
    rx.sic_detect(osym, zs, zi, max_out=mo, out_layout=layout)
    order, nu = rx.sic_order(), rx.sic_mse()          # (synchronises)
    z = zs.download(np.uint32, nsym * 2)
    idx = zi.download(np.uint8, nsym)
    _garbage(zs, zi, nsym)
    rx.sic_detect(osym, None, zi, max_out=mo, out_layout=layout)
    _lib.check(_lib.lib().mimo_stream_sync(None), "sync")
    rx.results()
    idx_only = zi.download(np.uint8, nsym)
    z_untouched = zs.download(np.uint32, nsym * 2)
    _garbage(zs, zi, nsym)
    rx.sic_detect(osym, zs, zi, max_out=mo, out_layout=layout)
    res2 = rx.results()
    again = (zs.download(np.uint32, nsym * 2), zi.download(np.uint8, nsym))
    after = (osym.download(np.uint32, nsym * 2), oidx.download(np.uint8, nsym), res2)
    G = rx.G()
    occ = np.flatnonzero(rx.p != 0)
    view = (lambda a: a.reshape(shape).swapaxes(1, 2)) if layout == _lib.LAYOUT_SYMBOL_MAJOR \
        else (lambda a: a.reshape(shape))              # -> [F][N][mo][M_occ]
    lam = {_lib.DET_MMSE: 1.0}.get(det, 0.0)
    free, forced = {}, {}
    for f, r in enumerate(res):
        if r["status"] != _lib.FRAME_OK:
            continue
        s2 = float(np.float32(r["noise_var"]))
        free[f] = sic.sic_tables(G[f][occ], s2, lam * s2)
        forced[f] = sic.sic_tables(G[f][occ], s2, lam * s2, order=order[f])
    return dict(y=view(before[0].view(np.complex64)), d=view(before[1]), res=res, G=G, occ=occ,
                order=order, nu=nu, order0=order0, nu0=nu0, z=view(z.view(np.complex64)),
                idx=view(idx), raw=(z, idx), idx_only=idx_only, z_untouched=z_untouched,
                again=again, before=before, after=after, free=free, forced=forced, qam=qam,
                mo=mo, mocc=mocc, N=N)


@_case_params(CASES)
def test_order_and_mse_match_the_model(name, layout):
    """sic_order() is the model's order for the GPU's own G() and noise_var on every carrier,
    except where the model's two candidate MSEs of the first differing stage agree to 1e-6
    relative (both are fp64 evaluations of the same quantity; at most 1% of a frame's carriers),
    and sic_mse() is the model's within 1e-5 relative (+1e-12): fp64 arithmetic stored as fp32
    (6e-8), with the model forced to the GPU's order on the tie carriers."""
    c = run_case(name, layout)
    N, mocc = c["N"], c["mocc"]
    assert c["res"][NOISE_FRAME]["status"] != _lib.FRAME_OK
    assert sum(r["status"] == _lib.FRAME_OK for r in c["res"]) == N_FRAMES - 1
    assert np.array_equal(c["order"], c["order0"]) and np.array_equal(c["nu"], c["nu0"])
    assert c["order"].shape == (N_FRAMES, mocc, N) and c["nu"].shape == (N_FRAMES, N, mocc)
    for f, r in enumerate(c["res"]):
        if r["status"] != _lib.FRAME_OK:
            assert np.all(c["order"][f] == 0) and np.all(c["nu"][f] == 0.0)
            continue
        got = c["order"][f].astype(np.int64)
        assert np.array_equal(np.sort(got, axis=1), np.tile(np.arange(N), (mocc, 1)))
        want = c["free"][f][0].astype(np.int64)
        diff = np.flatnonzero(np.any(got != want, axis=1))
        assert len(diff) <= 0.01 * mocc, (f, len(diff))
        if len(diff):
            s2 = float(np.float32(r["noise_var"]))
            cand = sic.sic_stage_mse(c["G"][f][c["occ"]][diff], s2, got[diff])
            for n, j in enumerate(diff):
                k = int(np.flatnonzero(got[j] != want[j])[0])
                a, b = cand[n, k, got[j, k]], cand[n, k, want[j, k]]
                if s2 > 0:
                    a, b = s2 * a / (1 - s2 * a), s2 * b / (1 - s2 * b)
                assert abs(a - b) < 1e-6 * min(a, b), (f, j, k, a, b)
        nu_m = c["forced"][f][3].T                    # [N][M_occ]
        nu_g = c["nu"][f].astype(np.float64)
        err = np.abs(nu_g - nu_m) / (nu_m + 1e-300)
        print("%s layout %d frame %d: %d tie carriers, worst nu_sic relative error %.3g" % (
            name, layout, f, len(diff), err.max()))
        assert np.all(np.abs(nu_g - nu_m) <= 1e-5 * nu_m + 1e-12), (f, err.max())
        assert np.all(nu_g > 0)


@_case_params(CASES)
def test_symbols_match_the_model_teacher_forced(name, layout):
    """Every stage's z against the model's, computed from the GPU's y and the GPU's own earlier
    decisions: |z_gpu - z_model| <= 1e-5 (sum_u |T[k][u]| |y_u| + sum_i |C[k][i]| |s^_i|). The
    kernel stores the tables in fp32 and sums at most 2N fp32 products, so its error is about
    (2N + 2) 6e-8 of that sum, 1e-6 at N = 8; 1e-5 leaves about 10x. No exclusions."""
    c = run_case(name, layout)
    worst = 0.0
    for f, r in enumerate(c["res"]):
        n = _n_out(r, c["mo"])
        if n == 0:
            continue
        order, T, Ct, _ = c["forced"][f]
        y = c["y"][f, :, :n]
        zm, _, mag = sic.sic_apply(y, order, T, Ct, c["qam"], decided=c["idx"][f, :, :n],
                                   with_mag=True)
        err = np.abs(c["z"][f, :, :n].astype(np.complex128) - zm)
        assert np.all(mag > 0)
        worst = max(worst, float((err / mag).max()))
        assert np.all(err <= 1e-5 * mag), (f, (err / mag).max())
    print("%s layout %d: worst |z_gpu - z_model| / magnitude sum = %.3g" % (name, layout, worst))


@_case_params(CASES)
def test_indices_are_the_slicer_of_z_and_erasures_are_zero(name, layout):
    """On every row the decode wrote, d_out_idx is the float32 restatement of qam_demap of the
    GPU's own z, exactly; every other row (the noise frame, symbols >= min(n_sym, max_out)) is
    z = 0 and idx = 0 exactly, over the garbage the buffers held."""
    c = run_case(name, layout)
    erased = 0
    for f, r in enumerate(c["res"]):
        n = _n_out(r, c["mo"])
        assert n < c["mo"]                            # erased rows exist in every frame
        assert np.array_equal(c["idx"][f, :, :n], sic.qam_demap_f32(c["z"][f, :, :n], c["qam"]))
        assert np.all(c["z"][f, :, n:].view(np.uint32) == 0)
        assert np.all(c["idx"][f, :, n:] == 0)
        erased += c["idx"][f, :, n:].size
        if n:
            assert len(np.unique(c["idx"][f, :, :n])) > 1
    assert erased > 0


@_case_params(CASES)
def test_idx_only_output_and_repeatability(name, layout):
    """A call with d_out_sym NULL gives the same indices (and writes no z); a second full call
    repeats both outputs bitwise; d_sym, the batch's d_out_idx and results() are unchanged."""
    c = run_case(name, layout)
    assert np.array_equal(c["idx_only"], c["raw"][1])
    assert np.all(c["z_untouched"].view(np.float32) == 7.5)
    assert np.array_equal(c["again"][0], c["raw"][0])
    assert np.array_equal(c["again"][1], c["raw"][1])
    assert np.array_equal(c["before"][0], c["after"][0])      # d_sym, bitwise
    assert np.array_equal(c["before"][1], c["after"][1])      # the batch's d_out_idx
    assert _res_bytes(c["before"][2]) == _res_bytes(c["after"][2])


@pytest.mark.parametrize("name", ["qam64_mmse_4x4", "qam16_zf_allocc"])
def test_sic_makes_fewer_symbol_errors_than_the_batch(name):
    """Against the synthesiser's transmitted indices (ref_mode 1), no noise frame: the SIC
    indices have strictly fewer symbol errors in total than the batch's own `errors`. The CPU
    simulation of the definition on the oracle's frames gives 4012 < 4482 (4x4 MMSE 64-QAM) and
    394 < 1817 (2x2 ZF 16-QAM) with the identity bias kept, as here; the GPU's y and G are
    pinned to the oracle's at 1e-4, so the counts move by boundary cases only."""
    M, cp, N, nac, pid, qam, det, sct, seed = CASES[name]
    p = _sctype(M, sct)
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=det, keep_identity_bias=True, qam_order=qam, p=p))
    mocc, F = rx.M_occ, N_FRAMES
    nsym = F * N * pid * mocc
    tx = _lib.DeviceBuffer(nsym)
    iq, L = _synth_capture(M, cp, N, nac, pid, qam, p, seed=seed, noise_frame=None, tx=tx)
    osym = _lib.DeviceBuffer(nsym * 8)
    oidx = _lib.DeviceBuffer(nsym)
    zi = _lib.DeviceBuffer(nsym)
    rx.process(iq, L, L, F, max_out=pid, out_sym=osym, out_idx=oidx, ref_mode=1, ref_idx=tx)
    rx.sic_detect(osym, None, zi, max_out=pid)
    res = rx.results()
    assert all(r["status"] == _lib.FRAME_OK for r in res)
    shape = (F, N, pid, mocc)
    sent = tx.download(np.uint8, nsym).reshape(shape)
    lin_idx = oidx.download(np.uint8, nsym).reshape(shape)
    sic_idx = zi.download(np.uint8, nsym).reshape(shape)
    lin = sicn = 0
    for f, r in enumerate(res):
        n = _n_out(r, pid)
        assert n == pid
        lin += int(r["errors"].sum())
        assert int(r["errors"].sum()) == int(np.sum(lin_idx[f, :, :n] != sent[f, :, :n]))
        sicn += int(np.sum(sic_idx[f, :, :n] != sent[f, :, :n]))
    print("%s: batch %d, SIC %d symbol errors of %d" % (name, lin, sicn, nsym))
    assert sicn < lin


def _check_pass(rx, res, y, z, idx, qam, det, mo):
    """The per-frame checks of the tests above on one batch: y, z, idx as [F][N][mo][M_occ].
    Returns the number of frames checked."""
    G, order = rx.G(len(res)), rx.sic_order(len(res))
    occ = np.flatnonzero(rx.p != 0)
    done = 0
    for f, r in enumerate(res):
        n = _n_out(r, mo)
        assert np.all(z[f, :, n:].view(np.uint32) == 0) and np.all(idx[f, :, n:] == 0)
        if n == 0:
            continue
        s2 = float(np.float32(r["noise_var"]))
        lam = s2 if det == _lib.DET_MMSE else 0.0
        free = sic.sic_tables(G[f][occ], s2, lam)[0]
        assert np.sum(np.any(free != order[f], axis=1)) <= 0.01 * len(occ)
        o, T, Ct, _ = sic.sic_tables(G[f][occ], s2, lam, order=order[f])
        zm, _, mag = sic.sic_apply(y[f, :, :n], o, T, Ct, qam, decided=idx[f, :, :n],
                                   with_mag=True)
        assert np.all(np.abs(z[f, :, :n].astype(np.complex128) - zm) <= 1e-5 * mag), f
        assert np.array_equal(idx[f, :, :n], sic.qam_demap_f32(z[f, :, :n], qam))
        done += 1
    return done


@pytest.mark.parametrize("mode", ["cfo_correct", "split_stages"])
def test_pass_follows_a_cfo_corrected_and_a_split_batch(mode):
    """The same checks after a batch with the opt-in CFO correction, and after a batch run as
    its front half then its decode half (MIMO_STAGES_FRONT, MIMO_STAGES_DECODE)."""
    M, cp, N, nac, pid, qam, det, sct, seed = CASES["qam64_mmse_4x4"]
    iq, L = _synth_capture(M, cp, N, nac, pid, qam, None, seed=seed)
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=det, qam_order=qam, cfo_correct=(mode == "cfo_correct")))
    mocc, mo, F = rx.M_occ, pid + 3, N_FRAMES
    nsym = F * N * mo * mocc
    osym, oidx = _lib.DeviceBuffer(nsym * 8), _lib.DeviceBuffer(nsym)
    zs, zi = _lib.DeviceBuffer(nsym * 8), _lib.DeviceBuffer(nsym)
    osym.zero()
    _garbage(zs, zi, nsym)
    kw = dict(max_out=mo, out_sym=osym, out_idx=oidx)
    if mode == "split_stages":
        rx.process(iq, L, L, F, stages=_lib.STAGES_FRONT, **kw)
        rx.process(iq, L, L, F, stages=_lib.STAGES_DECODE, **kw)
    else:
        rx.process(iq, L, L, F, **kw)
    rx.sic_detect(osym, zs, zi, max_out=mo)
    res = rx.results()
    shape = (F, N, mo, mocc)
    y = osym.download(np.complex64, nsym).reshape(shape)
    z = zs.download(np.complex64, nsym).reshape(shape)
    idx = zi.download(np.uint8, nsym).reshape(shape)
    assert _check_pass(rx, res, y, z, idx, qam, det, mo) == N_FRAMES - 1


def test_pass_follows_a_batch_of_back_to_back_frames():
    """frames_per_capture > 1: the frame slots of one capture that holds the golden stream's
    frames back to back, the slot after the last frame erased."""
    g = dict(np.load([p for p in GOLDEN if p.endswith("_stream.npz")][0], allow_pickle=False))
    M, cp, N, nac, pid, qam = (int(g[k]) for k in ("M", "cp", "N", "nac", "pid", "qam"))
    det = int(g["detector"])
    K = int(g["n_ok"]) + 1
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=det, qam_order=qam, p=g["p"]))
    cap = np.ascontiguousarray(g["rx"])
    L = cap.shape[1]
    iq = _lib.DeviceBuffer(cap.nbytes)
    iq.upload(cap)
    mocc = rx.M_occ
    nsym = K * N * pid * mocc
    osym, zs, zi = _lib.DeviceBuffer(nsym * 8), _lib.DeviceBuffer(nsym * 8), _lib.DeviceBuffer(nsym)
    osym.zero()
    _garbage(zs, zi, nsym)
    rx.process(iq, L, L, 1, max_out=pid, out_sym=osym, frames_per_capture=K)
    rx.sic_detect(osym, zs, zi, max_out=pid)
    res = rx.results(K)
    assert [r["status"] == _lib.FRAME_OK for r in res] == [True] * (K - 1) + [False]
    shape = (K, N, pid, mocc)
    y = osym.download(np.complex64, nsym).reshape(shape)
    z = zs.download(np.complex64, nsym).reshape(shape)
    idx = zi.download(np.uint8, nsym).reshape(shape)
    assert np.all(rx.sic_order(K)[K - 1] == 0) and np.all(rx.sic_mse(K)[K - 1] == 0)
    assert _check_pass(rx, res, y, z, idx, qam, det, pid) == K - 1


def test_three_streams_have_no_receiver():
    """The N = 3 case cannot be run: the receiver itself refuses three streams, so no batch
    exists for the SIC pass to follow. If that ever changes, CASES gets an N = 3 row."""
    with pytest.raises(_lib.MimoError, match="-6"):
        Receiver(RxParams(M=64, cp_len=16, num_streams=3, num_access_codes=4, pid_max=10,
                          detector=_lib.DET_MMSE, qam_order=16))


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
    """Every error code of mimo_rx_sic_detect and its getters in one handle's lifetime, then
    the two unsupported detectors."""
    M, cp, N, nac, pid, qam = 64, 16, 2, 4, 10, 4
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=_lib.DET_ZF2, qam_order=qam))
    F, mocc = N_FRAMES, rx.M_occ
    nsym = F * N * pid * mocc
    osym = _lib.DeviceBuffer(nsym * 8)
    zs = _lib.DeviceBuffer(nsym * 8 + 16)
    zi = _lib.DeviceBuffer(nsym + 16)
    order = np.zeros((F, mocc, N), np.uint8)
    nu = np.zeros((F, N, mocc), np.float32)
    L_ = _lib.lib()
    assert _sic_rc(rx, osym.addr, zs.addr, zi.addr, F, pid) == -3          # no batch yet
    assert L_.mimo_rx_sic_order(rx._h, order.ctypes.data, F) == -3
    assert L_.mimo_rx_sic_mse(rx._h, nu.ctypes.data, F) == -3
    iq, L = _synth_capture(M, cp, N, nac, pid, qam, None, seed=75, noise_frame=None)
    rx.process(iq, L, L, F, max_out=pid, out_sym=osym)
    rx.results()
    assert _sic_rc(rx, osym.addr, zs.addr, zi.addr, F, pid) == 0
    assert _sic_rc(rx, osym.addr, zs.addr, None, F, pid) == 0
    assert _sic_rc(rx, osym.addr, None, zi.addr, F, pid) == 0
    assert _sic_rc(rx, osym.addr, zs.addr, zi.addr, F - 1, pid) == -1      # not the batch's frames
    assert _sic_rc(rx, osym.addr, zs.addr, zi.addr, F, pid - 1) == -1      # not its max_out
    assert _sic_rc(rx, osym.addr, zs.addr, zi.addr, F, pid, layout=1) == -1    # not its layout
    assert _sic_rc(rx, osym.addr, zs.addr, zi.addr, F, pid, layout=2) == -1    # no layout at all
    assert _sic_rc(rx, osym.addr + 8, zs.addr, zi.addr, F, pid) == -1      # misaligned d_sym
    assert _sic_rc(rx, osym.addr, zs.addr + 8, zi.addr, F, pid) == -1      # misaligned d_out_sym
    assert _sic_rc(rx, osym.addr, zs.addr, zi.addr + 4, F, pid) == -1      # misaligned d_out_idx
    assert _sic_rc(rx, osym.addr, osym.addr, zi.addr, F, pid) == -1        # z over d_sym
    assert _sic_rc(rx, osym.addr, osym.addr + 16, zi.addr, F, pid) == -1   # overlapping it
    assert _sic_rc(rx, osym.addr, None, None, F, pid) == -1                # no output
    assert _sic_rc(rx, None, zs.addr, zi.addr, F, pid) == -1
    assert L_.mimo_rx_sic_order(rx._h, order.ctypes.data, F + 1) == -1
    assert L_.mimo_rx_sic_mse(rx._h, nu.ctypes.data, F + 1) == -1
    assert L_.mimo_rx_sic_order(rx._h, None, F) == -1
    assert L_.mimo_rx_sic_order(rx._h, order.ctypes.data, F) == 0
    assert L_.mimo_rx_sic_mse(rx._h, nu.ctypes.data, F) == 0
    rx.results()
    # SISO
    g = dict(np.load([p for p in GOLDEN if "siso" in p][0], allow_pickle=False))
    rs, out, Fs, pids, Ns = _golden_batch(g)
    zi2 = _lib.DeviceBuffer(Fs * Ns * pids * rs.M_occ)
    assert _sic_rc(rs, out.addr, None, zi2.addr, Fs, pids) == -6
    o2 = np.zeros((Fs, rs.M_occ, Ns), np.uint8)
    n2 = np.zeros((Fs, Ns, rs.M_occ), np.float32)
    assert L_.mimo_rx_sic_order(rs._h, o2.ctypes.data, Fs) == -6
    assert L_.mimo_rx_sic_mse(rs._h, n2.ctypes.data, Fs) == -6
    # ZF2 at N = 4 (identity weights) never reaches the pass: mimo_rx_create refuses it, as the
    # reference's invert() is 2x2 only; the pass keeps its own MIMO_ERR_UNSUPPORTED behind that
    with pytest.raises(_lib.MimoError, match="2x2 only"):
        Receiver(RxParams(M=128, cp_len=32, num_streams=4, num_access_codes=8, pid_max=8,
                          detector=_lib.DET_ZF2, qam_order=64))
