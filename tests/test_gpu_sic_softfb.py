"""GPU tests of the soft-feedback SIC pass (mimo_rx_sic_soft_fb; sic_pass_kernel's FB instances
in sic_kernels.hip) against mimo_rx_sic_soft on the same batch (stage 0 bitwise) and against
the written definition in rub_mimo_amd/sic.py (sic_apply_soft, teacher-forced on the call's own
z; sic_llr on the model's nu), with the tables from the model on the handle's G(), noise_var
and detection order and the handle's own nu_sic. Cases of test_gpu_sic_soft.py's table: every
N with a receiver, every QAM order, both layouts, both formats, two scales, a guard-band
allocation over two 32-symbol blocks, and N = 1 (which is mimo_rx_sic_soft throughout)."""
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest

from postpass_support import (N_FRAMES, NOISE_FRAME, _case_params, _n_out, _res_bytes, _sctype,
                              _synth_capture)
from rub_mimo_amd import _lib, sic, soft
from rub_mimo_amd.receiver import Receiver, RxParams, Synthesizer, SynthParams

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "m[0-9]*.npz")))
FORMATS = [_lib.LLR_F32, _lib.LLR_I8]
SCALES = (1.0, 0.05)
U = 2.0 ** -24
K = 64.0

# M, cp, N, nac, pid, qam, detector, sctype, synthesiser seed: test_gpu_sic_soft.py's rows
CASES = {
    "qpsk_zf2": (64, 16, 2, 4, 10, 4, _lib.DET_ZF2, None, 79),
    "qam16_zf_allocc": (256, 32, 2, 4, 10, 16, _lib.DET_ZF, "all", 76),
    "qam64_mmse_4x4": (128, 32, 4, 8, 8, 64, _lib.DET_MMSE, None, 77),
    "qam256_mmse_8x8": (256, 32, 8, 4, 6, 256, _lib.DET_MMSE, None, 79),
    "qpsk_zf_guard_2blocks": (64, 16, 2, 4, 34, 4, _lib.DET_ZF, "liquid", 79),
    "qam16_zf_1x1": (64, 16, 1, 4, 10, 16, _lib.DET_ZF, None, 79),
}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need an MI355X")


def _fb_rc(rx, sym, llr, osym, oidx, n_frames, max_out, layout=0, fmt=_lib.LLR_I8, scale=1.0):
    a = _lib.SicSoft(sym, llr, osym, oidx, n_frames, max_out, layout, fmt, scale)
    return _lib.lib().mimo_rx_sic_soft_fb(rx._h, C.byref(a), None)


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


def _soft_symbol_errors(zf, nuk, qam):
    """The error bounds of one stage's expected symbol and variance as the kernel computes them
    in fp32 from z `zf` and error power `nuk` (both [n][J]): test_sic_softfb_model.py's
    float32 bound at K = 64 per dimension, es = sum over Re and Im of
    K u (1 + d^2 / nu) (1 + |x| / d) d and ev = the same sum with (d^2 + v_dim) in place of d."""
    lv = soft.qam_levels(qam)
    d = lv[1] - lv[0]
    es = np.zeros(zf.shape)
    ev = np.zeros(zf.shape)
    for x in (zf.real, zf.imag):
        vd = 0.5 * sic.soft_symbol(x + 1j * x, nuk, qam)[1]       # one dimension's variance
        base = K * U * (1.0 + d * d / nuk) * (1.0 + np.abs(x) / d)
        es += base * d
        ev += base * (d * d + vd)
    return es, ev


def _frame_model(y, zg, G_occ, s2, det, order, nu_gpu, qam):
    """The teacher-forced model of one frame and the bounds of checks 2 and 4. y, zg
    [N][n][J] the decode's output and the call's own z, G_occ [J][N][N], order [J][N] and
    nu_gpu [N][J] the handle's. Returns z_model, nu_model, the z tolerance
    1e-5 mag_k + sum_{i<k} |C[k][i]| (es_i + 64 rho_i d) and rho_k =
    sum_{l<k} |C[k][l]|^2 ev_l / nu_k, all [N][n][J] by stream, and the stage of every stream
    [N][J]."""
    lam = s2 if det == _lib.DET_MMSE else 0.0
    o, T, Ct, _ = sic.sic_tables(G_occ, s2, lam, order=order)
    zg = zg.astype(np.complex128)
    zm, _, num, mag = sic.sic_apply_soft(y, o, T, Ct, nu_gpu.astype(np.float64).T, qam,
                                         fed_z=zg, with_mag=True)
    assert np.all(mag > 0) and np.all(num > 0)
    N, n, J = zg.shape
    lv = soft.qam_levels(qam)
    d = lv[1] - lv[0]
    ar = np.arange(J)
    od = o.astype(np.int64)
    tol = np.zeros((N, n, J))
    rho = np.zeros((N, n, J))
    stage = np.zeros((N, J), np.int64)
    es, ev = [], []
    for k in range(N):
        pi = od[:, k]
        nuk = num[pi, :, ar].T                                    # [n][J]
        rk = np.zeros((n, J))
        tk = 1e-5 * mag[pi, :, ar].T
        for i in range(k):
            rk += (np.abs(Ct[:, k, i]) ** 2)[None, :] * ev[i] / nuk
        e_s, e_v = _soft_symbol_errors(zg[pi, :, ar].T, nuk, qam)
        es.append(e_s + 64.0 * rk * d)                            # 32 rho d per dimension
        ev.append(e_v)
        for i in range(k):
            tk += np.abs(Ct[:, k, i])[None, :] * es[i]
        tol[pi, :, ar] = tk.T
        rho[pi, :, ar] = rk.T
        stage[pi, ar] = k
    return zm, num, tol, rho, stage


def _llr_check(z, llr, num, rho, qam):
    """Check 4 on one frame: |LLR nu_model - delta(z_gpu)| <= (1e-5 + rho_k) (A^2 + |delta|),
    A = max(|x|, l_max). Returns the worst ratio to the bound."""
    b = soft.qam_bits(qam)
    lmax = soft.qam_levels(qam)[-1]
    zz = z.astype(np.complex128)
    ref = soft.llr_delta(zz, qam)
    got = llr.astype(np.float64) * num[..., None]
    A = np.concatenate([np.repeat(np.maximum(np.abs(zz.real), lmax)[..., None], b, -1),
                        np.repeat(np.maximum(np.abs(zz.imag), lmax)[..., None], b, -1)], -1)
    bound = (1e-5 + rho[..., None]) * (A ** 2 + np.abs(ref))
    worst = float((np.abs(got - ref) / bound).max())
    assert np.all(np.abs(got - ref) <= bound), worst
    return worst


@functools.lru_cache(maxsize=None)
def run_case(name, layout):
    """One batch of the case in `layout`; mimo_rx_sic_soft's outputs in both formats at both
    scales, then mimo_rx_sic_soft_fb's, its LLR-only call and a repeat, then mimo_rx_sic_soft
    once more; the teacher-forced model of every synced frame. Computed once and shared (the
    tests modify none of it)."""
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

    def three(call, fmt, sc):
        o.garbage()
        call(osym, o.llr_buf(fmt), o.zs, o.zi, fmt=fmt, llr_scale=sc, **kw)
        rx.results()                                  # (synchronises)
        return o.z(), o.idx(), o.llr(fmt)

    hard = {(fmt, sc): three(rx.sic_soft, fmt, sc) for sc in SCALES for fmt in FORMATS}
    fb = {(fmt, sc): three(rx.sic_soft_fb, fmt, sc) for sc in SCALES for fmt in FORMATS}
    # LLRs only: both optional outputs NULL
    o.garbage()
    rx.sic_soft_fb(osym, o.li, None, None, fmt=_lib.LLR_I8, llr_scale=SCALES[1], **kw)
    rx.results()
    llr_only = (o.llr(_lib.LLR_I8), o.z(), o.idx(), o.llr(_lib.LLR_F32))
    again = three(rx.sic_soft_fb, _lib.LLR_F32, SCALES[0])
    res2 = rx.results()
    after = (osym.download(np.uint32, nsym * 2), oidx.download(np.uint8, nsym), res2)
    order1, nu1 = rx.sic_order(), rx.sic_mse()
    hard_after = three(rx.sic_soft, _lib.LLR_F32, SCALES[0])
    G = rx.G()
    occ = np.flatnonzero(rx.p != 0)
    shape = (F, mo, N, mocc) if layout == _lib.LAYOUT_SYMBOL_MAJOR else (F, N, mo, mocc)
    view = (lambda a, *t: a.reshape(shape + t).swapaxes(1, 2)) \
        if layout == _lib.LAYOUT_SYMBOL_MAJOR else (lambda a, *t: a.reshape(shape + t))
    y = view(before[0].view(np.complex64))            # -> [F][N][mo][M_occ]
    z = view(fb[_lib.LLR_F32, 1.0][0].view(np.complex64))
    model = {}
    for f, r in enumerate(res):
        n = _n_out(r, mo)
        if n:
            model[f] = _frame_model(y[f, :, :n], z[f, :, :n], G[f][occ],
                                    float(np.float32(r["noise_var"])), det, order1[f], nu1[f],
                                    qam)
    return dict(res=res, before=before, after=after, order=(order0, order1), nu=(nu0, nu1),
                hard=hard, fb=fb, llr_only=llr_only, again=again, hard_after=hard_after,
                model=model, view=view, z=z, idx=view(fb[_lib.LLR_F32, 1.0][1]),
                llr={k: view(v[2], nb) for k, v in fb.items()},   # -> [F][N][mo][M_occ][2b]
                qam=qam, mo=mo, mocc=mocc, N=N, nb=nb)


@_case_params(CASES)
def test_stage0_is_bitwise_that_of_sic_soft(name, layout):
    """Check 1: stage 0 cancels nothing. On every carrier the z, idx and LLRs of stream pi_0
    are mimo_rx_sic_soft's bit for bit, in both formats at both scales, over all rows; at
    N = 1 the whole output is."""
    c = run_case(name, layout)
    assert c["res"][NOISE_FRAME]["status"] != _lib.FRAME_OK
    assert sum(r["status"] == _lib.FRAME_OK for r in c["res"]) == N_FRAMES - 1
    view, nb, ar = c["view"], c["nb"], np.arange(c["mocc"])
    for key in c["fb"]:
        (zh, ih, lh), (zf, jf, lf) = c["hard"][key], c["fb"][key]
        if c["N"] == 1:
            assert np.array_equal(zh, zf) and np.array_equal(ih, jf)
            assert np.array_equal(lh.view(np.uint8), lf.view(np.uint8))
        lw = np.uint32 if key[0] == _lib.LLR_F32 else np.uint8
        for f in range(N_FRAMES):
            pi0 = c["order"][1][f][:, 0].astype(np.int64)
            for a, b, t in ((zh.view(np.uint64), zf.view(np.uint64), ()), (ih, jf, ()),
                            (lh.view(lw), lf.view(lw), (nb,))):
                assert np.array_equal(view(a, *t)[f][pi0, :, ar], view(b, *t)[f][pi0, :, ar]), \
                    (key, f)
    assert len(np.unique(c["fb"][_lib.LLR_F32, 1.0][1])) > 1


@_case_params(CASES)
def test_z_matches_the_model_teacher_forced_on_its_own_z(name, layout):
    """Check 2: every stage's z against sic_apply_soft fed the call's own earlier z (and the
    handle's nu_sic): |z_gpu - z_model| <= 1e-5 mag_k + sum_{i<k} |C[k][i]| (es_i,Re + es_i,Im).
    The first term is the pass's existing bound (tables in fp32, 2N fp32 products). es_i is the
    error of the kernel's fp32 expected symbol: per dimension the float32 bound of
    test_sic_softfb_model.py, K u (1 + d^2 / nu_i) (1 + |x| / d) d, at K = 64 (8x the CPU
    restatement's: v_exp_f32 and v_rcp_f32 at 1 ulp, the log2 e scaling, another summation
    order), plus 32 rho_i d for the kernel's own nu_i being off by rho_i = sum_{l<i} |C[i][l]|^2
    ev_l / nu_i relative (ev the same bound on the variance). No exclusions.
    Worst |z_gpu - z_model| / bound measured: 0.0137 (qam256_mmse_8x8; 0.0113 qam64_mmse_4x4,
    0.0112 qam16_zf_allocc, 0.0058 the QPSK cases, 3e-11 at N = 1 where T = 1), the same in
    both layouts."""
    c = run_case(name, layout)
    worst = 0.0
    for f, (zm, _, tol, _, _) in c["model"].items():
        n = zm.shape[1]
        err = np.abs(c["z"][f, :, :n].astype(np.complex128) - zm)
        worst = max(worst, float((err / tol).max()))
        assert np.all(err <= tol), (f, (err / tol).max())
    assert c["model"]
    print("%s layout %d: worst |z_gpu - z_model| / bound = %.3g" % (name, layout, worst))


@_case_params(CASES)
def test_idx_is_the_slicer_of_the_calls_z(name, layout):
    """Check 3: idx is the float32 restatement of qam_demap of the call's own z, exactly."""
    c = run_case(name, layout)
    for f, r in enumerate(c["res"]):
        n = _n_out(r, c["mo"])
        assert np.array_equal(c["idx"][f, :, :n], sic.qam_demap_f32(c["z"][f, :, :n], c["qam"]))
        if n:
            assert len(np.unique(c["idx"][f, :, :n])) > 1


@_case_params(CASES)
def test_fp32_llrs_match_the_definition(name, layout):
    """Check 4: fp32 LLRs at llr_scale 1 against the definition on the call's own z with the
    teacher-forced model's nu_k: |LLR nu_model - delta(z_gpu)| <= (1e-5 + rho_k) (A^2 +
    |delta|), the soft output's bound plus the relative error rho_k of the kernel's nu_k.
    Measured worst ratio to the bound: 0.025 (the QPSK cases; 0.011-0.012 the others)."""
    c = run_case(name, layout)
    llr = c["llr"][_lib.LLR_F32, 1.0]
    worst = 0.0
    for f, (zm, num, _, rho, _) in c["model"].items():
        n = zm.shape[1]
        worst = max(worst, _llr_check(c["z"][f, :, :n], llr[f, :, :n], num, rho, c["qam"]))
    print("%s layout %d: worst |LLR nu - ref| / bound = %.3g" % (name, layout, worst))


@pytest.mark.parametrize("layout", [_lib.LAYOUT_STREAM_MAJOR, _lib.LAYOUT_SYMBOL_MAJOR])
def test_the_feedback_is_exercised(layout):
    """Check 5: in qam64_mmse_4x4 some written symbols of a stage >= 1 have nu_model > 1.01
    nu_sic, and among those some z differ from mimo_rx_sic_soft's: without that every other
    check could pass on a kernel that cancels hard decisions."""
    c = run_case("qam64_mmse_4x4", layout)
    zh = c["view"](c["hard"][_lib.LLR_F32, 1.0][0].view(np.complex64))
    raised = differ = 0
    for f, (zm, num, _, _, stage) in c["model"].items():
        n = zm.shape[1]
        nu_sic = c["nu"][1][f].astype(np.float64)[:, None, :]
        sel = (num > 1.01 * nu_sic) & (stage[:, None, :] >= 1)
        raised += int(sel.sum())
        differ += int(np.sum(sel & (c["z"][f, :, :n] != zh[f, :, :n])))
    print("layout %d: %d symbols with nu_model > 1.01 nu_sic, %d of them with another z"
          % (layout, raised, differ))
    assert raised > 0 and differ > 0


@_case_params(CASES)
def test_int8_is_the_quantised_fp32(name, layout):
    c = run_case(name, layout)
    allv = []
    for sc in SCALES:
        want = soft.quantise_i8(c["fb"][_lib.LLR_F32, sc][2])
        assert np.array_equal(c["fb"][_lib.LLR_I8, sc][2], want), sc
        allv.append(c["fb"][_lib.LLR_I8, sc][2])
    allv = np.concatenate(allv).astype(np.int32)
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
    garbage; z and idx do not depend on format or scale; a repeat call is bitwise equal;
    d_sym, the batch's d_out_idx, results(), sic_order() and sic_mse() are unchanged by the
    calls; a mimo_rx_sic_soft call after them gives the bytes it gave before them."""
    c = run_case(name, layout)
    only, z_g, idx_g, lf_g = c["llr_only"]
    first = c["fb"][_lib.LLR_F32, SCALES[0]]
    assert np.array_equal(only, c["fb"][_lib.LLR_I8, SCALES[1]][2])
    assert np.all(z_g.view(np.float32) == 7.5) and np.all(idx_g == 77) and np.all(lf_g == 7.5)
    for key, (z, idx, _) in c["fb"].items():
        assert np.array_equal(z, first[0]) and np.array_equal(idx, first[1]), key
    for a, b in ((c["again"], first), (c["hard_after"], c["hard"][_lib.LLR_F32, SCALES[0]])):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    assert np.array_equal(c["before"][0], c["after"][0])      # d_sym, bitwise
    assert np.array_equal(c["before"][1], c["after"][1])      # the batch's d_out_idx
    assert _res_bytes(c["before"][2]) == _res_bytes(c["after"][2])
    assert np.array_equal(c["order"][0], c["order"][1])
    assert np.array_equal(c["nu"][0].view(np.uint32), c["nu"][1].view(np.uint32))


def _check_pass(rx, res, osym, nsym, shape, qam, det, mo):
    """Checks 1 and 4 on the last batch of rx (stream-major `shape` [F][N][mo][M_occ]).
    Returns the number of frames whose LLRs were checked."""
    nb = 2 * soft.qam_bits(qam)
    F, N, _, mocc = shape
    o = _Out(nsym, nb)
    o.garbage()
    rx.sic_soft(osym, o.lf, o.zs, o.zi, max_out=mo, fmt=_lib.LLR_F32)
    rx.results()
    hard = (o.z(), o.idx(), o.llr(_lib.LLR_F32))
    o.garbage()
    rx.sic_soft_fb(osym, o.lf, o.zs, o.zi, max_out=mo, fmt=_lib.LLR_F32)
    rx.results()
    fb = (o.z(), o.idx(), o.llr(_lib.LLR_F32))
    z = fb[0].view(np.complex64).reshape(shape)
    llr = fb[2].reshape(shape + (nb,))
    y = osym.download(np.complex64, nsym).reshape(shape)
    G, order, nu = rx.G(len(res)), rx.sic_order(len(res)), rx.sic_mse(len(res))
    occ = np.flatnonzero(rx.p != 0)
    ar = np.arange(mocc)
    done = 0
    for f, r in enumerate(res):
        n = _n_out(r, mo)
        pi0 = order[f][:, 0].astype(np.int64)
        for a, b, t, w in ((hard[0], fb[0], (), np.uint64), (hard[1], fb[1], (), np.uint8),
                           (hard[2], fb[2], (nb,), np.uint32)):
            assert np.array_equal(a.view(w).reshape(shape + t)[f][pi0, :, ar],
                                  b.view(w).reshape(shape + t)[f][pi0, :, ar]), f
        assert np.all(llr[f, :, n:] == 0)
        if n == 0:
            continue
        zm, num, tol, rho, _ = _frame_model(y[f, :, :n], z[f, :, :n], G[f][occ],
                                            float(np.float32(r["noise_var"])), det, order[f],
                                            nu[f], qam)
        assert np.all(np.abs(z[f, :, :n].astype(np.complex128) - zm) <= tol), f
        _llr_check(z[f, :, :n], llr[f, :, :n], num, rho, qam)
        done += 1
    return done


@pytest.mark.parametrize("mode", ["cfo_correct", "split_stages"])
def test_pass_follows_a_cfo_corrected_and_a_split_batch(mode):
    """Checks 1 and 4 (and 2) after a batch with the opt-in CFO correction, and after a batch
    run as its front half then its decode half (MIMO_STAGES_FRONT, MIMO_STAGES_DECODE)."""
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
    assert _check_pass(rx, res, osym, nsym, (F, N, mo, mocc), qam, det, mo) == N_FRAMES - 1


def test_pass_follows_a_batch_of_back_to_back_frames():
    """frames_per_capture > 1: the frame slots of one capture that holds the golden stream's
    frames back to back, the slot after the last frame erased."""
    g = dict(np.load([p for p in GOLDEN if p.endswith("_stream.npz")][0], allow_pickle=False))
    M, cp, N, nac, pid, qam = (int(g[k]) for k in ("M", "cp", "N", "nac", "pid", "qam"))
    det = int(g["detector"])
    K_ = int(g["n_ok"]) + 1
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=det, qam_order=qam, p=g["p"]))
    cap = np.ascontiguousarray(g["rx"])
    L = cap.shape[1]
    iq = _lib.DeviceBuffer(cap.nbytes)
    iq.upload(cap)
    mocc = rx.M_occ
    nsym = K_ * N * pid * mocc
    osym = _lib.DeviceBuffer(nsym * 8)
    osym.zero()
    rx.process(iq, L, L, 1, max_out=pid, out_sym=osym, frames_per_capture=K_)
    res = rx.results(K_)
    assert [r["status"] == _lib.FRAME_OK for r in res] == [True] * (K_ - 1) + [False]
    assert _check_pass(rx, res, osym, nsym, (K_, N, pid, mocc), qam, det, pid) == K_ - 1


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
    """Every error code of mimo_rx_sic_soft_fb in one handle's lifetime (mimo_rx_sic_soft's
    list), then the SISO detector."""
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
    assert _fb_rc(rx, s, l, z, i, F, pid) == -3                       # no batch yet
    iq, L = _synth_capture(M, cp, N, nac, pid, qam, None, seed=75, noise_frame=None)
    rx.process(iq, L, L, F, max_out=pid, out_sym=osym)
    rx.results()
    assert _fb_rc(rx, s, l, z, i, F, pid) == 0
    assert _fb_rc(rx, s, l, z, None, F, pid) == 0
    assert _fb_rc(rx, s, l, None, i, F, pid) == 0
    assert _fb_rc(rx, s, l, None, None, F, pid) == 0                  # LLRs alone
    assert _fb_rc(rx, s, l, z, i, F, pid, fmt=_lib.LLR_F32, scale=0.05) == 0
    assert _fb_rc(rx, s, l, z, i, F - 1, pid) == -1                   # not the batch's frames
    assert _fb_rc(rx, s, l, z, i, F, pid - 1) == -1                   # not its max_out
    assert _fb_rc(rx, s, l, z, i, F, pid, layout=1) == -1             # not its layout
    assert _fb_rc(rx, s, l, z, i, F, pid, layout=2) == -1             # no layout at all
    assert _fb_rc(rx, s + 8, l, z, i, F, pid) == -1                   # misaligned d_sym
    assert _fb_rc(rx, s, l + 8, z, i, F, pid) == -1                   # misaligned d_llr
    assert _fb_rc(rx, s, l, z + 8, i, F, pid) == -1                   # misaligned d_out_sym
    assert _fb_rc(rx, s, l, z, i + 4, F, pid) == -1                   # misaligned d_out_idx
    assert _fb_rc(rx, s, l, s, i, F, pid) == -1                       # z over d_sym
    assert _fb_rc(rx, s, l, s + 16, i, F, pid) == -1                  # overlapping it
    assert _fb_rc(rx, s, l, z, i, F, pid, scale=0.0) == -1
    assert _fb_rc(rx, s, l, z, i, F, pid, scale=-1.0) == -1
    assert _fb_rc(rx, s, l, z, i, F, pid, scale=float("nan")) == -1
    assert _fb_rc(rx, s, l, z, i, F, pid, scale=float("inf")) == -1
    assert _fb_rc(rx, s, l, z, i, F, pid, fmt=2) == -1
    assert _fb_rc(rx, None, l, z, i, F, pid) == -1
    assert _fb_rc(rx, s, None, z, i, F, pid) == -1                    # d_llr is required
    assert _lib.lib().mimo_rx_sic_soft_fb(rx._h, None, None) == -1
    rx.results()
    # SISO
    g = dict(np.load([p for p in GOLDEN if "siso" in p][0], allow_pickle=False))
    rs, out, Fs, pids, Ns = _golden_batch(g)
    l2 = _lib.DeviceBuffer(Fs * Ns * pids * rs.M_occ * 8)
    assert _fb_rc(rs, out.addr, l2.addr, None, None, Fs, pids) == -6


@pytest.mark.parametrize("N,det", [(4, _lib.DET_MMSE), (2, _lib.DET_ZF)], ids=["mmse4", "zf2x2"])
def test_weight_has_the_units_of_the_measured_error_under_error_propagation(N, det):
    """Check 9. The geometry of test_gpu_sic_soft.py's
    test_weight_has_the_units_of_the_measured_error_by_stage (M 256, cp 32, 16 access codes,
    12 symbols, three frames, seed 76), but 64-QAM at 20 dB with plateau_threshold 0.85, where
    wrong decisions are common and all three frames still sync. Per detection stage and frame,
    the measured mean |z - s_tx|^2 of mimo_rx_sic_soft_fb over the mean nu_k of the
    teacher-forced model lies in [0.5, 2] at stage 0 and in [0.4, 2.5] at the later stages;
    on the same batch mimo_rx_sic_soft's ratio against nu_sic exceeds 2.5 at some stage of
    some frame (else the inputs show nothing).
    Chosen on the CPU first: the oracle's synthesiser and framesync (threshold 0.85) on these
    three frames with the float64 models (sic_tables, sic_apply, sic_apply_soft) alone give
    soft-feedback ratios 1.20-1.46 with 0.74 at one last stage and hard-SIC ratios up to 6.99
    (4x4 MMSE), and 1.06-1.13 against up to 55 (2x2 ZF): both conditions hold in the model."""
    M, cp, nac, pid, qam = 256, 32, 16, 12, 64
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=det, keep_identity_bias=False, qam_order=qam,
                           plateau_threshold=0.85))
    mocc, F = rx.M_occ, N_FRAMES
    nsym = F * N * pid * mocc
    S = Synthesizer(SynthParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid=pid,
                                qam_order=qam, seed=76, snr_db=20.0))
    L = max(S.frame_len(i) for i in range(F))
    iq = _lib.DeviceBuffer(F * N * L * 8)
    tx = _lib.DeviceBuffer(nsym)
    S.generate(iq, L, L, F, tx_idx=tx)
    _lib.check(_lib.lib().mimo_stream_sync(None), "sync")
    out = _lib.DeviceBuffer(nsym * 8)
    rx.process(iq, L, L, F, max_out=pid, out_sym=out, ref_mode=1, ref_idx=tx)
    res = rx.results()
    assert all(r["status"] == _lib.FRAME_OK for r in res)
    o = _Out(nsym, 2 * soft.qam_bits(qam))
    shape = (F, N, pid, mocc)
    o.garbage()
    rx.sic_soft(out, o.li, o.zs, None, max_out=pid)
    rx.results()
    zh = o.z().view(np.complex64).reshape(shape).astype(np.complex128)
    o.garbage()
    rx.sic_soft_fb(out, o.li, o.zs, None, max_out=pid)
    rx.results()
    zf = o.z().view(np.complex64).reshape(shape)
    y = out.download(np.complex64, nsym).reshape(shape)
    sent = sic.qam_points(tx.download(np.uint8, nsym).reshape(shape), qam)
    G, order, nu = rx.G(), rx.sic_order(), rx.sic_mse()
    occ = np.flatnonzero(rx.p != 0)
    ar = np.arange(mocc)
    hard_worst = 0.0
    for f, r in enumerate(res):
        assert _n_out(r, pid) == pid
        _, num, _, _, _ = _frame_model(y[f], zf[f], G[f][occ], float(np.float32(r["noise_var"])),
                                       det, order[f], nu[f], qam)
        err_f = np.abs(zf[f].astype(np.complex128) - sent[f]) ** 2    # [N][pid][M_occ]
        err_h = np.abs(zh[f] - sent[f]) ** 2
        r_fb, r_hard = np.empty(N), np.empty(N)
        for k in range(N):
            pi = order[f][:, k].astype(np.int64)
            r_fb[k] = err_f[pi, :, ar].mean() / num[pi, :, ar].mean()
            r_hard[k] = err_h[pi, :, ar].mean() / nu[f].astype(np.float64)[pi, ar].mean()
        print("N %d frame %d: measured / predicted error power per stage, soft feedback %s, "
              "hard cancellation %s" % (N, f, np.round(r_fb, 3), np.round(r_hard, 3)))
        assert 0.5 <= r_fb[0] <= 2.0, (f, r_fb)
        assert np.all((r_fb[1:] >= 0.4) & (r_fb[1:] <= 2.5)), (f, r_fb)
        hard_worst = max(hard_worst, float(r_hard.max()))
    assert hard_worst > 2.5, hard_worst
