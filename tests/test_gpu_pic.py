"""GPU tests of the soft-input MMSE-PIC pass (mimo_rx_pic_soft; pic_kernels.hip) against the
written definition in rub_mimo_amd/pic.py, which runs on the handle's G(), noise_var and the
bytes of the priors. Cases are the small rows of test_gpu_sic_soft.py's table plus a 4x4
256-QAM row: both layouts, both formats, llr_scale 1 and 0.05, prior_scale 4 and 0.5, three
kinds of priors (uniform random int8 over the full range, all zero, genie +-127 from the
transmitted indices), a guard-band allocation over two 32-symbol blocks, and N = 1.

Bounds: with u = 2^-24, kappa the 2-norm condition number of A and mag the magnitude sum of
pic.pic_detect, |z_gpu - z_model| <= 8 pic.Z_RATIO_F32 u kappa mag and the relative error of nu
rho = 8 pic.NU_RATIO_F32 u kappa (nu + v) / nu: 8 times the float32 restatement's measured
ratios (tests/test_pic_model.py), the margin the soft-feedback tests gave theirs, for
v_exp_f32 and v_rcp_f32 at 1 ulp and a Q rounded to fp32. The LLRs are checked on the call's own
z as |LLR nu_model / llr_scale - delta(z_gpu)| <= (1e-5 + rho) (A^2 + |delta|), A = max(|x|,
l_max), the soft-feedback tests' form. No exclusions."""
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest

from postpass_support import (N_FRAMES, NOISE_FRAME, _case_params, _n_out, _res_bytes, _sctype,
                              _synth_capture)
from rub_mimo_amd import _lib, fec, pic, sic, soft
from rub_mimo_amd.receiver import Receiver, RxParams, Synthesizer, SynthParams

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "m[0-9]*.npz")))
F32, I8 = _lib.LLR_F32, _lib.LLR_I8
# (format, llr_scale, prior_scale) of every call per kind of priors
COMBOS = [(F32, 1.0, 4.0), (I8, 1.0, 4.0), (F32, 0.05, 0.5), (I8, 0.05, 0.5)]
KINDS = ("random", "zero", "genie")
U = 2.0 ** -24

# M, cp, N, nac, pid, qam, detector, sctype, synthesiser seed
CASES = {
    "qpsk_zf2": (64, 16, 2, 4, 10, 4, _lib.DET_ZF2, None, 79),
    "qam16_zf_allocc": (256, 32, 2, 4, 10, 16, _lib.DET_ZF, "all", 76),
    "qam64_mmse_4x4": (128, 32, 4, 8, 8, 64, _lib.DET_MMSE, None, 77),
    "qpsk_zf_guard_2blocks": (64, 16, 2, 4, 34, 4, _lib.DET_ZF, "liquid", 79),
    "qam16_zf_1x1": (64, 16, 1, 4, 10, 16, _lib.DET_ZF, None, 79),
    "qam256_mmse_4x4": (64, 16, 4, 2, 8, 256, _lib.DET_MMSE, None, 79),
}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need an MI355X")


def _pic_rc(rx, sym, prior, llr, osym, oidx, n_frames, max_out, layout=0, fmt=I8, scale=1.0,
            pscale=1.0):
    a = _lib.PicSoft(sym, prior, llr, osym, oidx, n_frames, max_out, layout, fmt, scale, pscale)
    return _lib.lib().mimo_rx_pic_soft(rx._h, C.byref(a), None)


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
        return self.lf if fmt == F32 else self.li

    def z(self):
        return self.zs.download(np.uint32, 2 * self.nsym)

    def idx(self):
        return self.zi.download(np.uint8, self.nsym)

    def llr(self, fmt):
        if fmt == F32:
            return self.lf.download(np.float32, self.nsym * self.nb)
        return self.li.download(np.int8, self.nsym * self.nb)


def _bits_of(idx, nb):
    return (np.asarray(idx).astype(np.int64)[..., None] >> (nb - 1 - np.arange(nb))) & 1


def _priors(kind, rng, sent, res, mo, nb):
    """Priors [F][N][mo][M_occ][nb] int8 by stream: `kind` on the written rows, 0x80 on every row
    the decode did not write (erased symbols, the noise frame): the pass must not read those.
    The decode writes the frame's tail symbols too, which the synthesiser's tx_idx does not
    cover: their genie priors are +-127 at random."""
    F, N, pid, mocc = sent.shape
    p = np.full((F, N, mo, mocc, nb), -128, np.int8)
    for f, r in enumerate(res):
        n = _n_out(r, mo)
        if kind == "random":
            p[f, :, :n] = rng.integers(-128, 128, (N, n, mocc, nb)).astype(np.int8)
        elif kind == "zero":
            p[f, :, :n] = 0
        else:
            p[f, :, :n] = np.where(rng.integers(0, 2, (N, n, mocc, nb)) == 1, -127, 127)
            k = min(n, pid)
            p[f, :, :k] = np.where(_bits_of(sent[f, :, :k], nb) == 1, -127, 127)
    return p


def _frame_bounds(m):
    """The z tolerance [N][n][J] and the relative nu error rho [N][n][J] of one frame's model."""
    k = U * m["cond"]
    tol = 8.0 * pic.Z_RATIO_F32 * k[None] * m["mag"]
    rho = 8.0 * pic.NU_RATIO_F32 * k[None] * (m["nu"] + m["v"]) / m["nu"]
    return tol, rho


def _llr_check(z, llr, nu, rho, qam, llr_scale=1.0, extra=0.0):
    """|LLR nu / llr_scale - delta(z_gpu)| <= (1e-5 + extra + rho) (A^2 + |delta|), A = max(|x|,
    l_max). Returns the worst ratio to the bound."""
    b = soft.qam_bits(qam)
    lmax = soft.qam_levels(qam)[-1]
    zz = z.astype(np.complex128)
    ref = soft.llr_delta(zz, qam)
    got = llr.astype(np.float64) * nu[..., None] / llr_scale
    A = np.concatenate([np.repeat(np.maximum(np.abs(zz.real), lmax)[..., None], b, -1),
                        np.repeat(np.maximum(np.abs(zz.imag), lmax)[..., None], b, -1)], -1)
    bound = (1e-5 + extra + rho[..., None]) * (A ** 2 + np.abs(ref))
    worst = float((np.abs(got - ref) / bound).max())
    assert np.all(np.abs(got - ref) <= bound), worst
    return worst


@functools.lru_cache(maxsize=None)
def run_case(name, layout):
    """One batch of the case in `layout`; mimo_rx_sic_soft_fb before and after; every kind of
    priors in every combination of COMBOS, the NULL-prior call, the LLR-only call and a repeat;
    the model of every synced frame per (kind, prior_scale). Computed once and shared (the tests
    modify none of it)."""
    M, cp, N, nac, pid, qam, det, sct, seed = CASES[name]
    p = _sctype(M, sct)
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=det, keep_identity_bias=True, qam_order=qam, p=p))
    mocc, mo, F = rx.M_occ, pid + 3, N_FRAMES
    tx = _lib.DeviceBuffer(F * N * pid * mocc)
    iq, L = _synth_capture(M, cp, N, nac, pid, qam, p, seed=seed, tx=tx)
    sent = tx.download(np.uint8, F * N * pid * mocc).reshape(F, N, pid, mocc)
    nsym = F * N * mo * mocc
    nb = 2 * soft.qam_bits(qam)
    osym = _lib.DeviceBuffer(nsym * 8)
    oidx = _lib.DeviceBuffer(nsym)
    osym.zero()
    oidx.zero()
    rx.process(iq, L, L, F, max_out=mo, out_sym=osym, out_idx=oidx, out_layout=layout)
    res = rx.results()
    before = (osym.download(np.uint32, nsym * 2), oidx.download(np.uint8, nsym), res)
    o = _Out(nsym, nb)
    kw = dict(max_out=mo, out_layout=layout)
    sym_major = layout == _lib.LAYOUT_SYMBOL_MAJOR
    shape = (F, mo, N, mocc) if sym_major else (F, N, mo, mocc)
    view = (lambda a, *t: a.reshape(shape + t).swapaxes(1, 2)) if sym_major \
        else (lambda a, *t: a.reshape(shape + t))

    def fb():
        o.garbage()
        rx.sic_soft_fb(osym, o.lf, o.zs, o.zi, fmt=F32, **kw)
        rx.results()
        return o.z(), o.idx(), o.llr(F32)

    fb_before = fb()
    rng = np.random.default_rng(seed)
    pbuf = _lib.DeviceBuffer(nsym * nb)
    priors, calls = {}, {}

    def three(prior, fmt, sc, ps, osym_=True):
        o.garbage()
        rx.pic_soft(osym, o.llr_buf(fmt), prior, o.zs if osym_ else None, o.zi if osym_ else None,
                    fmt=fmt, llr_scale=sc, prior_scale=ps, **kw)
        rx.results()                                  # (synchronises)
        return o.z(), o.idx(), o.llr(fmt)

    for kind in KINDS:
        pr = _priors(kind, rng, sent, res, mo, nb)
        priors[kind] = pr
        pbuf.upload(np.ascontiguousarray(pr.swapaxes(1, 2) if sym_major else pr))
        for fmt, sc, ps in COMBOS:
            calls[kind, fmt, sc, ps] = three(pbuf, fmt, sc, ps)
    null = three(None, F32, 1.0, 4.0)
    # still the genie priors in pbuf: LLRs only, then a repeat of the first genie call
    llr_only = three(pbuf, I8, 0.05, 0.5, osym_=False)
    again = three(pbuf, F32, 1.0, 4.0)
    res2 = rx.results()
    after = (osym.download(np.uint32, nsym * 2), oidx.download(np.uint8, nsym), res2)
    fb_after = fb()
    G, order, nu_sic = rx.G(), rx.sic_order(), rx.sic_mse()
    occ = np.flatnonzero(rx.p != 0)
    y = view(before[0].view(np.complex64))            # -> [F][N][mo][M_occ]
    lam = lambda r: float(np.float32(r["noise_var"])) if det == _lib.DET_MMSE else 0.0
    model = {}
    for f, r in enumerate(res):
        n = _n_out(r, mo)
        if n:
            for kind in KINDS:
                for ps in (4.0, 0.5):
                    model[f, kind, ps] = pic.pic_frame(
                        y[f, :, :n], G[f][occ], float(np.float32(r["noise_var"])), lam(r),
                        priors[kind][f, :, :n], ps, qam, with_bound=True)
    return dict(res=res, before=before, after=after, fb=(fb_before, fb_after), calls=calls,
                null=null, llr_only=llr_only, again=again, model=model, view=view, order=order,
                nu_sic=nu_sic, det=det, qam=qam, mo=mo, mocc=mocc, N=N, nb=nb)


def _z(c, key):
    return c["view"](c["calls"][key][0].view(np.complex64))


@_case_params(CASES)
def test_z_matches_the_model(name, layout):
    """z^ of both fp32 calls of every kind of priors against pic.pic_frame, every written symbol.
    Worst |z_gpu - z_model| / bound measured on the GPU: DESIGN.md "Soft-input MMSE-PIC"."""
    c = run_case(name, layout)
    assert c["res"][NOISE_FRAME]["status"] != _lib.FRAME_OK
    assert sum(r["status"] == _lib.FRAME_OK for r in c["res"]) == N_FRAMES - 1
    worst = 0.0
    for kind in KINDS:
        for fmt, sc, ps in COMBOS:
            z = _z(c, (kind, fmt, sc, ps))
            for f, r in enumerate(c["res"]):
                n = _n_out(r, c["mo"])
                if not n:
                    continue
                m = c["model"][f, kind, ps]
                assert not m["erased"].any()
                tol, _ = _frame_bounds(m)
                err = np.abs(z[f, :, :n].astype(np.complex128) - m["z"])
                worst = max(worst, float((err / tol).max()))
                assert np.all(err <= tol), (kind, ps, f, float((err / tol).max()))
    assert c["model"]
    print("%s layout %d: worst |z_gpu - z_model| / bound = %.3g" % (name, layout, worst))


@_case_params(CASES)
def test_fp32_llrs_match_the_definition(name, layout):
    """The fp32 LLRs at both scales on the call's own z with the model's nu."""
    c = run_case(name, layout)
    worst = 0.0
    for kind in KINDS:
        for fmt, sc, ps in COMBOS:
            if fmt != F32:
                continue
            key = (kind, fmt, sc, ps)
            z, llr = _z(c, key), c["view"](c["calls"][key][2], c["nb"])
            for f, r in enumerate(c["res"]):
                n = _n_out(r, c["mo"])
                if n:
                    m = c["model"][f, kind, ps]
                    _, rho = _frame_bounds(m)
                    worst = max(worst, _llr_check(z[f, :, :n], llr[f, :, :n], m["nu"], rho,
                                                  c["qam"], sc))
    print("%s layout %d: worst |LLR nu - ref| / bound = %.3g" % (name, layout, worst))


@_case_params(CASES)
def test_idx_is_the_slicer_and_int8_the_quantised_fp32(name, layout):
    """idx is the float32 restatement of qam_demap of the call's own z, exactly; z and idx do
    not depend on format or llr_scale; the int8 LLRs are quantise_i8 of the fp32 call's."""
    c = run_case(name, layout)
    allv = []
    for kind in KINDS:
        for fmt, sc, ps in COMBOS:
            zb, ib, lb = c["calls"][kind, fmt, sc, ps]
            z, idx = c["view"](zb.view(np.complex64)), c["view"](ib)
            for f, r in enumerate(c["res"]):
                n = _n_out(r, c["mo"])
                assert np.array_equal(idx[f, :, :n], sic.qam_demap_f32(z[f, :, :n], c["qam"]))
            if fmt == I8:
                zf, jf, lf = c["calls"][kind, F32, sc, ps]
                assert np.array_equal(zb, zf) and np.array_equal(ib, jf)
                assert np.array_equal(lb, soft.quantise_i8(lf)), (kind, sc)
                allv.append(lb)
    allv = np.concatenate(allv).astype(np.int32)
    assert np.any(allv == 127) and np.any(allv == -127)
    assert np.any((np.abs(allv) < 127) & (allv != 0)) and not np.any(allv == -128)
    assert len(np.unique(c["calls"]["random", F32, 1.0, 4.0][1])) > 1


@_case_params(CASES)
def test_null_priors_are_the_zero_buffer_bit_for_bit(name, layout):
    c = run_case(name, layout)
    a, b = c["null"], c["calls"]["zero", F32, 1.0, 4.0]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


@pytest.mark.parametrize("layout", [_lib.LAYOUT_STREAM_MAJOR, _lib.LAYOUT_SYMBOL_MAJOR])
def test_the_priors_are_exercised(layout):
    """In qam64_mmse_4x4 with random priors every written symbol's z^ differs from the
    NULL-prior call's: without that every other check could pass on a kernel that ignores
    d_prior."""
    c = run_case("qam64_mmse_4x4", layout)
    z = _z(c, ("random", F32, 1.0, 4.0))
    z0 = c["view"](c["null"][0].view(np.complex64))
    for f, r in enumerate(c["res"]):
        n = _n_out(r, c["mo"])
        assert np.all(z[f, :, :n] != z0[f, :, :n])


@pytest.mark.parametrize("layout", [_lib.LAYOUT_STREAM_MAJOR, _lib.LAYOUT_SYMBOL_MAJOR])
def test_one_stream_is_bitwise_independent_of_the_priors(layout):
    c = run_case("qam16_zf_1x1", layout)
    for fmt, sc, ps in COMBOS:
        a = c["calls"]["zero", fmt, sc, ps]
        for kind in ("random", "genie"):
            b = c["calls"][kind, fmt, sc, ps]
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            assert np.array_equal(a[2].view(np.uint8), b[2].view(np.uint8))
    assert np.array_equal(c["null"][2].view(np.uint32), c["calls"]["zero", F32, 1.0, 4.0][2].view(np.uint32))


@pytest.mark.parametrize("name", ["qam64_mmse_4x4", "qam256_mmse_4x4"])
@pytest.mark.parametrize("layout", [_lib.LAYOUT_STREAM_MAJOR, _lib.LAYOUT_SYMBOL_MAJOR])
def test_zero_priors_give_stage_0_of_the_sic_pass(name, layout):
    """With zero priors the nu implied by the fp32 LLRs of stream pi_0 (sic_order) is sic_mse's
    nu_sic: |LLR nu_sic - delta(z)| <= (1e-5 + 1e-6 + rho) (A^2 + |delta|), rho the nu bound and
    1e-6 for v, the energy of qam_point's fp32 levels, which is 1 to 2e-7."""
    c = run_case(name, layout)
    key = ("zero", F32, 1.0, 4.0)
    z, llr = _z(c, key), c["view"](c["calls"][key][2], c["nb"])
    ar = np.arange(c["mocc"])
    for f, r in enumerate(c["res"]):
        n = _n_out(r, c["mo"])
        if not n:
            continue
        pi0 = c["order"][f][:, 0].astype(np.int64)
        _, rho = _frame_bounds(c["model"][f, "zero", 4.0])
        nu = np.broadcast_to(c["nu_sic"][f].astype(np.float64)[pi0, ar][None, :], (n, c["mocc"]))
        _llr_check(z[f, :, :n][pi0, :, ar].T, llr[f, :, :n][pi0, :, ar].transpose(1, 0, 2), nu,
                   rho[pi0, :, ar].T, c["qam"], extra=1e-6)


@_case_params(CASES)
def test_erasures_are_zero_over_the_garbage(name, layout):
    """Rows the decode did not write and the noise frame are all zero in every output of every
    call; their priors were 0x80."""
    c = run_case(name, layout)
    erased = 0
    for key, (zb, ib, lb) in c["calls"].items():
        z, idx, llr = c["view"](zb.view(np.uint64)), c["view"](ib), c["view"](lb, c["nb"])
        for f, r in enumerate(c["res"]):
            n = _n_out(r, c["mo"])
            assert n < c["mo"]                            # erased rows exist in every frame
            assert np.all(llr[f, :, n:] == 0), (f, key)
            assert np.all(z[f, :, n:] == 0) and np.all(idx[f, :, n:] == 0)
            if n:
                assert np.any(llr[f, :, :n] != 0), (f, key)
            erased += idx[f, :, n:].size
    assert erased > 0 and _n_out(c["res"][NOISE_FRAME], c["mo"]) == 0


@_case_params(CASES)
def test_llr_only_call_repeats_and_side_effects(name, layout):
    """With both optional outputs NULL the LLRs are the same and the other buffers keep their
    garbage; a repeat call is bitwise equal; d_sym, the batch's d_out_idx and results() are
    unchanged by the calls; a mimo_rx_sic_soft_fb call after them gives the bytes it gave before
    them."""
    c = run_case(name, layout)
    lo_z, lo_i, lo_l = c["llr_only"]
    assert np.array_equal(lo_l, c["calls"]["genie", I8, 0.05, 0.5][2])
    assert np.all(lo_z.view(np.float32) == 7.5) and np.all(lo_i == 77)
    first = c["calls"]["genie", F32, 1.0, 4.0]
    for a, b in ((c["again"], first), (c["fb"][1], c["fb"][0])):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    assert np.array_equal(c["before"][0], c["after"][0])      # d_sym, bitwise
    assert np.array_equal(c["before"][1], c["after"][1])      # the batch's d_out_idx
    assert _res_bytes(c["before"][2]) == _res_bytes(c["after"][2])


def _check_pass(rx, res, osym, nsym, shape, qam, det, mo, seed=5):
    """z, LLRs and erasures of one random-prior fp32 call on the last batch of rx (stream-major
    `shape` [F][N][mo][M_occ]). Returns the number of frames checked against the model."""
    nb = 2 * soft.qam_bits(qam)
    F, N, _, mocc = shape
    prior = np.random.default_rng(seed).integers(-128, 128, shape + (nb,)).astype(np.int8)
    pbuf = _lib.DeviceBuffer(prior.nbytes)
    pbuf.upload(prior)
    o = _Out(nsym, nb)
    o.garbage()
    rx.pic_soft(osym, o.lf, pbuf, o.zs, o.zi, max_out=mo, fmt=F32, prior_scale=4.0)
    rx.results()
    z = o.z().view(np.complex64).reshape(shape)
    idx = o.idx().reshape(shape)
    llr = o.llr(F32).reshape(shape + (nb,))
    y = osym.download(np.complex64, nsym).reshape(shape)
    G = rx.G(len(res))
    occ = np.flatnonzero(rx.p != 0)
    done = 0
    for f, r in enumerate(res):
        n = _n_out(r, mo)
        assert np.all(llr[f, :, n:] == 0) and np.all(idx[f, :, n:] == 0)
        assert np.all(z[f, :, n:].view(np.uint64) == 0)
        if n == 0:
            continue
        s2 = float(np.float32(r["noise_var"]))
        m = pic.pic_frame(y[f, :, :n], G[f][occ], s2, s2 if det == _lib.DET_MMSE else 0.0,
                          prior[f, :, :n], 4.0, qam, with_bound=True)
        tol, rho = _frame_bounds(m)
        assert np.all(np.abs(z[f, :, :n].astype(np.complex128) - m["z"]) <= tol), f
        assert np.array_equal(idx[f, :, :n], sic.qam_demap_f32(z[f, :, :n], qam))
        _llr_check(z[f, :, :n], llr[f, :, :n], m["nu"], rho, qam)
        done += 1
    return done


@pytest.mark.parametrize("mode", ["cfo_correct", "split_stages"])
def test_pass_follows_a_cfo_corrected_and_a_split_batch(mode):
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
    return rx, out, F, pid, N, qam


def test_state_and_argument_errors():
    """Every error code of mimo_rx_pic_soft in one handle's lifetime, then the SISO detector and
    the 8x8 golden configuration."""
    M, cp, N, nac, pid, qam = 64, 16, 2, 4, 10, 4
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=_lib.DET_ZF2, qam_order=qam))
    F, mocc = N_FRAMES, rx.M_occ
    nsym = F * N * pid * mocc
    osym = _lib.DeviceBuffer(nsym * 8)
    zs = _lib.DeviceBuffer(nsym * 8 + 16)
    zi = _lib.DeviceBuffer(nsym + 16)
    llr = _lib.DeviceBuffer(nsym * 2 * 4 + 32)
    pr = _lib.DeviceBuffer(nsym * 2 + 16)
    pr.zero()
    s, l, z, i, p = osym.addr, llr.addr, zs.addr, zi.addr, pr.addr
    assert _pic_rc(rx, s, p, l, z, i, F, pid) == -3                   # no batch yet
    iq, L = _synth_capture(M, cp, N, nac, pid, qam, None, seed=75, noise_frame=None)
    rx.process(iq, L, L, F, max_out=pid, out_sym=osym)
    rx.results()
    assert _pic_rc(rx, s, p, l, z, i, F, pid) == 0
    assert _pic_rc(rx, s, None, l, z, i, F, pid) == 0                 # no priors
    assert _pic_rc(rx, s, p, l, z, None, F, pid) == 0
    assert _pic_rc(rx, s, p, l, None, i, F, pid) == 0
    assert _pic_rc(rx, s, p, l, None, None, F, pid) == 0              # LLRs alone
    assert _pic_rc(rx, s, p, l, z, i, F, pid, fmt=F32, scale=0.05, pscale=0.5) == 0
    assert _pic_rc(rx, s, p, l, z, i, F - 1, pid) == -1               # not the batch's frames
    assert _pic_rc(rx, s, p, l, z, i, F, pid - 1) == -1               # not its max_out
    assert _pic_rc(rx, s, p, l, z, i, F, pid, layout=1) == -1         # not its layout
    assert _pic_rc(rx, s, p, l, z, i, F, pid, layout=2) == -1         # no layout at all
    assert _pic_rc(rx, s + 8, p, l, z, i, F, pid) == -1               # misaligned d_sym
    assert _pic_rc(rx, s, p + 8, l, z, i, F, pid) == -1               # misaligned d_prior
    assert _pic_rc(rx, s, p, l + 8, z, i, F, pid) == -1               # misaligned d_llr
    assert _pic_rc(rx, s, p, l, z + 8, i, F, pid) == -1               # misaligned d_out_sym
    assert _pic_rc(rx, s, p, l, z, i + 4, F, pid) == -1               # misaligned d_out_idx
    assert _pic_rc(rx, s, p, l, s, i, F, pid) == -1                   # z over d_sym
    assert _pic_rc(rx, s, p, l, s + 16, i, F, pid) == -1              # overlapping it
    assert _pic_rc(rx, s, l, l, z, i, F, pid) == -1                   # d_prior over d_llr
    assert _pic_rc(rx, s, l + 16, l, z, i, F, pid) == -1              # overlapping it
    assert _pic_rc(rx, s, l + 16, l, z, i, F, pid, fmt=F32) == -1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert _pic_rc(rx, s, p, l, z, i, F, pid, scale=bad) == -1
        assert _pic_rc(rx, s, p, l, z, i, F, pid, pscale=bad) == -1
    assert _pic_rc(rx, s, p, l, z, i, F, pid, fmt=2) == -1
    assert _pic_rc(rx, None, p, l, z, i, F, pid) == -1
    assert _pic_rc(rx, s, p, None, z, i, F, pid) == -1                # d_llr is required
    assert _lib.lib().mimo_rx_pic_soft(rx._h, None, None) == -1
    rx.results()
    for tag in ("siso", "8x8"):
        g = dict(np.load([q for q in GOLDEN if tag in q][0], allow_pickle=False))
        rs, out, Fs, pids, Ns, qs = _golden_batch(g)
        l2 = _lib.DeviceBuffer(Fs * Ns * pids * rs.M_occ * 8 * 4)
        assert _pic_rc(rs, out.addr, None, l2.addr, None, None, Fs, pids) == -6, tag
        assert b"PIC" in _lib.lib().mimo_last_error() or tag == "siso"


# ---- end to end: detector -> soft-output decoder -> detector --------------------------------
LOOP_SCALE = 4.0
# N, QAM order, snr_db, synthesiser seed: chosen on the CPU (the docstring below)
LOOP_CASES = {"mmse4_qam64": (4, 64, 20.0, 75), "mmse2_qam16": (2, 16, 14.0, 76)}


def loop_codewords(sent, nb, rate, seed):
    """Random info bits per row and their codewords, and the flips x ^ c that turn the
    transmitted random bits x of `sent` ([rows][J] indices) into those codewords by the code's
    linearity. Returns (info [rows][n_info], flip [rows][n_c] bool)."""
    rows, J = sent.shape
    n_c = J * nb
    _, n_info, _ = fec.geometry(rate, n_c)
    info = np.random.default_rng(seed).integers(0, 2, (rows, n_info)).astype(np.uint8)
    c = fec.encode(rate, n_c, info)
    x = _bits_of(sent, nb).reshape(rows, n_c).astype(np.uint8)
    return info, (x ^ c) == 1


def model_loop(y, G_occ, s2, sent, qam, rate=fec.R12, passes=2, seed=11):
    """The float64 model chain on one frame: pic_frame -> int8 at LOOP_SCALE -> decode_siso
    (extrinsic) -> priors at the same scale -> pic_frame. y [N][n][J], sent [N][n][J]. Returns
    the info-bit errors after every pass."""
    N, n, J = y.shape
    nb = 2 * soft.qam_bits(qam)
    info, flip = loop_codewords(sent.reshape(N * n, J), nb, rate, seed)
    prior, errs = None, []
    for _ in range(passes):
        out = pic.pic_frame(y, G_occ, s2, s2, prior, LOOP_SCALE, qam, llr_scale=LOOP_SCALE)
        rows = soft.quantise_i8(out["llr"]).reshape(N * n, J * nb)
        ext, _, il, _ = fec.decode_siso(rate, J * nb, np.where(flip, -rows, rows).astype(np.int8),
                                        mode=fec.SISO_EXT)
        errs.append(int(np.sum((il[:, :info.shape[1]] < 0) != info)))
        prior = np.where(flip, -ext, ext).astype(np.int8).reshape(N, n, J, nb)
    return errs


@pytest.mark.parametrize("name", list(LOOP_CASES))
def test_the_loop_through_the_decoder_removes_errors(name):
    """M 256, cp 32, 16 access codes, 12 symbols, MMSE, plateau_threshold 0.85, three captures of
    which one is replaced by noise; rate 1/2, one codeword per (stream, symbol) row through the
    code's linearity on the synthesiser's transmitted indices; mimo_rx_pic_soft (NULL priors,
    int8 at scale 4) -> mimo_fec_siso (extrinsic) -> mimo_rx_pic_soft (priors at scale 4).
    Asserted: info-bit errors after pass 1 > 0, fewer after pass 2, the noise frame's rows all
    zero LLRs and all-zero info bits.
    Seed and SNR were chosen on the CPU first, with the oracle's synthesiser and framesync
    (threshold 0.85) on the same frames (0 and 2) and model_loop above, over seeds 70..89 at 18
    and 20 dB (4x4; many seeds draw a channel with no error at all) and 10..16 dB (2x2). The
    model chain's info-bit errors per pass there: 5058 -> 88 (-> 27 after a third pass) for 4x4
    64-QAM at 20 dB, seed 75, and 5942 -> 1267 (-> 1246) for 2x2 16-QAM at 14 dB, seed 76.
    DESIGN.md "Soft-input MMSE-PIC" has the GPU's counts beside the model's."""
    N, qam, snr, seed = LOOP_CASES[name]
    M, cp, nac, pid = 256, 32, 16, 12
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=_lib.DET_MMSE, keep_identity_bias=False, qam_order=qam,
                           plateau_threshold=0.85))
    mocc, F = rx.M_occ, N_FRAMES
    nsym = F * N * pid * mocc
    nb = 2 * soft.qam_bits(qam)
    n_c = mocc * nb
    S = Synthesizer(SynthParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid=pid,
                                qam_order=qam, seed=seed, snr_db=snr))
    L = max(S.frame_len(i) for i in range(F))
    iq = _lib.DeviceBuffer(F * N * L * 8)
    tx = _lib.DeviceBuffer(nsym)
    S.generate(iq, L, L, F, tx_idx=tx)
    _lib.check(_lib.lib().mimo_stream_sync(None), "sync")
    host = iq.download(np.complex64, F * N * L).reshape(F, N, L)
    rng = np.random.default_rng(seed)
    host[NOISE_FRAME] = 0.01 * (rng.standard_normal((N, L)) + 1j * rng.standard_normal((N, L)))
    iq.upload(host)
    out = _lib.DeviceBuffer(nsym * 8)
    out.zero()
    rx.process(iq, L, L, F, max_out=pid, out_sym=out)
    res = rx.results()
    assert [r["status"] == _lib.FRAME_OK for r in res] == [f != NOISE_FRAME for f in range(F)]
    sent = tx.download(np.uint8, nsym).reshape(F, N, pid, mocc)
    rows = F * N * pid
    info = np.zeros((rows, fec.geometry(fec.R12, n_c)[1]), np.uint8)
    flip = np.zeros((rows, n_c), bool)
    live = np.zeros(rows, bool)
    for f, r in enumerate(res):
        if f != NOISE_FRAME:
            assert _n_out(r, pid) == pid
            sl = slice(f * N * pid, (f + 1) * N * pid)
            info[sl], flip[sl] = loop_codewords(sent[f].reshape(N * pid, mocc), nb, fec.R12, 11 + f)
            live[sl] = True
    code = fec.Fec(fec.R12, n_c)
    llr, ext, prior = (_lib.DeviceBuffer(rows * n_c) for _ in range(3))
    il = _lib.DeviceBuffer(rows * code.min_info_pitch())
    errs, p = [], None
    for _ in range(2):
        llr.upload(np.full(rows * n_c, 77, np.int8))
        rx.pic_soft(out, llr, p, max_out=pid, llr_scale=LOOP_SCALE, prior_scale=LOOP_SCALE)
        rx.results()
        v = llr.download(np.int8, rows * n_c).reshape(rows, n_c)
        assert np.all(v[~live] == 0)
        llr.upload(np.where(flip, -v, v).astype(np.int8))
        ext.zero()
        code.siso(llr, rows, ext, None, il, None, fec.SISO_EXT)
        _lib.check(_lib.lib().mimo_stream_sync(None), "sync")
        e = ext.download(np.int8, rows * n_c).reshape(rows, n_c)
        bits = il.download(np.int8, rows * code.min_info_pitch()).reshape(rows, -1)[:, :info.shape[1]] < 0
        assert not bits[~live].any()                  # the noise frame decodes to zeros
        errs.append(int(np.sum(bits[live] != info[live])))
        prior.upload(np.where(flip, -e, e).astype(np.int8))
        p = prior
    # the float64 model chain on the handle's own y, G and noise_var, for the record
    y = out.download(np.complex64, nsym).reshape(F, N, pid, mocc)
    G = rx.G()
    occ = np.flatnonzero(rx.p != 0)
    model = np.zeros(2, np.int64)
    for f, r in enumerate(res):
        if f != NOISE_FRAME:
            model += model_loop(y[f], G[f][occ], float(np.float32(r["noise_var"])), sent[f], qam,
                                seed=11 + f)
    print("%s: info-bit errors per pass, GPU %s, model on the handle's estimates %s"
          % (name, errs, model.tolist()))
    assert errs[0] > 0
    assert errs[1] < errs[0]
