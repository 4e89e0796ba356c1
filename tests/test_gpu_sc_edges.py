"""GPU parity tests of the Schmidl-Cox decisions where they are close calls (DESIGN.md section 2,
"Exactness of the S&C decision"): the captures of tests/sc_edge_support.py -- tie thresholds,
threshold-hugging and all-ambiguous captures that overflow the exact pass's lists, energy-floor
and zero-window guards, cp edges, and triggers on chunk, iteration and phase boundaries --
received by the HIP path and compared with the oracle. Only exact integers (and the bits of
the f_sc traces) are compared; there are no tolerances. test_sc_edges_model.py asserts on the
CPU that every capture is as adversarial as it is meant to be."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import sc_edge_support as S
from oracle import ref
from rub_mimo_amd import _lib
from rub_mimo_amd import framing as fr
from rub_mimo_amd.receiver import Receiver, RxParams

pytestmark = pytest.mark.gpu

STATUS = {ref.STATE_SEEK_PLATEAU: _lib.FRAME_NO_SYNC,
          ref.STATE_SAVE_ACCESS_CODES: _lib.FRAME_INCOMPLETE,   # synced, window not complete
          ref.STATE_MIMO: _lib.FRAME_OK}
KEYS = ("status", "trigger", "sync_index", "num_samples_processed", "plateau_start",
        "plateau_end")
LOC_AMB = 128        # sync_kernels.hip kLocAmb


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need an MI355X")


def receiver(g, thr):
    return Receiver(RxParams(M=g.M, cp_len=g.cp, num_streams=g.N, num_access_codes=g.nac,
                             pid_max=g.pid, detector=S.detector(g.N), qam_order=S.QAM,
                             plateau_threshold=thr))


def run_batch(g, thr, cases, calls=2, sc16=False):
    """The cases (one geometry, threshold and length) as one batch through Receiver.process,
    `calls` times on one handle (the second call replays the captured graph). Returns each
    call's per-capture sync fields and its sc_exact_count()."""
    F, L = len(cases), cases[0].rx.shape[1]
    if sc16:
        host = np.stack([c.meta["wire"] for c in cases])
        scale = float(cases[0].meta["scale"])
    else:
        host = np.stack([c.rx for c in cases])
        scale = None
    buf = _lib.DeviceBuffer(host.nbytes)
    buf.upload(host)
    rxo = receiver(g, thr)
    rxo.sc_exact_count()
    out = []
    for _ in range(calls):
        rxo.process(buf, L, L, F, max_out=g.pid, sc16=sc16, sc16_scale=scale)
        res = rxo.results(F)
        out.append(([{k: r[k] for k in KEYS} for r in res], rxo.sc_exact_count()))
    return out


def check(case, r):
    """One capture's batch result against the oracle's: the status the oracle's state maps to
    (OK exactly when it reaches STATE_MIMO; INCOMPLETE when it syncs but the capture ends
    inside the window) and, once synced, every sync field bit for bit."""
    w = case.want
    assert r["status"] == STATUS[w["state"]], (case.name, r, w)
    assert r["num_samples_processed"] == w["nsp"], (case.name, r, w)
    if w["synced"]:
        N = case.geom.N
        assert r["sync_index"] == w["sync_index"], (case.name, r, w)
        assert r["plateau_start"][:N] == w["starts"], (case.name, r, w)
        assert r["plateau_end"][:N] == w["ends"], (case.name, r, w)
        assert r["trigger"] == w["trigger"], (case.name, r, w)


def run_and_check(cases, **kw):
    """Every batch of `cases` twice; returns {batch index: [count of call 1, of call 2]}."""
    counts = []
    for g, thr, group in S.batches(cases):
        runs = run_batch(g, thr, group, **kw)
        for res, _ in runs:
            for c, r in zip(group, res):
                check(c, r)
        assert runs[0][0] == runs[1][0], [c.name for c in group]     # graph replay
        counts.append((group, [n for _, n in runs]))
        print("sc_exact_count", [c.name for c in group], [n for _, n in runs])
    return counts


@pytest.mark.parametrize("tag", S.A_TAGS)
def test_tie_pairs(tag):
    """Family A: the threshold equals y32 of the sample that starts a run (or completes it) and
    is one fp32 ulp lower; a GPU chain one ulp off the oracle's at that sample fails one side."""
    for hi, lo in S.family_a(tag):
        run_and_check([hi])
        run_and_check([lo])


@pytest.mark.parametrize("M", [256, 1024, 2048])
def test_hugging_captures(M):
    """Family B: at least 1024 of some 4096 samples before the trigger are inside the band, so
    the exact kernel's per-iteration list (kLocAmb = 128) overflows into the one-lane path.
    sc_exact_count() counts the recomputed samples of a call (list passes and one-lane
    overflow alike): at least 129 after each call."""
    for group, counts in run_and_check([c for c in S.family_b() if c.geom.M == M]):
        assert min(counts) > LOC_AMB, (group, counts)


@pytest.mark.parametrize("M", [64, 128, 256, 1024])
def test_all_ambiguous_captures(M):
    """Family C: every sample of the periodic part is a rounding decision. M 64 and 128 run
    the item path (kScAmbMax = 256 deferred samples per item, then its hot list; the item
    kernel counts what it resolves, lazily: only items that still hold a candidate), M 256
    and 1024 the screened path (count at least 129)."""
    for group, counts in run_and_check([c for c in S.family_c() if c.geom.M == M]):
        assert min(counts) > (LOC_AMB if M >= 256 else 0), (group, counts)


@pytest.mark.parametrize("M", [1024, 256])
def test_energy_floor_and_zero_windows(M):
    """Family D: a burst that puts S0 under the energy floor, exact-zero windows, windows whose
    |x|^2 underflows in fp32, and zeros with the burst: the result of the undisturbed frame."""
    plain, cases = [f for f in S.family_d() if f[0].geom.M == M][0]
    run_and_check([plain] + cases)
    for c in cases:
        assert S.outcome(c.want) == S.outcome(plain.want)


def test_cp_edges():
    """Family E: cp 1, 14 and 15 (the per-bit run condition, cp + 2 <= 16, and the first cp of
    the walk) at M 64 and 256, cp = M/2 at M 256 and 1024, and tie pairs at cp 14 and 15. Every
    geometry is accepted as listed."""
    plain, ties = S.family_e()
    run_and_check(plain)
    for hi, lo in ties:
        run_and_check([hi])
        run_and_check([lo])


def test_boundary_triggers():
    """Family F: triggers on the first position of chunk 1, of an inner iteration and of the
    first phase-2 chunk (16-chunk captures), their neighbours, and a run that straddles the
    chunk boundary."""
    run_and_check(S.family_f())


def test_plain_frames_recompute_little():
    """A plain 30 dB frame keeps sc_exact_count() below what the hugging captures force (129)."""
    for g in (S.Geom(1024, 76, 2, 4, 4), S.Geom(256, 19, 2, 4, 4)):
        c = S.Case("plain_m%d" % g.M, "P", g, 0.95, S.frame(g, 5, 30.0))
        for _, counts in run_and_check([c]):
            assert max(counts) <= LOC_AMB, counts


def test_sc16_input():
    """A hugging case, a tie pair and a boundary case as sc16 wire samples read in place; the
    oracle runs on the widened floats, and thresholds, ties and the landing position come
    from them."""
    f = S.family_sc16()
    for c in (f["hug"],) + f["tie"] + (f["edge"],):
        runs = run_batch(c.geom, c.thr, [c], sc16=True)
        for res, _ in runs:
            check(c, res[0])
        assert runs[0][0] == runs[1][0]


def _phase_cases():
    """One case of each family; F's is a 16-chunk capture whose trigger opens phase 2."""
    e_plain, _ = S.family_e()
    return [S.family_a("A_m256_n2")[0][0], S.family_b()[0], S.family_c()[3],
            S.family_d()[1][1][3], e_plain[4],
            [c for c in S.family_f() if c.name == "F_phase2+0"][0]]


def _phase_runs():
    return [[r for r in run_batch(c.geom, c.thr, [c], calls=1)[0][0]] for c in _phase_cases()]


def test_one_pass_equals_two_phases():
    """One case of each family with the screen in one pass (RMIMO_SC_PHASES=1, read once per
    process: a child interpreter) gives the results of the two-phase run, field for field."""
    two = _phase_runs()
    for c, res in zip(_phase_cases(), two):
        check(c, res[0])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        dst = os.path.join(td, "one_pass.json")
        code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
                "import json, test_gpu_sc_edges as t\n"
                "json.dump(t._phase_runs(), open(%r, 'w'))\nprint('one pass ok')\n"
                % (root, os.path.join(root, "tests"), dst))
        env = dict(os.environ, RMIMO_SC_PHASES="1")
        out = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, timeout=100,
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        one = json.load(open(dst))
    assert one == two


def _facade_cases():
    return {"B_m1024": S.family_b()[4], "C_m1024": S.family_c()[5],
            "D_m1024": S.family_d()[0][1][3], "C_m64": S.family_c()[1]}


@pytest.mark.parametrize("name", ["B_m1024", "C_m1024", "D_m1024", "C_m64"])
def test_streaming_facade_traces(tmp_path, name):
    """Hugging, all-ambiguous and zeros-plus-burst captures fed in ragged chunks through
    framesync.execute with the debug log on: the sync outputs equal the oracle's and f_sc_<k>.dat
    equals the oracle's y32 trace -- NaN (the 0/0 of an all-zero window, whose sign may differ
    between host and device) in the same positions, the same bits everywhere else. Runs stay
    open across the chunk boundaries, which the stream trim's reach-back probe must honour."""
    c = _facade_cases()[name]
    g = c.geom
    o = ref.FrameSyncRef(g.M, g.cp, g.N, g.nac, pid_max=g.pid, detector=S.detector(g.N),
                         threshold=c.thr, trace_sc=True, search_mode=1, qam=S.QAM)
    ms0 = fr.msequence_create(fr.LFSR_SMALL_LENGTH, fr.LFSR_SMALL_0_GEN_POLY, 1)
    ms1 = [fr.msequence_create(fr.LFSR_LARGE_LENGTH, p, 1) for p in fr.s1_polynomials(g.N)]
    fs = fr.framesync(g.M, g.cp, g.N, g.nac, fr.ofdmframe_init_default_sctype(g.M), ms0, ms1,
                      pid_max=g.pid, detector=S.detector(g.N), qam_order=S.QAM,
                      plateau_threshold=c.thr)
    fs.set_debug_log(tmp_path)
    rng = np.random.default_rng(3)
    pos, L = 0, c.rx.shape[1]
    while pos < L:       # the same ragged chunks to both (every call in STATE_MIMO counts a sample)
        n = min(int(rng.integers(1, 5000)), L - pos)
        st = fs.execute([r[pos:pos + n] for r in c.rx], n)
        assert st == o.execute([r[pos:pos + n] for r in c.rx], n), pos
        assert fs.get_num_samples_processed() == o.get_num_samples_processed(), pos
        pos += n
    fs.set_debug_log(None)
    w = c.want
    assert o.state == w["state"]
    if w["synced"]:
        assert fs.get_sync_index() == o.get_sync_index() == w["sync_index"]
        assert [fs.get_plateau_start(s) for s in range(g.N)] == w["starts"]
        assert [fs.get_plateau_end(s) for s in range(g.N)] == w["ends"]
    y32 = np.stack([o.sc_trace(k) for k in range(g.N)])
    assert y32.shape[1] == (w["trigger"] + 1 if w["synced"] else L)
    for k in range(g.N):
        y = np.fromfile(tmp_path / f"f_sc_{k + 1}.dat", np.float32)
        yo = y32[k]
        assert len(y) == len(yo)
        nan = np.isnan(yo)
        assert np.array_equal(np.isnan(y), nan), k
        assert np.array_equal(y[~nan].view(np.uint32), yo[~nan].view(np.uint32)), k
    if name == "D_m1024":
        assert np.isnan(y32).any()


def test_two_frames_per_capture_tie_in_the_second():
    """Back-to-back frames through receive_streams (the stream walk, cert and fixup kernels)
    with the threshold on a tie of the second frame, both sides of the ulp: every frame's
    origin, sync index, plateau starts and ends and samples processed equal ref.stream_ref's."""
    g = S.G_GEOM
    K = 3
    for rx, hi, lo, rh, rl in S.family_streams():
        L = rx.shape[1]
        dev = _lib.DeviceBuffer(rx.nbytes)
        dev.upload(rx)
        for thr, recs in ((hi, rh), (lo, rl)):
            rxo = receiver(g, thr)
            res = rxo.receive_streams(dev, L, L, 1, K, max_out=g.pid)
            assert len(recs) <= K
            for k, o in enumerate(recs):
                r = res[k]
                assert r["status"] == STATUS[o["state"]], (k, r, o)
                assert r["origin"] == o["origin"], (k, r, o)
                assert r["num_samples_processed"] == o["num_samples_processed"], (k, r, o)
                if o["state"] != ref.STATE_SEEK_PLATEAU:
                    assert r["sync_index"] == o["sync_index"], (k, r, o)
                    assert r["plateau_start"] == o["plateau_start"], (k, r, o)
                    assert r["plateau_end"] == o["plateau_end"], (k, r, o)
