"""Captures on which the Schmidl-Cox decisions are close calls, shared by test_sc_edges_model.py
(CPU: the captures are what they claim to be) and test_gpu_sc_edges.py (GPU: the HIP path
decides every one of them as the oracle does). A plain module, imported by name.

Every capture is generated from a seed here; nothing is read from disk. The oracle
(oracle/ref.py, search_mode 1: the search is not under test) is the definition of every
expected value. Families ("Exactness of the S&C decision"):

  A  tie pairs        real frames, threshold = y32 of a deciding sample and one fp32 ulp lower
  B  hugging          periodic half-symbols + noise, threshold a quantile of the plateau's y32
  C  all-ambiguous    noiseless periodic half-symbols, threshold 1 - k 2^-24
  D  energy floor     real frames behind a burst, exact zeros, or samples whose |x|^2 underflows
  E  cp edges         cp in {1, 14, 15} and cp = M/2
  F  boundaries       triggers on chunk, iteration and phase-1/phase-2 boundaries

Each family function is cached: the model test and the GPU tests of one pytest run share one
set of captures and oracle results, and treat them as read-only."""
import functools
from collections import namedtuple

import numpy as np

from oracle import ref

QAM = 16
U24 = 2.0 ** -24
SC_SPAN, SC_ITER = 16384, 4096      # kernels.hpp kScSpan, kScIterLen

Geom = namedtuple("Geom", "M cp N nac pid")


def band(M):
    """engine_stages.cpp sc_band(M): the half-width of the fp64 metric's decision band."""
    return 1.25 * U24 * (np.sqrt(2.0) * (M + 4.0) + 2.0 * M + 6.0)


def chunk_len(cp):
    """kernels.hpp sc_chunk_len(cp): candidate positions per 16384-sample S&C item."""
    return SC_SPAN - (cp + 2 + 15) // 16 * 16


def first_phase2_chunk(g):
    """engine_stages.cpp run_sync: the first chunk of the second screen phase (captures of at
    least 16 chunks)."""
    K = chunk_len(g.cp)
    s0_end = (g.M + g.cp) * (g.N * g.nac + 4) + g.M
    return max(2, (s0_end + K - 1) // K + 1)


def ulp_below(y):
    return float(np.nextafter(np.float32(y), np.float32(-np.inf)))


def detector(N):
    return ref.DET_ZF2 if N == 2 else ref.DET_MMSE


class Case:
    """One capture, its geometry and threshold, and the oracle's verdict on it (`want`)."""

    def __init__(self, name, family, geom, thr, rx, **meta):
        self.name, self.family, self.geom, self.thr = name, family, geom, float(thr)
        self.rx = np.ascontiguousarray(rx, np.complex64)
        self.rx.setflags(write=False)
        self.meta = meta
        self._want = None

    @property
    def want(self):
        if self._want is None:
            self._want = run_oracle(self.rx, self.geom, self.thr)
        return self._want

    def __repr__(self):
        return "Case(%s)" % self.name


def run_oracle(rx, g, thr, trace=False):
    """The oracle's framesync over the whole capture: state, sync_index, plateau starts and
    ends, trigger (the sample at which the plateau rule fired), samples processed and, with
    trace, y32 [N][samples scanned while seeking]."""
    o = ref.FrameSyncRef(g.M, g.cp, g.N, g.nac, pid_max=g.pid, detector=detector(g.N),
                         threshold=float(thr), trace_sc=trace, search_mode=1, qam=QAM)
    st = o.execute(list(rx))
    d = dict(state=st, synced=st != ref.STATE_SEEK_PLATEAU, sync_index=o.get_sync_index(),
             starts=[o.get_plateau_start(s) for s in range(g.N)],
             ends=[o.get_plateau_end(s) for s in range(g.N)],
             nsp=o.get_num_samples_processed())
    # at the trigger every antenna is inside its run, so each plateau_end is that sample
    d["trigger"] = d["ends"][0] if d["synced"] else None
    if trace:
        d["y32"] = np.stack([o.sc_trace(s) for s in range(g.N)])
    return d


def outcome(d):
    """The integers the GPU must reproduce."""
    if not d["synced"]:
        return (d["state"], d["nsp"])
    return (d["state"], d["sync_index"], tuple(d["starts"]), tuple(d["ends"]), d["nsp"])


def y32_trace(rx, g):
    """y32 of every sample of the capture (a threshold no metric exceeds)."""
    return run_oracle(rx, g, 4.0, trace=True)["y32"]


def in_band_max(y, thr, M, n_end, frac=0.2, span=SC_ITER):
    """Largest number of samples with |y32 - thr| <= frac band(M) among `span` consecutive
    samples of y[:n_end]. frac 0.2: the oracle's fp32 metric is within 0.8 band of the fp64
    one (band is 1.25 x the bound), so such a sample is inside the GPU's band too."""
    m = np.abs(y[:n_end].astype(np.float64) - thr) <= frac * band(M)
    c = np.concatenate([[0], np.cumsum(m)])
    if len(m) <= span:
        return int(c[-1])
    return int((c[span:] - c[:-span]).max())


def cnoise(rng, shape, std):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
            * (std / np.sqrt(2.0))).astype(np.complex64)


def frame(g, seed, snr_db=25.0):
    return ref.synth_frame(g.M, g.cp, g.N, g.nac, g.pid, QAM, seed=seed, frame=0, offset=-1,
                           snr_db=snr_db)[0]


# ------------------------------------------------------------------------------------------
# A. tie pairs
# (geometry, seed of a frame the oracle syncs on, pairs kept at most). N = 4 stops at M 1024,
# and there at two pairs: every candidate costs two oracle runs over the capture.
A_FRAMES = [(Geom(64, 16, 2, 4, 6), 1, 4), (Geom(64, 16, 4, 2, 4), 4, 4),
            (Geom(256, 19, 2, 4, 6), 5, 4), (Geom(256, 19, 4, 2, 4), 4, 4),
            (Geom(1024, 76, 2, 4, 4), 5, 4), (Geom(1024, 76, 4, 2, 3), 4, 2),
            (Geom(2048, 152, 2, 2, 3), 5, 4)]


def tie_pairs(rx, g, tag, family="A", limit=4, base_thr=0.95):
    """For every antenna of a frame the oracle syncs on at base_thr: the sample that starts its
    final run and the one that makes the run exceed cp. Threshold = y32 there (the sample
    compares false) and one fp32 ulp lower (it compares true). A pair is kept when the
    oracle's two outcomes differ. Returns [(case_hi, case_lo)]."""
    base = run_oracle(rx, g, base_thr, trace=True)
    if not base["synced"]:
        return []
    pairs = []
    for s in range(g.N):
        for kind, n in (("start", base["starts"][s]), ("cp", base["starts"][s] + g.cp + 1)):
            if len(pairs) >= limit or n >= base["y32"].shape[1]:
                continue
            y = base["y32"][s, n]
            hi, lo = float(y), ulp_below(y)
            ch = Case("%s_a%d_%s_hi" % (tag, s, kind), family, g, hi, rx, sample=n, antenna=s, y32=float(y))
            cl = Case("%s_a%d_%s_lo" % (tag, s, kind), family, g, lo, rx, sample=n, antenna=s)
            if outcome(ch.want) != outcome(cl.want):
                pairs.append((ch, cl))
    return pairs


A_TAGS = ["A_m%d_n%d" % (g.M, g.N) for g, _, _ in A_FRAMES]


@functools.lru_cache(maxsize=None)
def family_a(tag):
    """[(case_hi, case_lo)] of one frame of A_FRAMES (tag in A_TAGS)."""
    g, seed, limit = A_FRAMES[A_TAGS.index(tag)]
    return tie_pairs(frame(g, seed), g, tag, limit=limit)


# ------------------------------------------------------------------------------------------
# B, C. periodic half-symbols
def periodic_capture(M, N, L, seed, noise_db, noiseless_body=False, amp=0.25):
    """Per antenna: a 3M-sample noise lead, then its own random half-symbol of M/2 samples
    tiled to the end, plus white noise noise_db below the tiled signal (none on the tiled
    part with noiseless_body)."""
    rng = np.random.default_rng(seed)
    lead = 3 * M
    x = np.zeros((N, L), np.complex64)
    for s in range(N):
        half = cnoise(rng, M // 2, amp)
        noise = cnoise(rng, L, amp * 10.0 ** (-noise_db / 20.0))
        if noiseless_body:
            noise[lead:] = 0
        x[s] = noise
        x[s, lead:] += np.tile(half, (L - lead) // (M // 2) + 1)[:L - lead]
    return x


# (geometry, generated length, noise dB below the signal, [(seed, quantile)]). The spread of
# the plateau's y32 falls with the noise power and with M, the band grows with M: 22 dB gives
# a 4096-sample window with 1024 samples within 0.2 band at M 2048 only; M 1024 needs 28 dB
# and M 256 needs 40 dB for the same condition.
B_SPECS = [(Geom(256, 19, 2, 2, 3), 20000, 40.0, [(2, 0.7), (2, 0.8), (3, 0.8), (3, 0.9)]),
           (Geom(1024, 76, 2, 2, 3), 22000, 28.0, [(2, 0.2), (2, 0.5), (1, 0.5), (4, 0.5)]),
           (Geom(2048, 152, 2, 2, 3), 24000, 22.0, [(12, 0.5), (12, 0.7), (7, 0.7), (23, 0.05)])]


@functools.lru_cache(maxsize=None)
def family_b():
    """Hugging cases; meta: in_band (the 0.2-band maximum per 4096 samples before the
    trigger)."""
    out = []
    for g, L, ndb, picks in B_SPECS:
        caps = {}
        for seed, q in picks:
            if seed not in caps:
                rx = periodic_capture(g.M, g.N, L, seed, ndb)
                caps[seed] = (rx, y32_trace(rx, g))
            rx, y = caps[seed]
            thr = float(np.quantile(y[0, 4 * g.M:], q))
            c = Case("B_m%d_s%d_q%02d" % (g.M, seed, round(100 * q)), "B", g, thr, rx)
            n_end = c.want["trigger"] + 1 if c.want["synced"] else L
            c.meta["in_band"] = in_band_max(y[0], thr, g.M, n_end)
            out.append(c)
    return out


# (geometry, generated length, kept length, seed, k): threshold 1 - k 2^-24. The two cases of
# one M share k and length, so they run as one batch.
C_SPECS = [(Geom(64, 16, 2, 2, 3), 9192, 9192, 6, 5),      # syncs
           (Geom(64, 16, 2, 2, 3), 9192, 9192, 1, 5),      # never: > 256 in-band in one item
           (Geom(128, 16, 2, 2, 3), 9000, 9000, 1, 4),     # syncs
           (Geom(256, 19, 2, 2, 3), 20000, 12000, 1, 5),   # syncs
           (Geom(256, 19, 2, 2, 3), 20000, 12000, 2, 5),   # never
           (Geom(1024, 76, 2, 2, 3), 23000, 16000, 2, 0),  # syncs
           (Geom(1024, 76, 2, 2, 3), 23000, 16000, 1, 0)]  # never


@functools.lru_cache(maxsize=None)
def family_c():
    """All-ambiguous cases; meta: in_band (samples of the plateau scanned before the trigger
    with |y32 - thr| <= 0.2 band, per 16384-sample item at most)."""
    out = []
    for g, Lg, L, seed, k in C_SPECS:
        rx = periodic_capture(g.M, g.N, Lg, seed, 22.0, noiseless_body=True)[:, :L]
        thr = 1.0 - k * U24
        c = Case("C_m%d_s%d_k%d" % (g.M, seed, k), "C", g, thr, rx)
        y = y32_trace(rx, g)
        n_end = c.want["trigger"] + 1 if c.want["synced"] else L
        c.meta["in_band"] = in_band_max(y[0], thr, g.M, n_end, span=chunk_len(g.cp))
        c.meta["in_band_iter"] = in_band_max(y[0], thr, g.M, n_end)
        out.append(c)
    return out


# ------------------------------------------------------------------------------------------
# D. energy floor and zero count
D_FRAMES = [(Geom(1024, 76, 2, 4, 4), 5), (Geom(256, 19, 2, 4, 4), 5)]
D_KINDS = ("burst", "zeros", "tiny", "zeros_burst")
BURST_AMP = 3000.0


@functools.lru_cache(maxsize=None)
def family_d():
    """[(plain case, [disturbed cases])] per frame. The capture is a noise lead and the frame;
    the disturbances lie strictly before the frame's S0: a burst of amplitude 3000 over 2M
    samples ending 4000 samples before S0 (same 16384-sample item as S0), 2M exact zeros after
    a nonzero lead, 2M samples scaled by 1e-24 (|x|^2 underflows to 0 in fp32, x != 0), and
    zeros and burst together."""
    out = []
    for g, seed in D_FRAMES:
        M, SL = g.M, g.M + g.cp
        fr_ = frame(g, seed)
        lead_len = max(0, 5 * M + 4096 - SL * (g.N * g.nac + 1))
        rng = np.random.default_rng(100 + M)
        nstd = np.sqrt(0.0625 * 10.0 ** (-25.0 / 10.0))
        rx = np.concatenate([cnoise(rng, (g.N, lead_len), nstd * np.sqrt(2.0)), fr_], axis=1)
        plain = Case("D_m%d_plain" % M, "D", g, 0.95, rx)
        assert plain.want["synced"]
        s0 = min(plain.want["starts"]) - M            # about where S0's body begins
        b1 = s0 - 4000
        b0 = b1 - 2 * M
        assert b0 >= 3 * M and s0 < chunk_len(g.cp)
        cases = []
        for kind in D_KINDS:
            x = rx.copy()
            if kind in ("zeros", "zeros_burst"):
                x[:, M:3 * M] = 0
            if kind == "tiny":
                x[:, M:3 * M] *= np.complex64(1e-24)
                assert np.all(x[:, M:3 * M] != 0)
                assert not np.any(np.abs(x[:, M:3 * M].real) ** 2 + np.abs(x[:, M:3 * M].imag) ** 2)
            if kind in ("burst", "zeros_burst"):
                x[:, b0:b1] = cnoise(rng, (g.N, 2 * M), BURST_AMP)
            cases.append(Case("D_m%d_%s" % (M, kind), "D", g, 0.95, x, s0=s0, burst=(b0, b1)))
        out.append((plain, cases))
    return out


# ------------------------------------------------------------------------------------------
# E. cp edges
E_GEOMS = [(Geom(64, 1, 2, 2, 4), 5), (Geom(64, 14, 2, 2, 4), 5), (Geom(64, 15, 2, 2, 4), 5),
           (Geom(256, 1, 2, 2, 4), 5), (Geom(256, 14, 2, 2, 4), 5), (Geom(256, 15, 2, 2, 4), 5),
           (Geom(256, 128, 2, 2, 4), 5), (Geom(1024, 512, 2, 2, 3), 5)]
E_TIE_GEOMS = [(Geom(256, 14, 2, 2, 4), 5), (Geom(256, 15, 2, 2, 4), 5),
               (Geom(64, 14, 2, 2, 4), 5), (Geom(64, 15, 2, 2, 4), 5)]


@functools.lru_cache(maxsize=None)
def family_e():
    """(plain cases, tie pairs): frames at cp 1, 14, 15 (both sides of the cp + 2 <= 16 split
    of the run condition) and cp = M/2; one tie pair each at cp 14 and 15, M 256 and M 64."""
    plain = [Case("E_m%d_cp%d" % (g.M, g.cp), "E", g, 0.95, frame(g, seed, 30.0))
             for g, seed in E_GEOMS]
    ties = []
    for g, seed in E_TIE_GEOMS:
        ties += tie_pairs(frame(g, seed, 30.0), g, "E_m%d_cp%d" % (g.M, g.cp), "E", limit=1)
    return plain, ties


# ------------------------------------------------------------------------------------------
# F. boundaries
F_GEOM = Geom(256, 19, 2, 2, 4)
F_SHORT, F_ITER = 33000, 2


def f_targets():
    """{name: (trigger position, capture length)}: chunk c = 1 (c K - 1, c K, c K + 1), the
    item's iteration F_ITER (w0 + 4096 it and +-1, w0 = c K - (16384 - K) the item's origin), a
    run that starts in chunk 0 and triggers in chunk 1, and the first phase-2 chunk c1 of a
    capture of 16 chunks."""
    g = F_GEOM
    K = chunk_len(g.cp)
    w0 = K - (SC_SPAN - K)
    t = {}
    for d in (-1, 0, 1):
        t["chunk1%+d" % d] = (K + d, F_SHORT)
        t["iter%d%+d" % (F_ITER, d)] = (w0 + SC_ITER * F_ITER + d, F_SHORT)
    t["straddle"] = (K + g.cp // 2, F_SHORT)
    c1 = first_phase2_chunk(g)
    for d in (-1, 0, 1):
        t["phase2%+d" % d] = (c1 * K + d, 15 * K + 2048)
    return t


def place_frame(fr_, L, pos, seed, nstd):
    rng = np.random.default_rng(seed)
    x = cnoise(rng, (fr_.shape[0], L), nstd)
    x[:, pos:pos + fr_.shape[1]] = fr_
    return x


@functools.lru_cache(maxsize=None)
def family_f(only=None, sc16=False):
    """Boundary cases (all of f_targets(), or the one named `only`); meta: target (where the
    trigger must land). The frame replaces a stretch of a noise capture; its position is found
    by running the oracle, correcting by the miss and running it again. sc16: the capture as a
    16-bit radio delivers it (sc16_round_trip)."""
    g = F_GEOM
    fr_ = frame(g, 5, 30.0)
    nstd = np.sqrt(0.0625 * 10.0 ** (-30.0 / 10.0)) * np.sqrt(2.0)
    out = []
    for i, (name, (target, L)) in enumerate(sorted(f_targets().items())):
        if only is not None and name != only:
            continue
        pos = target - fr_.shape[1] // 3
        for _ in range(4):
            x = place_frame(fr_, L, pos, 200 + i, nstd)
            if sc16:
                x = sc16_round_trip(x, SC16_AMAX)[0]
            c = Case("F_" + name, "F", g, 0.95, x, target=target)
            if not c.want["synced"] or c.want["trigger"] == target:
                break
            pos += target - c.want["trigger"]
        out.append(c)
    return out


# ------------------------------------------------------------------------------------------
# sc16 input: the captures as a 16-bit radio delivers them
SC16_AMAX = 2.0      # full scale; the synthetic frames and periodic captures peak below 1.5


def sc16_round_trip(rx, amax):
    """(widened complex64 capture, int16 wire samples [N][L][2], scale): quantised to the
    sc16 wire format at full scale amax and widened as the kernels read it,
    float(i16) * float32(scale)."""
    scale = np.float32(amax / 32767.0)
    v = np.ascontiguousarray(rx, np.complex64).view(np.float32).reshape(rx.shape + (2,))
    q = np.clip(np.rint(v.astype(np.float64) * (32767.0 / amax)), -32768, 32767).astype(np.int16)
    wide = (q.astype(np.float32) * scale).reshape(rx.shape[0], -1).view(np.complex64)
    return np.ascontiguousarray(wide), q, scale


@functools.lru_cache(maxsize=None)
def family_sc16():
    """One hugging case (M 1024), one tie pair (M 256) and one boundary case (chunk 1's first
    position), all decided on the widened samples: thresholds, ties and the landing position
    are recomputed from them. Returns dict(hug=case, tie=(hi, lo), edge=case); each case's
    meta holds wire (int16 [N][L][2]) and scale."""
    out = {}
    g, L, ndb, picks = B_SPECS[1]
    seed, q = picks[0]
    wide, wire, scale = sc16_round_trip(periodic_capture(g.M, g.N, L, seed, ndb), SC16_AMAX)
    y = y32_trace(wide, g)
    thr = float(np.quantile(y[0, 4 * g.M:], q))
    c = Case("S_hug_m%d" % g.M, "B", g, thr, wide, wire=wire, scale=scale)
    n_end = c.want["trigger"] + 1 if c.want["synced"] else L
    c.meta["in_band"] = in_band_max(y[0], thr, g.M, n_end)
    out["hug"] = c
    g, seed, _ = A_FRAMES[2]
    wide, wire, scale = sc16_round_trip(frame(g, seed), SC16_AMAX)
    hi, lo = tie_pairs(wide, g, "S_tie_m%d" % g.M, limit=1)[0]
    for c in (hi, lo):
        c.meta.update(wire=wire, scale=scale)
    out["tie"] = (hi, lo)
    c = family_f("chunk1+0", True)[0]
    wide, wire, scale = sc16_round_trip(c.rx, SC16_AMAX)
    assert np.array_equal(wide, c.rx)         # already on the sc16 grid
    c.meta.update(wire=wire, scale=scale)
    out["edge"] = c
    return out


# ------------------------------------------------------------------------------------------
# two frames per capture
G_GEOM = Geom(256, 19, 2, 2, 4)
G_SEEDS = [(5, 6), (9, 4)]


def stream_outcome(recs):
    return [(r["origin"], r["state"], r["num_samples_processed"], r.get("sync_index"),
             tuple(r.get("plateau_start", ())), tuple(r.get("plateau_end", ()))) for r in recs]


def stream_oracle(rx, g, thr):
    return ref.stream_ref(rx, g.M, g.cp, g.N, g.nac, pid_max=g.pid, threshold=float(thr),
                          detector=detector(g.N), search_mode=1, qam=QAM)


@functools.lru_cache(maxsize=None)
def family_streams():
    """[(rx, thr_hi, thr_lo, records_hi, records_lo)]: captures of two back-to-back frames; the
    threshold is y32 of the sample that starts a run of the second frame (seen from the
    second framesync's origin) and one ulp lower, on the first antenna where the oracle's
    records (ref.stream_ref) differ between the two."""
    g = G_GEOM
    out = []
    for sa, sb in G_SEEDS:
        rx = np.concatenate([frame(g, sa, 30.0), frame(g, sb, 30.0)], axis=1)
        base = stream_oracle(rx, g, 0.95)
        assert len(base) >= 2 and base[1]["state"] == ref.STATE_MIMO
        r1 = base[1]["origin"]
        second = run_oracle(rx[:, r1:], g, 0.95, trace=True)
        for s in range(g.N):
            y = second["y32"][s, second["starts"][s]]
            hi, lo = float(y), ulp_below(y)
            rh, rl = stream_oracle(rx, g, hi), stream_oracle(rx, g, lo)
            if stream_outcome(rh) != stream_outcome(rl):
                out.append((rx, hi, lo, rh, rl))
                break
    return out


# ------------------------------------------------------------------------------------------
def batches(cases):
    """Cases of one geometry, threshold and length, batched together: [(geom, thr, [cases])]
    in first-seen order."""
    groups = {}
    for c in cases:
        groups.setdefault((c.geom, c.thr, c.rx.shape[1]), []).append(c)
    return [(k[0], k[1], v) for k, v in groups.items()]
