"""CPU checks of the close-call S&C captures (tests/sc_edge_support.py), with the oracle alone:
every family is what the GPU tests (test_gpu_sc_edges.py) rely on it being. A capture that stops
being adversarial -- a tie pair whose two sides agree, a hugging capture that no longer fills
the exact kernel's lists, a boundary trigger that moved -- fails here, not silently there."""
import numpy as np
import pytest

import sc_edge_support as S
from oracle import ref


def test_band_restates_sc_band():
    """band(M) is engine_stages.cpp sc_band(M): 1.25 x the first-order bound of DESIGN.md
    section 2, about 5.2e-4 at M 2048."""
    u = 2.0 ** -24
    for M in (64, 256, 1024, 2048):
        y = 1.0
        bound = 2 * np.sqrt(2) * (M / 2 + 2) * u * np.sqrt(y) + 2 * (M + 1) * u * y + 4 * u * y
        assert abs(S.band(M) - 1.25 * bound) <= 1e-18
    assert 5.1e-4 < S.band(2048) < 5.3e-4
    assert S.chunk_len(19) == 16352 and S.chunk_len(14) == 16368 and S.chunk_len(15) == 16352


# pairs the frames of family A yield today; the sum is the "at least 8" of the family
A_PAIRS = {"A_m64_n2": 1, "A_m64_n4": 1, "A_m256_n2": 2, "A_m256_n4": 4, "A_m1024_n2": 2,
           "A_m1024_n4": 2, "A_m2048_n2": 2}


@pytest.mark.parametrize("tag", S.A_TAGS)
def test_tie_pairs_differ(tag):
    """Family A: at least 8 pairs over the frames, at least one per M in {64, 256, 1024, 2048}
    and at both stream counts. The two sides of a pair are one fp32 ulp apart, the upper one
    equal to y32 of the deciding sample, and the oracle's outcomes differ."""
    assert sum(A_PAIRS.values()) >= 8 and set(A_PAIRS) == set(S.A_TAGS)
    assert {int(t.split("_")[1][1:]) for t, n in A_PAIRS.items() if n} == {64, 256, 1024, 2048}
    assert {int(t.split("_")[2][1:]) for t, n in A_PAIRS.items() if n} == {2, 4}
    pairs = S.family_a(tag)
    assert len(pairs) >= A_PAIRS[tag]
    for hi, lo in pairs:
        assert np.float32(hi.thr) == hi.thr and np.float32(lo.thr) == lo.thr
        assert np.nextafter(np.float32(lo.thr), np.float32(2)) == np.float32(hi.thr)
        assert hi.meta["y32"] == hi.thr
        assert S.outcome(hi.want) != S.outcome(lo.want), hi.name
        assert lo.want["synced"], lo.name


def test_hugging_captures_fill_the_lists():
    """Family B: before the oracle's trigger some 4096 consecutive samples hold at least 1024
    with |y32 - thr| <= 0.2 band(M) (more than kLocAmb = 128 in-band samples per iteration of
    the exact kernel whatever the alignment); per M one case syncs; one case overall scans the
    whole capture. The noise is 22 dB below the signal at M 2048; at M 1024 (28 dB) and M 256
    (40 dB) it is lower, because at 22 dB no threshold meets the in-band condition there (the
    band shrinks with M while the spread of y32 grows)."""
    cases = S.family_b()
    assert {c.geom.M for c in cases} == {256, 1024, 2048}
    for M in (256, 1024, 2048):
        mine = [c for c in cases if c.geom.M == M]
        assert 3 <= len(mine) <= 4
        assert any(c.want["synced"] for c in mine), M
    for c in cases:
        assert c.meta["in_band"] >= 1024, (c.name, c.meta["in_band"])
        assert c.rx.shape[1] <= 30000
    assert any(not c.want["synced"] and c.want["nsp"] == c.rx.shape[1] for c in cases)


def test_all_ambiguous_captures():
    """Family C: on the noiseless periodic part y32 is within a few ulps of 1 and the threshold
    is 1 - k 2^-24, so every scanned sample there is inside the band. One M 64 and one M 128
    case sync; one M 64 case scans more than 256 (kScAmbMax) in-band samples in one item and
    never syncs; M 256 and M 1024 have one case each that never syncs with more than 128
    (kLocAmb) in-band samples per 4096 and one that syncs."""
    cases = S.family_c()
    by = {}
    for c in cases:
        by.setdefault(c.geom.M, []).append(c)
        assert 0 <= round((1.0 - c.thr) / S.U24) <= 8
        assert c.rx.shape[1] <= 2 * S.chunk_len(c.geom.cp)
        y = S.y32_trace(c.rx, c.geom)[0, 4 * c.geom.M:]
        assert np.all(np.abs(y.astype(np.float64) - c.thr) <= 0.2 * S.band(c.geom.M)), c.name
    assert any(c.want["synced"] for c in by[64]) and any(c.want["synced"] for c in by[128])
    assert any(not c.want["synced"] and c.meta["in_band"] > 256 for c in by[64])
    for M in (256, 1024):
        assert any(not c.want["synced"] and c.meta["in_band_iter"] > 1024 for c in by[M]), M
        assert any(c.want["synced"] for c in by[M]), M


def test_disturbed_leads_leave_the_oracle_result_unchanged():
    """Family D: every disturbance ends before the frame's S0 and gives the oracle result of
    the undisturbed capture; the burst lies in S0's 16384-sample item and puts S0's window
    energy below 1e-6 of the energy streamed since the item began."""
    fams = S.family_d()
    assert {p.geom.M for p, _ in fams} == {1024, 256}
    for plain, cases in fams:
        assert plain.want["state"] == ref.STATE_MIMO
        assert [c.name.split("_", 2)[2] for c in cases] == list(S.D_KINDS)
        M = plain.geom.M
        for c in cases:
            assert S.outcome(c.want) == S.outcome(plain.want), c.name
            b0, b1 = c.meta["burst"]
            assert 3 * M <= b0 < b1 <= c.meta["s0"] - M and c.meta["s0"] < S.chunk_len(c.geom.cp)
            changed = np.flatnonzero(np.any(c.rx != plain.rx, axis=0))
            assert changed.max() < c.meta["s0"] - M and changed.min() >= M
            if "burst" in c.name:
                x = c.rx[0].astype(np.complex128)
                e_burst = np.sum(np.abs(x[b0:b1]) ** 2)
                s = plain.want["starts"][0]
                e_win = np.sum(np.abs(x[s - M + 1:s + 1]) ** 2)
                assert e_win < 1e-6 * e_burst / 4


def test_cp_edge_frames_sync():
    """Family E: frames at cp 1, 14, 15 (M 64 and 256) and cp = M/2 (M 256 and 1024) sync in the
    oracle, and each cp 14 / cp 15 geometry has a tie pair whose sides differ."""
    plain, ties = S.family_e()
    assert {(c.geom.M, c.geom.cp) for c in plain} == {
        (64, 1), (64, 14), (64, 15), (256, 1), (256, 14), (256, 15), (256, 128), (1024, 512)}
    for c in plain:
        assert c.want["state"] == ref.STATE_MIMO, c.name
        assert all(e - s > c.geom.cp for s, e in zip(c.want["starts"], c.want["ends"]))
    assert {(hi.geom.M, hi.geom.cp) for hi, _ in ties} >= {(256, 14), (256, 15)}
    for hi, lo in ties:
        assert S.outcome(hi.want) != S.outcome(lo.want), hi.name


def test_boundary_triggers_land():
    """Family F: the oracle's trigger is exactly on each target -- chunk 1's first position and
    its neighbours, an inner iteration's first position and its neighbours, a run that begins
    in chunk 0 and fires in chunk 1, and the same three positions of the first phase-2 chunk in
    captures of 16 chunks."""
    cases = S.family_f()
    g = S.F_GEOM
    K = S.chunk_len(g.cp)
    c1 = S.first_phase2_chunk(g)
    want = {K - 1, K, K + 1, c1 * K - 1, c1 * K, c1 * K + 1}
    w0 = K - (S.SC_SPAN - K)
    want |= {w0 + S.SC_ITER * S.F_ITER + d for d in (-1, 0, 1)}
    assert want <= {c.meta["target"] for c in cases}
    for c in cases:
        assert c.want["state"] == ref.STATE_MIMO, c.name
        assert c.want["trigger"] == c.meta["target"], (c.name, c.want["trigger"])
        if c.name.startswith("F_phase2"):
            assert (c.rx.shape[1] + K - 1) // K >= 16 and c1 >= 2
    s = [c for c in cases if c.name == "F_straddle"][0]
    assert all(st < K for st in s.want["starts"]) and s.want["trigger"] >= K


def test_sc16_variants_stay_adversarial():
    """The sc16 cases are decided on the widened samples: the hugging case still holds 1024
    in-band samples in 4096 and syncs, the tie pair's sides differ, the boundary trigger is on
    chunk 1's first position, and the wire samples widen to exactly the capture."""
    f = S.family_sc16()
    assert f["hug"].meta["in_band"] >= 1024
    hi, lo = f["tie"]
    assert S.outcome(hi.want) != S.outcome(lo.want)
    assert f["edge"].want["trigger"] == f["edge"].meta["target"] == S.chunk_len(S.F_GEOM.cp)
    for c in (f["hug"], hi, lo, f["edge"]):
        wide = (c.meta["wire"].astype(np.float32) * c.meta["scale"]).reshape(c.rx.shape[0], -1)
        assert np.array_equal(wide.view(np.complex64), c.rx)
        assert np.abs(c.meta["wire"]).max() < 32767       # nothing clipped


def test_two_frame_captures_have_a_tie_in_the_second_frame():
    """Two captures of two back-to-back frames: both frames reach STATE_MIMO on both sides of
    the ulp, and the records differ between the sides in the second frame."""
    fam = S.family_streams()
    assert len(fam) == 2
    for rx, hi, lo, rh, rl in fam:
        assert np.nextafter(np.float32(lo), np.float32(2)) == np.float32(hi)
        for recs in (rh, rl):
            assert len(recs) >= 2 and all(r["state"] == ref.STATE_MIMO for r in recs[:2])
        assert S.stream_outcome(rh[:1]) == S.stream_outcome(rl[:1])
        assert S.stream_outcome(rh[1:2]) != S.stream_outcome(rl[1:2])
