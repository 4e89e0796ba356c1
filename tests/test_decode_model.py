"""CPU tests of tests/decode_support.py against the C oracle: the float64 decode reference and
its per-element unit are pinned against an independent implementation (the oracle's own
float32 decode stays within DEC_UNITS / 4 of the reference, which is the measurement DEC_UNITS
rests on), the index rules pass on the oracle's own indices, and select_fir keeps the oracle
at STATE_MIMO while multiplying the pivot orders of the weight solve. No GPU."""
import numpy as np
import pytest

import decode_support as ds
from oracle import ref

DETS = {"zf2": ref.DET_ZF2, "zf": ref.DET_ZF, "mmse": ref.DET_MMSE, "siso": ref.DET_SISO}

# M, cp, N, nac, pid, qam, detector, allocation, search_mode (1: the Parseval search, above
# M = 1024 where the brute-force search takes too long), seed
GEOMS = [
    (64, 16, 1, 4, 10, 4, "zf", None, 0, 11),
    (64, 16, 2, 4, 10, 16, "zf2", "liquid", 0, 12),
    (64, 16, 2, 4, 10, 4, "siso", None, 0, 13),
    (128, 16, 4, 2, 8, 64, "mmse", None, 0, 14),
    (256, 32, 8, 2, 6, 256, "mmse", None, 0, 15),
    (256, 32, 2, 4, 10, 4, "zf2", "all", 0, 16),
    (512, 40, 4, 2, 8, 16, "zf", "liquid", 0, 17),
    (1024, 76, 2, 2, 12, 16, "zf2", "liquid", 0, 18),
    (1024, 76, 4, 2, 6, 64, "mmse", None, 0, 119),
    (2048, 152, 2, 2, 6, 64, "zf", None, 1, 20),
]
IDS = ["m%d_n%d_%s_%s" % (g[0], g[2], g[6], g[7] or "default") for g in GEOMS]


def _sct(M, kind):
    if kind == "liquid":
        return ref.liquid_sctype(M)
    return np.full(M, 2, np.uint8) if kind == "all" else ref.default_sctype(M)


_RUNS = {}


def _oracle_run(geom):
    """One oracle receive per geometry, shared by the tests below and left unchanged."""
    if geom not in _RUNS:
        M, cp, N, nac, pid, qam, det, sct, mode, seed = geom
        p = _sct(M, sct)
        siso = (1, 0) if det == "siso" else None
        rx, tx_idx, _ = ref.synth_frame(M, cp, N, nac, pid, qam, seed, snr_db=30.0, p=p)
        o = ref.FrameSyncRef(M, cp, N, nac, pid_max=pid, detector=DETS[det], p=p,
                             search_mode=mode, siso_tx=siso[0] if siso else 0,
                             siso_rx=siso[1] if siso else 0)
        assert o.execute(rx) == ref.STATE_MIMO
        syms = o.symbols()[:pid]
        y64, u = ds.decode_reference(rx, o.get_W(), o.get_gain(), o.get_corr()[0],
                                     o.get_sync_index(), p, cp, nac, len(syms), siso=siso,
                                     G=o.get_G())
        _RUNS[geom] = dict(syms=syms, y64=y64, u=u, qam=qam, tx_idx=tx_idx, siso=siso)
    return _RUNS[geom]


@pytest.mark.parametrize("geom", GEOMS, ids=IDS)
def test_oracle_decode_within_a_quarter_of_dec_units(geom):
    """The oracle's symbols() through the reference with the oracle's own W, gain, corr indices
    and sync index: max e <= DEC_UNITS / 4 (the per-geometry values are in decode_support's
    docstring; run with -s to print them)."""
    r = _oracle_run(geom)
    assert r["syms"].shape == r["y64"].shape and r["syms"].shape[0] == geom[4]
    e = ds.normalised_error(r["syms"], r["y64"], r["u"])
    print("oracle max e %.2f (mean %.2f)" % (e.max(), e.mean()))
    assert e.max() <= ds.DEC_UNITS / 4, ds.describe_errors(e, ds.DEC_UNITS / 4)
    # the unit is no slack: the oracle's float32 error is at least a third of a unit somewhere
    assert e.max() >= 1.0 / 3


def test_reference_equals_the_numpy_model():
    """decode_reference on the numpy model's own float64 W, gain and corr indices gives the
    model's symbols to float64 rounding (the model is the written definition)."""
    from oracle import codes, numpy_model as nm
    M, cp, N, nac, pid, qam = 64, 16, 2, 4, 10, 16
    p = ref.liquid_sctype(M)
    rx, _, _ = ref.synth_frame(M, cp, N, nac, pid, qam, 12, snr_db=30.0, p=p)
    s0b, s1b = ref.code_bits(M, N, nac, codes.s1_polynomials(N))
    d = nm.receive(rx, M, cp, N, nac, pid, s0b, s1b, p=p, detector="zf2")
    y64, u = ds.decode_reference(rx, d["W"], d["gain"], d["corr_idx"], d["sync_index"], p, cp,
                                 nac, d["symbols"].shape[0])
    assert np.abs(y64 - d["symbols"]).max() <= 1e-12 * np.abs(d["symbols"]).max()
    assert u.min() > 0


def test_demap64_equals_the_oracle_rule():
    rng = np.random.default_rng(5)
    for qam in (4, 16, 64, 256):
        y = (rng.uniform(-1.6, 1.6, 400) + 1j * rng.uniform(-1.6, 1.6, 400)).astype(np.complex64)
        got = ds.demap64(y, qam)
        far = ds.boundary_distance(y, qam) > 1e-5
        want = np.array([ref.qam_demap(complex(v), qam) for v in y])
        assert np.array_equal(got[far], want[far]) and far.sum() > 390, qam
    # the boundary distance: level boundaries at v = 1 .. L-1, none beyond the outer levels
    s = np.sqrt(2.0 * 15 / 3.0)
    for v, d in ((1.0, 0.0), (1.25, 0.25), (2.5, 0.5), (-3.0, 4.0), (7.5, 4.5)):
        y = np.array([(2 * v - 4) / s + 1j * (2 * 2.5 - 4) / s])
        assert abs(ds.boundary_distance(y, 16)[0] - min(d, 0.5)) < 1e-12, v


def test_index_rules_pass_on_the_oracle_indices():
    """The index check of the GPU element tests on the oracle's own hard decisions of its own
    symbols, every geometry in one pool: nothing unexcused, at most 0.1 % excused."""
    total = excused = 0
    for geom in GEOMS:
        r = _oracle_run(geom)
        dec, _, _, _ = ref.demap_evm(r["syms"], r["qam"], None)
        chk = ds.ElementCheck(r["qam"], ds.DEC_UNITS)
        rows = slice(None) if r["siso"] is None else [r["siso"][1]]
        chk.frame(r["y64"][:, rows], r["u"][:, rows], y=r["syms"][:, rows],
                  idx=dec.transpose(1, 0, 2)[:, rows], label=str(geom))
        total += chk.total
        excused += chk.excused
    print("excused %d of %d" % (excused, total))
    assert excused <= ds.MAX_EXCUSED * total


def test_index_rules_catch_a_wrong_index():
    r = _oracle_run(GEOMS[3])
    dec = ref.demap_evm(r["syms"], r["qam"], None)[0].transpose(1, 0, 2).copy()
    far = np.argmax(ds.boundary_distance(r["y64"], r["qam"]))
    dec.reshape(-1)[far] ^= 1
    with pytest.raises(AssertionError, match="indices differ"):
        ds.ElementCheck(r["qam"]).frame(r["y64"], r["u"], y=r["syms"], idx=dec)
    y = r["syms"].copy()
    y.reshape(-1)[far] *= np.complex64(1 + 2e-5)         # ~170 roundings on one element
    with pytest.raises(AssertionError, match="worst e"):
        ds.ElementCheck(r["qam"]).frame(r["y64"], r["u"], y=y)


# floors the GPU weight tests assert (tests/test_gpu_decode_elements.py) on a selective channel
PIVOT_FLOOR = {8: 8, 4: 3}


@pytest.mark.parametrize("M,cp,N,nac,seed", [(256, 32, 8, 2, 15), (512, 40, 4, 2, 21)],
                         ids=["8x8_m256", "4x4_m512"])
def test_select_fir_keeps_sync_and_varies_the_pivots(M, cp, N, nac, seed):
    """select_fir (3 taps, seeds 7 + f) on a batch of three synthetic captures, as the GPU
    weight tests build theirs: the oracle still reaches STATE_MIMO, cond(G) stays far below the
    1e6 those tests skip at, and the float64 pivot-sequence count over the batch's carriers
    rises from the flat channel's handful to at least the floors those tests assert."""
    pid, qam, F = 4, 16, 3
    seqs = {(k, d): set() for k in ("flat", "fir") for d in ("zf", "mmse")}
    for f in range(F):
        rx, _, _ = ref.synth_frame(M, cp, N, nac, pid, qam, seed, frame=f, snr_db=30.0)
        for name, cap in (("flat", rx), ("fir", ds.select_fir(rx, 3, 7 + f))):
            o = ref.FrameSyncRef(M, cp, N, nac, pid_max=pid, detector=ref.DET_MMSE)
            assert o.execute(cap) == ref.STATE_MIMO, (name, f)
            G, s2 = o.get_G(), o.get_noise_var()
            assert np.linalg.cond(G.astype(np.complex128)).max() < 1e4
            for d in ("zf", "mmse"):
                seqs[name, d] |= {tuple(r) for r in ds.pivot_sequences(ds.solve_matrix(G, s2, d))}
    counts = {k: len(v) for k, v in seqs.items()}
    print(counts)
    for d in ("zf", "mmse"):
        assert counts["fir", d] >= PIVOT_FLOOR[N], counts
        assert counts["fir", d] > counts["flat", d], counts


def test_weights_reference_and_pivots_on_known_matrices():
    rng = np.random.default_rng(9)
    G = rng.standard_normal((50, 4, 4)) + 1j * rng.standard_normal((50, 4, 4))
    W, g, cond = ds.weights_reference(G, 0.0, "zf")
    assert np.abs(W @ G - np.eye(4)).max() < 1e-10 and np.all(g == 1)
    Wm, _, _ = ds.weights_reference(G, 1e-12, "mmse")
    assert np.abs(Wm - W).max() < 1e-6 * np.abs(W).max()
    W2, g2, _ = ds.weights_reference(G[:, :2, :2], 0.0, "zf2")
    assert np.abs(W2 * g2[:, None, None] @ G[:, :2, :2] - np.eye(2)).max() < 1e-10
    # a permutation matrix pivots on its own permutation
    P = np.eye(4)[[2, 0, 3, 1]][None].astype(np.complex128)
    assert ds.pivot_sequences(P)[0].tolist() == [1, 3, 3, 3]
    assert ds.count_pivot_sequences(np.concatenate([P, np.eye(4)[None]])) == 2
