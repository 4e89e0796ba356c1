"""CPU tests of the channel code's written definition (rub_mimo_amd/fec.py) and of the host-only
mimo_fec_* calls (create, geometry, encode, destroy): the model decodes its own encoding, with
and without hard errors below half the free distance, the geometry formulas, the library's
encoder against the model's under identity, random and sparse permutations, and the arguments
mimo_fec_create refuses. No GPU calls."""
import ctypes as C

import numpy as np
import pytest

from rub_mimo_amd import _lib, fec

RATES = [fec.R12, fec.R23, fec.R34]
RATE_IDS = ["r12", "r23", "r34"]
N_FLIP = {fec.R12: 4, fec.R23: 2, fec.R34: 2}        # < d_free / 2 (d_free 10, 6, 5)


def _llr_of(row, mag):
    """Hard LLRs of a coded row: +mag for bit 0, -mag for bit 1."""
    return (mag * (1 - 2 * row.astype(np.int64))).astype(np.int8)


def _create_rc(rate, n_c, perm=None):
    p = None if perm is None else np.ascontiguousarray(perm, np.uint16)
    cfg = _lib.FecConfig(rate, n_c, None if p is None else p.ctypes.data)
    h = C.c_void_p()
    rc = _lib.lib().mimo_fec_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        _lib.lib().mimo_fec_destroy(h)
    return rc


@pytest.mark.parametrize("rate", RATES, ids=RATE_IDS)
@pytest.mark.parametrize("n_c", [100, 128, 12288])
def test_model_decodes_its_own_encoding_with_and_without_flips(rate, n_c):
    """Row 0 clean, rows 1.. with n_flip hard errors at used positions, all at magnitude m: the
    info bits come back exactly and the final metric is m n_tx - 2 m n_flip."""
    rng = np.random.default_rng(100 * rate + n_c)
    T, n_info, ntx = fec.geometry(rate, n_c)
    m, rows = 20, 6
    info = rng.integers(0, 2, (rows, n_info)).astype(np.uint8)
    coded = fec.encode(rate, n_c, info)
    llr = _llr_of(coded, m)
    llr[:, ntx:] = rng.integers(-128, 128, (rows, n_c - ntx))       # unused: ignored
    flips = np.zeros(rows, np.int64)
    for r in range(1, rows):
        at = rng.choice(ntx, N_FLIP[rate], replace=False)
        llr[r, at] = -llr[r, at]
        flips[r] = N_FLIP[rate]
    bits, metric = fec.viterbi(*fec.depuncture(rate, n_c, llr))
    assert np.array_equal(bits, info)
    assert np.array_equal(metric, m * ntx - 2 * m * flips)
    packed, met32 = fec.decode(rate, n_c, llr)
    assert packed.shape == (rows, fec.min_pitch(n_info)) and met32.dtype == np.int32
    assert np.array_equal(np.unpackbits(packed, axis=1)[:, :n_info], info)
    assert not np.unpackbits(packed, axis=1)[:, n_info:].any()


def test_model_burst_of_adjacent_flips_at_rate_half():
    """Four adjacent hard errors at rate 1/2 (weight 4 < d_free / 2) anywhere in the row."""
    n_c = 128
    T, n_info, ntx = fec.geometry(fec.R12, n_c)
    rng = np.random.default_rng(5)
    info = rng.integers(0, 2, (ntx - 3, n_info)).astype(np.uint8)
    llr = _llr_of(fec.encode(fec.R12, n_c, info), 7)
    for r in range(ntx - 3):
        llr[r, r:r + 4] = -llr[r, r:r + 4]
    bits, metric = fec.viterbi(*fec.depuncture(fec.R12, n_c, llr))
    assert np.array_equal(bits, info) and np.all(metric == 7 * ntx - 2 * 7 * 4)


def test_all_zero_and_extreme_rows():
    """An all-zero row gives zero bits and metric 0 (every tie keeps p0); all +127 is the zero
    codeword; all -128 is decoded with -128 meaning -128."""
    for rate in RATES:
        n_c = 100
        T, n_info, ntx = fec.geometry(rate, n_c)
        llr = np.zeros((3, n_c), np.int8)
        llr[1] = 127
        llr[2] = -128
        bits, metric = fec.viterbi(*fec.depuncture(rate, n_c, llr))
        assert not bits[:2].any() and metric[0] == 0 and metric[1] == 127 * ntx
        # the all-ones input is no codeword (the tail is zero): its metric is below 128 n_tx
        # and at least that of the zero codeword
        assert -128 * ntx <= metric[2] < 128 * ntx


def test_tie_rule_keeps_the_predecessor_with_oldest_bit_zero():
    """With L_A = L_B = 0 at every step every path ties: the survivor is p0 everywhere."""
    LA = np.zeros((1, 20), np.int64)
    bits, metric = fec.viterbi(LA, LA)
    assert not bits.any() and metric[0] == 0
    # one informative step in the middle: still a unique answer, reproducible
    LA2 = LA.copy()
    LA2[0, 9] = -5
    b1, m1 = fec.viterbi(LA2, LA)
    b2, m2 = fec.viterbi(LA2, LA)
    assert np.array_equal(b1, b2) and m1[0] == m2[0] == 5


def test_geometry_values():
    for T in range(0, 200):
        assert fec.n_tx(fec.R12, T) == 2 * T
        assert fec.n_tx(fec.R23, T) == T // 2 * 3 + (T % 2) * 2
        assert fec.n_tx(fec.R34, T) == T // 3 * 4 + (0, 2, 3)[T % 3]
    assert [fec.geometry(r, 100)[0] for r in RATES] == [50, 66, 75]
    assert fec.geometry(fec.R34, 98) == (73, 67, 98)
    assert fec.geometry(fec.R23, 100) == (66, 60, 99)
    assert fec.geometry(fec.R12, 14) == (7, 1, 14)
    assert fec.geometry(fec.R12, 12288) == (6144, 6138, 12288)
    assert fec.geometry(fec.R34, 32768) == (24576, 24570, 32768)
    for rate in RATES:
        for n_c in (14, 15, 98, 99, 100, 101, 126, 128, 130, 12288, 32768):
            T, n_info, ntx = fec.geometry(rate, n_c)
            assert ntx <= n_c < fec.n_tx(rate, T + 1) and n_info == T - 6
            f = fec.Fec(rate, n_c)
            assert f.geometry() == (T, n_info, ntx)
    kA, kB = fec.coded_index(fec.R34, 6)
    assert kA.tolist() == [0, 2, -1, 4, 6, -1] and kB.tolist() == [1, -1, 3, 5, -1, 7]
    kA, kB = fec.coded_index(fec.R23, 4)
    assert kA.tolist() == [0, 2, 3, 5] and kB.tolist() == [1, -1, 4, -1]


def test_encoder_generators():
    """The impulse response is the two generators, 133 and 171 octal, MSB first."""
    info = np.zeros(10, np.uint8)
    info[0] = 1
    row = fec.encode(fec.R12, 32, info)
    assert "".join(map(str, row[0:14:2])) == format(0o133, "07b")
    assert "".join(map(str, row[1:14:2])) == format(0o171, "07b")


def _perms(rng, n_c, ntx):
    sparse = np.sort(rng.choice(n_c, ntx, replace=False))
    return {"identity": None, "random": rng.permutation(n_c)[:ntx], "sparse": sparse}


@pytest.mark.parametrize("rate", RATES, ids=RATE_IDS)
@pytest.mark.parametrize("n_c", [14, 100, 131, 12288])
def test_library_encoder_equals_the_model(rate, n_c):
    rng = np.random.default_rng(7 * n_c + rate)
    T, n_info, ntx = fec.geometry(rate, n_c)
    for name, perm in _perms(rng, n_c, ntx).items():
        f = fec.Fec(rate, n_c, perm)
        for _ in range(3):
            info = rng.integers(0, 2, n_info).astype(np.uint8)
            got = f.encode(info)
            want = fec.encode(rate, n_c, info, perm)
            assert np.array_equal(got, want), name
        # and the model decodes through the same permutation
        llr = _llr_of(want[None, :], 3)
        bits, _ = fec.viterbi(*fec.depuncture(rate, n_c, llr, perm))
        assert np.array_equal(bits[0], info), name


def test_qam_indices_put_value_i_at_bit_i_from_the_msb():
    row = np.array([1, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 1], np.uint8)
    assert fec.qam_indices(row, 4).tolist() == [8, 7, 1]
    assert fec.qam_indices(row, 6).tolist() == [33, 49]


def test_create_refuses_bad_arguments():
    assert _create_rc(fec.R12, 14) == 0                 # n_info = 1
    assert fec.Fec(fec.R12, 14).n_info == 1
    assert _create_rc(fec.R12, 13) == -1                # T = 6 < 7
    assert _create_rc(fec.R34, 9) == -1                 # T = 6 at rate 3/4 (n_tx(7) = 10)
    assert _create_rc(fec.R12, 32768) == 0
    assert _create_rc(fec.R12, 32769) == -1
    assert _create_rc(3, 100) == -1                     # no such rate
    ntx = fec.geometry(fec.R23, 100)[2]
    good = np.arange(ntx)
    assert _create_rc(fec.R23, 100, good) == 0
    dup = good.copy()
    dup[5] = dup[70]
    assert _create_rc(fec.R23, 100, dup) == -1
    assert b"distinct" in _lib.lib().mimo_last_error()
    far = good.copy()
    far[3] = 100
    assert _create_rc(fec.R23, 100, far) == -1
    assert b"range" in _lib.lib().mimo_last_error()
    top = good.copy()
    top[3] = 99                                         # the unused position: allowed
    assert _create_rc(fec.R23, 100, top) == 0
    assert _lib.lib().mimo_fec_create(None, None) == -1
    for bad in (13, 32769):
        with pytest.raises(ValueError):
            fec.geometry(fec.R12, bad)
    with pytest.raises(ValueError):
        fec.geometry(3, 100)
    with pytest.raises(ValueError):
        fec.positions(fec.R23, 100, dup)
    with pytest.raises(_lib.MimoError):
        fec.Fec(fec.R12, 13)
