"""CPU checks of the coded transmit path's conventions and argument handling: the bit mapper
(fec.rows_to_idx / idx_to_rows) against the demapper's written definition (soft.llr_delta), the
info-bit packing against fec.decode's format, and every MIMO_ERR_ARG case of
mimo_fec_encode_rows and mimo_synth_frames_payload, which are refused before any HIP call and so
on a machine without a GPU too. Integer conventions: no tolerances."""
import ctypes as C

import numpy as np
import pytest

from rub_mimo_amd import _lib, fec, soft
from rub_mimo_amd.receiver import Synthesizer, SynthParams

ORDERS = [1, 2, 3, 4]


@pytest.mark.parametrize("b", ORDERS)
def test_mapper_and_its_inverse(b):
    """idx_to_rows and rows_to_idx are inverses, on every index and on random rows; row position
    i of a carrier is bit 2b - 1 - i of its index."""
    idx = np.arange(1 << (2 * b), dtype=np.uint8)[None]
    rows = fec.idx_to_rows(idx, b)
    assert rows.shape == (1, (1 << (2 * b)) * 2 * b) and rows.dtype == np.uint8
    assert np.array_equal(fec.rows_to_idx(rows, b), idx)
    per = rows.reshape(-1, 2 * b)
    for i in range(2 * b):
        assert np.array_equal(per[:, i], (idx[0] >> (2 * b - 1 - i)) & 1)
    rng = np.random.default_rng(b)
    r = rng.integers(0, 2, (3, 5, 24 * b)).astype(np.uint8)
    assert np.array_equal(fec.idx_to_rows(fec.rows_to_idx(r, b), b), r)
    assert np.array_equal(fec.rows_to_idx(r, b), fec.qam_indices(r, 2 * b))
    with pytest.raises(ValueError):
        fec.rows_to_idx(np.zeros(2 * b + 1, np.uint8), b)
    with pytest.raises(ValueError):
        fec.rows_to_idx(np.zeros(20, np.uint8), 5)


@pytest.mark.parametrize("b", ORDERS)
def test_mapper_is_the_demappers_inverse(b):
    """For every index of the order: at its noiseless constellation point the signs of
    soft.llr_delta (negative = bit 1) are idx_to_rows(idx), and the point is the one the
    index's Gray-coded halves name."""
    order = 1 << (2 * b)
    idx = np.arange(order)
    pts = fec.idx_to_points(idx, b)
    lv = soft.qam_levels(order)
    gray = np.arange(1 << b) ^ (np.arange(1 << b) >> 1)
    for i in idx:
        assert gray[np.argmin(np.abs(lv - pts[i].real))] == i >> b
        assert gray[np.argmin(np.abs(lv - pts[i].imag))] == i & ((1 << b) - 1)
    d = soft.llr_delta(pts, order)
    assert d.shape == (order, 2 * b) and np.all(d != 0)
    assert np.array_equal((d < 0).astype(np.uint8).reshape(1, -1), fec.idx_to_rows(idx[None], b))
    assert np.array_equal(fec.idx_to_points(idx | 0x100, b), pts)          # high bits dropped


@pytest.mark.parametrize("rate", fec.RATES)
@pytest.mark.parametrize("n_c", [14, 17, 128, 1030])
def test_packing_round_trips_through_the_decoders_format(rate, n_c):
    """unpack_bits inverts pack_bits at any pitch and drops what lies past n_info; noiseless
    LLRs of an encoded row decode (fec.decode) to pack_bits of the info; encode_rows reads
    exactly that format and ignores the padding."""
    T, n_info, ntx = fec.geometry(rate, n_c)
    rng = np.random.default_rng(n_c + rate)
    info = rng.integers(0, 2, (5, n_info)).astype(np.uint8)
    for pitch in (None, fec.min_pitch(n_info) + 8):
        packed = fec.pack_bits(info, pitch)
        assert np.array_equal(fec.unpack_bits(packed, n_info), info)
        dirty = np.unpackbits(packed, axis=1)
        dirty[:, n_info:] = 1
        dirty = np.packbits(dirty, axis=1)
        assert np.array_equal(fec.unpack_bits(dirty, n_info), info)
        row = fec.encode(rate, n_c, info)
        assert np.array_equal(fec.encode_rows(rate, n_c, dirty), row)
        llr = (127 * (1 - 2 * row.astype(np.int64))).astype(np.int8)
        bits, metric = fec.decode(rate, n_c, llr, bits_pitch=pitch)
        assert np.array_equal(bits, packed) and np.all(metric == 127 * ntx)
    if n_c % 4 == 0:
        assert np.array_equal(fec.encode_rows(rate, n_c, packed, form=fec.ENC_QAM, qam_bits=2),
                              fec.rows_to_idx(row, 2))


def _rc(f, info, out, n_rows, pitch, form, b):
    a = _lib.FecEncodeArgs(info, out, n_rows, pitch, form, b)
    return _lib.lib().mimo_fec_encode_rows(None if f is None else f._h, C.byref(a), None)


def test_encode_rows_argument_errors_need_no_gpu():
    """Every refusal of mimo_fec_encode_rows comes before the first HIP call: the addresses are
    never dereferenced, so plain integers stand in for device pointers."""
    L = _lib.lib()
    f = fec.Fec(fec.R12, 132)                  # n_info 60: 8 bytes, pitch >= 8; 132 = 6 * 22
    i, o = 0x10000, 0x20000
    B, Q = _lib.FEC_ENC_BITS, _lib.FEC_ENC_QAM
    bad = {
        "null d_info": (f, None, o, 4, 8, B, 0),
        "null d_out": (f, i, None, 4, 8, B, 0),
        "null f": (None, i, o, 4, 8, B, 0),
        "misaligned d_info": (f, i + 8, o, 4, 8, B, 0),
        "misaligned d_out": (f, i, o + 4, 4, 8, B, 0),
        "no rows": (f, i, o, 0, 8, B, 0),
        "pitch below ceil(n_info / 8)": (f, i, o, 4, 4, B, 0),
        "pitch no multiple of 4": (f, i, o, 4, 10, B, 0),
        "bad form": (f, i, o, 4, 8, 2, 0),
        "qam_bits with BITS": (f, i, o, 4, 8, B, 2),
        "qam_bits 0 with QAM": (f, i, o, 4, 8, Q, 0),
        "qam_bits 5 with QAM": (f, i, o, 4, 8, Q, 5),
        "n_c % 4 == 0 but n_c % 8 != 0": (f, i, o, 4, 8, Q, 4),
        "d_out inside d_info": (f, i, i + 16, 4, 8, B, 0),
        "d_info inside d_out": (f, o + 4 * 132 - 16, o, 4, 8, B, 0),
        "d_info inside a QAM d_out": (f, o + 64, o, 4, 8, Q, 3),      # 4 * 22 = 88 bytes
    }
    for what, args in bad.items():
        assert _rc(*args) == -1, what
        assert L.mimo_last_error(), what
    assert L.mimo_fec_encode_rows(f._h, None, None) == -1
    assert _rc(f, i, o, 4, 4, B, 0) == -1 and b"bits_pitch" in L.mimo_last_error()
    assert _rc(f, i, i + 16, 4, 8, B, 0) == -1 and b"overlap" in L.mimo_last_error()
    with pytest.raises(_lib.MimoError):
        f.encode_rows(i, 0, o)


def test_synth_payload_refuses_a_null_payload():
    """mimo_synth_frames_payload needs d_tx_idx unless pid = 0; refused before any HIP call."""
    S = Synthesizer(SynthParams(M=64, cp_len=16, num_streams=2, num_access_codes=4, pid=4,
                                qam_order=4))
    L = S.frame_len(0)
    with pytest.raises(_lib.MimoError):
        S.generate_payload(0x10000, L, L, 1, None)
    assert b"d_tx_idx" in _lib.lib().mimo_last_error()
    assert _lib.lib().mimo_synth_frames_payload(None, 0, 1, 0x10000, L, L, 0x20000, None,
                                                None) == -1
