"""GPU tests of the K = 7 encoder and bit mapper (mimo_fec_encode_rows; fec_encode_kernel in
fec_enc_kernels.hip) against the written definition in rub_mimo_amd/fec.py (fec.encode, the model
of the host's mimo_fec_encode, and fec.rows_to_idx). Integer arithmetic: every output byte is
compared, there are no tolerances.

Row lengths: 14 (the smallest row, T = 7 and one info bit at rate 1/2), 15 and 17 (a trailing
position no coded bit refers to; rows that start off a 16-byte boundary, and a row of one
16-byte unit plus one byte), 128 (a QPSK row of M_occ = 64), 1024, 12 288 (a C3 row) and 32 768
(the largest: 768 parity words at rate 3/4, three passes of the 256 threads). perm NULL and a
seeded random permutation of the n_tx coded bits into the n_c positions, so the holes fall
anywhere. Both forms, QAM for every b = 1..4 that divides n_c / 2. 1 and 3 rows, and 5000 rows at
n_c = 128: more workgroups than the grid has, so every workgroup strides.

The kernel has one path for every perm (the inverse position map makes perm a table read), so
there is no separate perm = NULL kernel to compare with."""
import functools

import numpy as np
import pytest

from rub_mimo_amd import _lib, fec

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0x4D
N_CS = [14, 15, 17, 128, 1024, 12288, 32768]
PERMS = ["null", "random"]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need an MI355X")


def _row_counts(n_c):
    return [1, 3, 5000] if n_c == 128 else [1, 3]


def _dirty(info, pitch):
    """pack_bits(info) with every bit outside the n_info info bits set: the low bits of the last
    info byte and all bytes up to the pitch."""
    n_info = info.shape[1]
    full = np.ones((info.shape[0], 8 * pitch), np.uint8)
    full[:, :n_info] = info
    return np.packbits(full, axis=1)


@functools.lru_cache(maxsize=None)
def _case(rate, n_c, kind):
    """Handle arguments, device input and the model's coded rows; computed once and shared (no
    test modifies them)."""
    rng = np.random.default_rng(100 * n_c + 10 * rate + PERMS.index(kind))
    T, n_info, ntx = fec.geometry(rate, n_c)
    perm = None if kind == "null" else rng.permutation(n_c)[:ntx].astype(np.uint16)
    rows = max(_row_counts(n_c))
    info = rng.integers(0, 2, (rows, n_info)).astype(np.uint8)
    pitch = fec.min_pitch(n_info) + (4 if kind == "random" else 0)
    packed = _dirty(info, pitch)
    assert np.array_equal(fec.unpack_bits(packed, n_info), info)
    assert np.all(packed[:, (n_info + 7) // 8:] == 0xFF)
    return perm, info, packed, pitch, fec.encode(rate, n_c, info, perm)


class _Out:
    """A device output of `nbytes` bytes between guard bytes, all pre-filled with FILL."""

    def __init__(self, nbytes):
        self.n = nbytes
        self.buf = _lib.DeviceBuffer(2 * GUARD + nbytes)
        self.fill()

    def fill(self):
        self.buf.upload(np.full(self.buf.nbytes, FILL, np.uint8))

    @property
    def addr(self):
        return self.buf.addr + GUARD

    def read(self):
        _lib.check(_lib.lib().mimo_stream_sync(None), "sync")
        b = self.buf.download(np.uint8, self.buf.nbytes)
        assert np.all(b[:GUARD] == FILL) and np.all(b[-GUARD:] == FILL)
        return b[GUARD:-GUARD].copy()


@pytest.mark.parametrize("kind", PERMS)
@pytest.mark.parametrize("n_c", N_CS)
@pytest.mark.parametrize("rate", fec.RATES)
def test_encode_rows_is_bitwise_the_model(rate, n_c, kind):
    """BITS: every one of the n_c bytes of every row is the model's (unreferenced positions 0,
    nothing left of the 0x4D fill). QAM, every b that divides n_c / 2: the model's rows through
    rows_to_idx. The set bits outside the info bits change nothing, the guard bytes stay, and a
    second call writes identical bytes."""
    perm, info, packed, pitch, row = _case(rate, n_c, kind)
    f = fec.Fec(rate, n_c, perm)
    assert f.geometry() == fec.geometry(rate, n_c)
    d_info = _lib.DeviceBuffer(packed.nbytes)
    d_info.upload(packed)
    forms = [(fec.ENC_BITS, 0)] + [(fec.ENC_QAM, b) for b in (1, 2, 3, 4) if n_c % (2 * b) == 0]
    for rows in _row_counts(n_c):
        for form, b in forms:
            want = row[:rows] if form == fec.ENC_BITS else fec.rows_to_idx(row[:rows], b)
            out = _Out(want.size)
            f.encode_rows(d_info, rows, out.addr, form=form, qam_bits=b, bits_pitch=pitch)
            got = out.read().reshape(want.shape)
            assert np.array_equal(got, want), (rows, form, b, np.argwhere(got != want)[:4])
            out.fill()
            f.encode_rows(d_info, rows, out.addr, form=form, qam_bits=b, bits_pitch=pitch)
            assert np.array_equal(out.read().reshape(want.shape), got), (rows, form, b)


@pytest.mark.parametrize("kind", PERMS)
@pytest.mark.parametrize("rate", fec.RATES)
def test_round_trip_through_the_decoder(rate, kind):
    """Encode (BITS) -> int8 LLRs +-127 -> mimo_fec_decode on the same handle: d_bits is the
    packed info with its padding zeroed and the metric is 127 n_tx."""
    n_c = 1024
    perm, info, packed, pitch, row = _case(rate, n_c, kind)
    rows = 3
    f = fec.Fec(rate, n_c, perm)
    d_info = _lib.DeviceBuffer(packed.nbytes)
    d_info.upload(packed)
    out = _Out(rows * n_c)
    f.encode_rows(d_info, rows, out.addr, bits_pitch=pitch)
    coded = out.read().reshape(rows, n_c)
    assert set(np.unique(coded)) <= {0, 1}
    llr = (127 * (1 - 2 * coded.astype(np.int64))).astype(np.int8)
    d_llr = _lib.DeviceBuffer(llr.nbytes)
    d_llr.upload(llr)
    bits, metric = _Out(rows * pitch), _Out(4 * rows)
    f.decode(d_llr, rows, bits.addr, pitch, metric.addr)
    assert np.array_equal(bits.read().reshape(rows, pitch), fec.pack_bits(info[:rows], pitch))
    assert np.all(metric.read().view(np.int32) == 127 * f.n_tx)
