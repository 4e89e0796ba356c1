"""GPU tests of the coded transmit path end to end: mimo_synth_frames_payload against
mimo_synth_frames, and frames that carry encoded payloads (mimo_fec_encode_rows, QAM form)
through the batch, the int8 soft demap and mimo_fec_decode, back to the info bits.

Which channel the links use. The synthesiser's identity channel cannot carry a frame with more
than one stream: S0 goes out on stream 0 only and every receive antenna must see the plateau, so
an N >= 2 identity capture never syncs, in the reference as here (tests/test_oracle.py,
test_identity_bias_magnitude). The links therefore run on the two easy channels that do sync: a
1x1 geometry on the identity channel, and a 2x2 geometry on the synthesiser's drawn flat channel
with ZF detection, at a seed whose three frames all sync and whose channels are well conditioned
(smallest singular value 0.89 over the three frames; chosen with the CPU oracle, which draws the
same offsets, channels and noise). Sync is decided before the first data symbol, so it does not
depend on the payload.

Row alignment. With max_out = pid and the stream-major layout the LLR rows [F][N][pid] of
n_c = M_occ 2b values line up with the payload rows [F][N][pid][M_occ]; with max_out > pid the
LLR rows have pitch max_out symbols per stream and the rows pid..max_out-1 are zero."""
import ctypes as C
import functools

import numpy as np
import pytest

from rub_mimo_amd import _lib, fec, soft
from rub_mimo_amd.receiver import Receiver, RxParams, Synthesizer, SynthParams

pytestmark = pytest.mark.gpu

F = 3
LLR_SCALE = 4.0


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need an MI355X")


def _sync():
    _lib.check(_lib.lib().mimo_stream_sync(None), "sync")


# ---- payload identity ----
# M, cp, N, nac, pid, qam, synthesiser seed: rows of the post-pass tables (test_gpu_soft.py)
IDENT = {
    "qpsk_2x2": (64, 16, 2, 4, 10, 4, 79),
    "qam64_4x4": (128, 32, 4, 8, 8, 64, 77),
}


@functools.lru_cache(maxsize=None)
def _ident(name):
    """The hash-drawn capture, its indices and channels (mimo_synth_frames), computed once."""
    M, cp, N, nac, pid, qam, seed = IDENT[name]
    S = Synthesizer(SynthParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid=pid,
                                qam_order=qam, seed=seed, snr_db=30.0))
    L = max(S.frame_len(i) for i in range(F))
    iq, tx, H = (_lib.DeviceBuffer(F * N * L * 8), _lib.DeviceBuffer(F * N * pid * M),
                 _lib.DeviceBuffer(F * N * N * 8))
    S.generate(iq, L, L, F, tx_idx=tx, H=H)
    _sync()
    return (S, L, iq.download(np.uint8, iq.nbytes), tx.download(np.uint8, tx.nbytes),
            H.download(np.uint8, H.nbytes))


def _payload_capture(S, L, N, idx):
    """(capture bytes, channel bytes) of mimo_synth_frames_payload for the indices idx."""
    iq, tx, H = (_lib.DeviceBuffer(F * N * L * 8), _lib.DeviceBuffer(idx.size),
                 _lib.DeviceBuffer(F * N * N * 8))
    iq.upload(np.full(iq.nbytes, 0x4D, np.uint8))
    H.upload(np.full(H.nbytes, 0x4D, np.uint8))
    tx.upload(idx)
    S.generate_payload(iq, L, L, F, tx, H=H)
    _sync()
    return iq.download(np.uint8, iq.nbytes), H.download(np.uint8, H.nbytes)


@pytest.mark.parametrize("name", list(IDENT))
def test_payload_of_the_hash_draw_gives_the_same_capture(name):
    """Fed the d_tx_idx mimo_synth_frames wrote, mimo_synth_frames_payload writes the same three
    captures (drawn offsets) and d_H, bit for bit; indices with bits above L^2 set give the same
    capture as the masked ones."""
    M, cp, N, nac, pid, qam, seed = IDENT[name]
    S, L, iq0, tx0, H0 = _ident(name)
    assert len({S.frame_len(i) for i in range(F)}) > 1            # the offsets differ
    assert tx0.max() == qam - 1 and len(np.unique(tx0)) == qam
    iq1, H1 = _payload_capture(S, L, N, tx0)
    assert np.array_equal(iq1, iq0) and np.array_equal(H1, H0)
    iq2, H2 = _payload_capture(S, L, N, tx0 | np.uint8(0x100 - qam))
    assert np.array_equal(iq2, iq0) and np.array_equal(H2, H0)


@pytest.mark.parametrize("name", list(IDENT))
def test_one_changed_index_changes_one_symbol_window(name):
    """A payload with one index changed differs from the original only inside that symbol's SL
    samples, in its frame, and there on every antenna (the drawn channel has no zero entry)."""
    M, cp, N, nac, pid, qam, seed = IDENT[name]
    S, L, iq0, tx0, H0 = _ident(name)
    SL = M + cp
    f, t, sym, j = 2, N - 1, pid - 3, M // 3
    idx = tx0.reshape(F, N, pid, M).copy()
    idx[f, t, sym, j] ^= 1
    iq1, H1 = _payload_capture(S, L, N, idx.reshape(-1))
    assert np.array_equal(H1, H0)
    a = iq0.view(np.complex64).reshape(F, N, L)
    b = iq1.view(np.complex64).reshape(F, N, L)
    u = S.frame_len(f) - SL * (2 * N * nac + 2 + pid + S.params.tail_syms)
    start = SL * (N * nac + 1) + u + SL * (N * nac + 1) + sym * SL
    diff = a.view(np.uint64) != b.view(np.uint64)
    assert not diff[:f].any() and not diff[f + 1:].any()
    for r in range(N):
        at = np.flatnonzero(diff[f, r])
        assert len(at) > SL // 2 and at.min() >= start and at.max() < start + SL, (r, at[:4])


# ---- a real link ----
# M, cp, N, nac, pid, detector, identity channel, synthesiser seed
GEOMS = {
    "1x1_identity": (64, 16, 1, 4, 10, _lib.DET_ZF, True, 1),
    "2x2_drawn": (64, 16, 2, 4, 10, _lib.DET_ZF, False, 99),
    "1x1_identity_m256": (256, 32, 1, 4, 8, _lib.DET_ZF, True, 1),
}


def _run_link(geom, rate, qam, with_perm, snr_db):
    """Encode (QAM form) -> generate_payload -> Receiver.process -> soft demap (int8) ->
    mimo_fec_decode. Returns the frame results, the info bits, the decoded bits and the raw bit
    errors of the batch's own hard decisions per row, counted against the payload."""
    M, cp, N, nac, pid, det, ident, seed = GEOMS[geom]
    b = soft.qam_bits(qam)
    n_c, rows = M * 2 * b, F * N * pid
    rng = np.random.default_rng(1000 * seed + 10 * qam + rate)
    T, n_info, ntx = fec.geometry(rate, n_c)
    perm = rng.permutation(n_c)[:ntx].astype(np.uint16) if with_perm else None
    f = fec.Fec(rate, n_c, perm)
    info = rng.integers(0, 2, (rows, n_info)).astype(np.uint8)
    pitch = f.min_pitch()
    d_info = _lib.DeviceBuffer(rows * pitch)
    d_info.upload(fec.pack_bits(info, pitch))
    tx = _lib.DeviceBuffer(rows * M)
    f.encode_rows(d_info, rows, tx, form=fec.ENC_QAM, qam_bits=b)
    S = Synthesizer(SynthParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid=pid,
                                qam_order=qam, seed=seed, snr_db=snr_db,
                                identity_channel=ident))
    L = max(S.frame_len(i) for i in range(F))
    iq = _lib.DeviceBuffer(F * N * L * 8)
    S.generate_payload(iq, L, L, F, tx)
    _sync()
    sent = tx.download(np.uint8, rows * M).reshape(rows, M)
    assert np.array_equal(sent, fec.rows_to_idx(fec.encode(rate, n_c, info, perm), b))
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=det, keep_identity_bias=False, qam_order=qam))
    assert rx.M_occ == M
    osym, oidx = _lib.DeviceBuffer(rows * M * 8), _lib.DeviceBuffer(rows * M)
    llr = _lib.DeviceBuffer(rows * n_c)
    rx.process(iq, L, L, F, max_out=pid, out_sym=osym, out_idx=oidx,
               out_layout=_lib.LAYOUT_STREAM_MAJOR)
    rx.soft_demap(osym, llr, max_out=pid, out_layout=_lib.LAYOUT_STREAM_MAJOR, fmt=_lib.LLR_I8,
                  llr_scale=LLR_SCALE)
    res = rx.results()                                   # (synchronises)
    bits = _lib.DeviceBuffer(rows * pitch)
    f.decode(llr, rows, bits, pitch)
    _sync()
    dec = fec.unpack_bits(bits.download(np.uint8, rows * pitch).reshape(rows, pitch), n_info)
    hard = oidx.download(np.uint8, rows * M).reshape(rows, M)
    raw = np.unpackbits(hard ^ sent, axis=1).sum(axis=1)
    return res, info, dec, raw, pid


def _all_synced(res, pid):
    return all(r["status"] == _lib.FRAME_OK and r["n_sym"] >= pid for r in res)


@pytest.mark.parametrize("with_perm", [False, True], ids=["perm_null", "perm_random"])
@pytest.mark.parametrize("qam", [4, 16])
@pytest.mark.parametrize("rate", fec.RATES)
@pytest.mark.parametrize("geom", ["1x1_identity", "2x2_drawn"])
def test_link_on_an_easy_channel_returns_the_info_bits(geom, rate, qam, with_perm):
    """30 dB: all three frames sync and every row of every frame decodes to exactly its info
    bits. A wrong bit order in the mapper, a wrong puncture phase or a perm applied in the wrong
    direction turns about half of the decoded bits over, noise or not."""
    res, info, dec, raw, pid = _run_link(geom, rate, qam, with_perm, 30.0)
    assert _all_synced(res, pid), [(r["status"], r["n_sym"]) for r in res]
    wrong = (dec != info).sum(axis=1)
    print("%s rate %d qam %d perm %s: raw bit errors %d, info-bit errors %d"
          % (geom, rate, qam, with_perm, raw.sum(), wrong.sum()))
    assert not wrong.any(), np.flatnonzero(wrong)


def test_link_where_the_code_has_work_to_do():
    """64-QAM, rate 1/2, 1x1 identity channel, M = 256 (24 rows of n_c = 1536), at 17 dB.

    Where the 17 comes from: the CPU models alone (unit-gain AWGN on the 64-QAM points, soft.py's
    max-log demap quantised to int8 at llr_scale 4, fec.decode) on 240 rows, ten times this
    test's, seeded: 12 info-bit errors at 13 dB, none at 14 dB and none at any whole dB up to 21.
    14 dB is the lowest whole-dB SNR without an error; 3 dB are added for the estimated channel
    and the int8 weights of the real pass: 17 dB. (The same model has 13 321 raw bit errors in
    368 640 coded bits at 17 dB.)

    At 17 dB on the GPU: all three frames sync, the batch's own hard decisions have raw bit
    errors against the payload, and the decoded info bits have none. (Measured on an MI355X:
    1702 raw bit errors of 36 864, 0 info-bit errors of 18 288.)"""
    res, info, dec, raw, pid = _run_link("1x1_identity_m256", fec.R12, 64, False, 17.0)
    assert _all_synced(res, pid), [(r["status"], r["n_sym"]) for r in res]
    wrong = (dec != info).sum(axis=1)
    print("raw bit errors %d of %d, info-bit errors %d of %d"
          % (raw.sum(), raw.size * 1536, wrong.sum(), info.size))
    assert raw.sum() > 0
    assert not wrong.any(), np.flatnonzero(wrong)


def _hip():
    """The HIP runtime the library has loaded, for stream capture."""
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln)
    return C.CDLL(path)


def test_encode_rows_replays_from_a_captured_graph():
    """After one warm-up call (which creates the handle's table), mimo_fec_encode_rows is
    captured into a graph on a side stream; the capture runs nothing, and every replay writes
    the bytes of the direct call."""
    rate, n_c, rows, b = fec.R34, 1536, 40, 3
    rng = np.random.default_rng(5)
    T, n_info, ntx = fec.geometry(rate, n_c)
    perm = rng.permutation(n_c)[:ntx].astype(np.uint16)
    f = fec.Fec(rate, n_c, perm)
    info = rng.integers(0, 2, (rows, n_info)).astype(np.uint8)
    want = fec.rows_to_idx(fec.encode(rate, n_c, info, perm), b)
    d_info = _lib.DeviceBuffer(rows * f.min_pitch())
    d_info.upload(fec.pack_bits(info, f.min_pitch()))
    out = _lib.DeviceBuffer(want.size)
    hip = _hip()
    side, graph, ex = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(side), 1) == 0          # hipStreamNonBlocking

    def read():
        assert hip.hipStreamSynchronize(side) == 0
        got = out.download(np.uint8, want.size).reshape(want.shape)
        out.upload(np.full(want.size, 0x4D, np.uint8))
        return got

    def encode():
        f.encode_rows(d_info, rows, out, form=fec.ENC_QAM, qam_bits=b, stream=side.value)

    try:
        encode()
        assert np.array_equal(read(), want)
        assert hip.hipStreamBeginCapture(side, 1) == 0                  # thread-local mode
        encode()
        assert hip.hipStreamEndCapture(side, C.byref(graph)) == 0
        assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, C.c_size_t(0)) == 0
        assert np.all(read() == 0x4D)                                   # captured, not run
        for _ in range(2):
            assert hip.hipGraphLaunch(ex, side) == 0
            assert np.array_equal(read(), want)
    finally:
        if ex:
            hip.hipGraphExecDestroy(ex)
        if graph:
            hip.hipGraphDestroy(graph)
        hip.hipStreamDestroy(side)
