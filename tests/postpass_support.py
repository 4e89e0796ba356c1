"""Helpers shared by the GPU tests of the opt-in passes after the batch (test_gpu_soft.py,
test_gpu_sic.py, test_gpu_sic_soft.py): the synthetic three-frame capture, the case
parametrisation and the small readers of a batch's results. A plain module, imported by name;
each test file keeps its own CASES, run_case and fixtures."""
import numpy as np
import pytest

from rub_mimo_amd import _lib
from rub_mimo_amd import framing as fr
from rub_mimo_amd.receiver import Synthesizer, SynthParams

LAYOUTS = [_lib.LAYOUT_STREAM_MAJOR, _lib.LAYOUT_SYMBOL_MAJOR]
LAYOUT_IDS = ["stream_major", "symbol_major"]
N_FRAMES = 3
NOISE_FRAME = 1


def _sctype(M, kind):
    if kind == "liquid":
        return fr.ofdmframe_init_liquid_sctype(M)
    if kind == "all":
        return np.full(M, 2, np.uint8)
    return None


def _synth_capture(M, cp, N, nac, pid, qam, p, seed, noise_frame=NOISE_FRAME, tx=None):
    """N_FRAMES synthetic captures at 30 dB on the device, one replaced by a noise-only
    capture (no plateau: MIMO_FRAME_NO_SYNC)."""
    S = Synthesizer(SynthParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid=pid,
                                qam_order=qam, seed=seed, snr_db=30.0, p=p))
    L = max(S.frame_len(i) for i in range(N_FRAMES))
    iq = _lib.DeviceBuffer(N_FRAMES * N * L * 8)
    S.generate(iq, L, L, N_FRAMES, tx_idx=tx)
    _lib.check(_lib.lib().mimo_stream_sync(None), "sync")
    if noise_frame is not None:
        host = iq.download(np.complex64, N_FRAMES * N * L).reshape(N_FRAMES, N, L)
        rng = np.random.default_rng(seed)
        host[noise_frame] = 0.01 * (rng.standard_normal((N, L)) + 1j * rng.standard_normal((N, L)))
        iq.upload(host)
    return iq, L


def _n_out(r, mo):
    return min(r["n_sym"], mo) if r["status"] == _lib.FRAME_OK else 0


def _res_bytes(res):
    return [tuple(v.tobytes() if isinstance(v, np.ndarray) else v for v in r.values())
            for r in res]


def _case_params(cases):
    """Decorator: every case of the table `cases`, in both layouts."""
    def deco(fn):
        fn = pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)(fn)
        return pytest.mark.parametrize("name", list(cases))(fn)
    return deco
