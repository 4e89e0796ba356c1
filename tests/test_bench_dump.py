"""bench.py's --dump-outputs writer and its --full switch, on host tensors. CPU only."""
import sys

import numpy as np
import pytest
import torch

import bench


def _res(status, n_sym, N):
    return [dict(status=s, n_sym=n, sync_index=100 + i, origin=i, evm_num=np.full(N, 1.5 + i),
                 evm_den=np.full(N, 2.0), errors=np.full(N, i, np.int64))
            for i, (s, n) in enumerate(zip(status, n_sym))]


@pytest.mark.parametrize("sym_major", [True, False])
def test_dump_outputs_masks_unwritten_positions(tmp_path, sym_major):
    OK = 0
    slots, pid, N, m_occ = 3, 5, 2, 7
    shape = (slots, pid, N, m_occ) if sym_major else (slots, N, pid, m_occ)
    rng = np.random.default_rng(3)
    sym = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    idx = rng.integers(1, 64, shape).astype(np.uint8)
    res = _res([OK, 2, OK], [pid, pid, 3], N)          # slot 1 never decoded, slot 2 short
    bench.dump_outputs(str(tmp_path), 0, res, torch.from_numpy(sym), torch.from_numpy(idx),
                       pid, N, m_occ, sym_major, OK)
    got_sym = np.load(tmp_path / "out_sym.npy")
    got_idx = np.load(tmp_path / "out_idx.npy")
    assert got_sym.dtype == np.float32 and got_idx.dtype == np.float32
    want = sym.copy()
    want_idx = idx.copy()
    want[1] = 0
    want_idx[1] = 0
    if sym_major:
        want[2, 3:] = 0
        want_idx[2, 3:] = 0
    else:
        want[2, :, 3:] = 0
        want_idx[2, :, 3:] = 0
    assert np.array_equal(got_sym[:, 0] + 1j * got_sym[:, 1], want.reshape(-1))
    assert np.array_equal(got_idx, want_idx.reshape(-1).astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "frame_status.npy"), [0.0, 2.0, 0.0])
    assert np.array_equal(np.load(tmp_path / "frame_n_sym.npy"), [5.0, 0.0, 3.0])
    evm = np.load(tmp_path / "frame_evm_num.npy")
    assert evm.dtype == np.float64 and evm.shape == (slots, N)
    assert np.array_equal(evm[:, 0], [1.5, 0.0, 3.5])


def test_dump_outputs_samples_large_outputs_identically(tmp_path):
    slots, pid, N, m_occ = 2, 40, 4, 8192                # 2.6M elements > the sample size
    n = slots * pid * N * m_occ
    assert n > bench.DUMP_SAMPLE
    sym = torch.arange(n, dtype=torch.float32).to(torch.complex64).reshape(slots, pid, N, m_occ)
    idx = torch.zeros((slots, pid, N, m_occ), dtype=torch.uint8)
    res = _res([0, 0], [pid, pid], N)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 0, res, sym, idx, pid, N, m_occ, True, 0)
    a = np.load(tmp_path / "a" / "out_sym.npy")
    assert a.shape == (bench.DUMP_SAMPLE, 2)
    assert np.array_equal(a, np.load(tmp_path / "b" / "out_sym.npy"))
    assert np.all(np.diff(a[:, 0]) >= 0) and a[:, 0].max() < n
    total = sum(f.stat().st_size for f in (tmp_path / "a").iterdir())
    assert total <= 64 * 2 ** 20


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"
