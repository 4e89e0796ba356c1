#!/usr/bin/env python
"""Times the soft-output pass (mimo_rx_soft_demap) on the bench's C3 batch: 64 synthetic
captures, 4x4 MMSE, 2048-pt FFT, 64-QAM, max_out 1000, symbol-major output.

Per format (int8, fp32): one warm-up, then `--reps` launches timed with HIP events on the
receiver's stream. Each launch is the MSE kernel plus the demap kernel, as a caller pays it.
Bytes moved per launch: every symbol of every frame slot is read (8 B) and its 2b LLRs
written (2b B as int8, 8b B as fp32); the MSE pass's own traffic (G, W once per frame) is
three orders smaller and left out. The same run's batch time (ms_per_step) gives the scale.
Writes one JSON file (default profiles/r07/soft_demap_c3.json) and prints it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--pid", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10, help="batch steps timed for ms_per_step")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--llr-scale", type=float, default=0.05)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "soft_demap_c3.json"))
    args = ap.parse_args()

    import torch

    from rub_mimo_amd import _lib, soft
    from rub_mimo_amd.receiver import Receiver, RxParams, Synthesizer, SynthParams

    M, cp, N, nac, qam, pid, F = 2048, 152, 4, 20, 64, args.pid, args.frames
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.Stream(dev)      # the receiver's launch stream; the events time it
    sh = stream.cuda_stream
    sp = SynthParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid=pid,
                     qam_order=qam, seed=args.seed, snr_db=30.0)
    syn = Synthesizer(sp)
    L = sp.max_frame_len()
    iq = torch.empty((F, N, L), dtype=torch.complex64, device=dev)
    tx_idx = torch.empty((F, N, pid, M), dtype=torch.uint8, device=dev)
    syn.generate(iq, L, L, F, tx_idx=tx_idx, stream=sh)
    torch.cuda.synchronize()
    ref_rows = tx_idx.transpose(1, 2).contiguous()
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=_lib.DET_MMSE, qam_order=qam), stream=sh)
    m_occ = rx.M_occ
    layout = _lib.LAYOUT_SYMBOL_MAJOR
    out_sym = torch.zeros((F, pid, N, m_occ), dtype=torch.complex64, device=dev)
    out_idx = torch.zeros((F, pid, N, m_occ), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def step():
        rx.process(iq, L, L, F, max_out=pid, out_sym=out_sym, out_idx=out_idx, ref_mode=1,
                   ref_idx=ref_rows, stream=sh, out_layout=layout)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    for _ in range(3):          # (the second identical call captures the batch graph)
        step()
    ms_step = timed(step, args.steps)
    res = rx.results()
    synced = sum(r["status"] == _lib.FRAME_OK for r in res)

    nb = 2 * soft.qam_bits(qam)
    n_sym = F * pid * N * m_occ
    result = {
        "config": {"M": M, "cp": cp, "streams": N, "access_codes": nac, "qam": qam,
                   "detector": "mmse", "captures": F, "max_out": pid, "out_layout": "symbol",
                   "llr_scale": args.llr_scale, "reps": args.reps},
        "device": torch.cuda.get_device_name(dev),
        "frames_synced": synced,
        "symbols": n_sym,
        "ms_per_step": ms_step,
        "formats": {},
    }
    for name, fmt, elt, dt in (("int8", _lib.LLR_I8, 1, torch.int8),
                               ("fp32", _lib.LLR_F32, 4, torch.float32)):
        llr = torch.empty((F, pid, N, m_occ, nb), dtype=dt, device=dev)

        def launch():
            rx.soft_demap(out_sym, llr, max_out=pid, out_layout=layout, fmt=fmt,
                          llr_scale=args.llr_scale, stream=sh)

        launch()
        torch.cuda.synchronize()
        ms = timed(launch, args.reps)
        nbytes = n_sym * (8 + nb * elt)
        result["formats"][name] = {
            "ms_per_launch": ms, "bytes_read": n_sym * 8, "bytes_written": n_sym * nb * elt,
            "bytes_moved": nbytes, "tb_per_s": nbytes / (ms * 1e-3) / 1e12,
            "copy_ms_at_6.29_tb_per_s": nbytes / 6.29e12 * 1e3,
            "fraction_of_step": ms / ms_step,
        }
        if fmt == _lib.LLR_I8:
            torch.cuda.synchronize()
            v = llr[:, :8].to(torch.int32)
            result["formats"][name]["saturated_fraction_first_8_symbols"] = float(
                (v.abs() == 127).float().mean().item())
        del llr
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
