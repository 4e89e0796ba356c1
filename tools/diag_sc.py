"""tools/diag_sc.py -- per-stage timing and per-frame sync positions of the receive pipeline.

Diagnostic only (GPU box): python tools/diag_sc.py [--frames F] [--reps R]
The library's RMIMO_* diagnostic switches (engine_diag.cpp: RMIMO_SC_PHASES, RMIMO_SC_COUNT,
RMIMO_LS_FORM, ...) apply to the run as to any other.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rub_mimo_amd import _lib  # noqa: E402
from rub_mimo_amd.receiver import Receiver, RxParams, Synthesizer, SynthParams  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--M", type=int, default=2048)
    ap.add_argument("--cp", type=int, default=152)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--pid", type=int, default=1000)
    ap.add_argument("--qam", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream(dev).cuda_stream
    F, N = args.frames, args.streams
    sp = SynthParams(M=args.M, cp_len=args.cp, num_streams=N, num_access_codes=20, pid=args.pid,
                     qam_order=args.qam, seed=1234, snr_db=30.0)
    syn = Synthesizer(sp)
    L = sp.max_frame_len()
    iq = torch.empty((F, N, L), dtype=torch.complex64, device=dev)
    syn.generate(iq, L, L, F, frame_id0=0, stream=sh)
    rx = Receiver(RxParams(M=args.M, cp_len=args.cp, num_streams=N, num_access_codes=20,
                           pid_max=args.pid, detector=_lib.DET_MMSE, qam_order=args.qam), stream=sh)
    m_occ = rx.M_occ
    out_sym = torch.empty((F, N, args.pid, m_occ), dtype=torch.complex64, device=dev)
    out_idx = torch.empty((F, N, args.pid, m_occ), dtype=torch.uint8, device=dev)

    def step():
        rx.process(iq, L, L, F, max_out=args.pid, out_sym=out_sym, out_idx=out_idx, ref_mode=2,
                   ref_seed=1234, frame_id0=0, stream=sh)

    for _ in range(3):
        step()
    torch.cuda.synchronize(dev)
    rx.stage_times()
    rx.set_timing(True)
    n0 = rx.sc_exact_count()
    for _ in range(args.reps):
        step()
    torch.cuda.synchronize(dev)
    st = rx.stage_times()
    n1 = rx.sc_exact_count()
    env = {k: v for k, v in os.environ.items() if k.startswith("RMIMO_")}
    print("env", env, "L", L, "chunks", (L + 8191) // 8192)
    print("stages_ms", {k: round(v[0] / max(v[1], 1), 4) for k, v in st.items()})
    print("exact/step", (n1 - n0) / args.reps)
    for f, r in enumerate(rx.results(F)):
        print(f"frame {f} status {r['status']} trigger {r.get('trigger')} sync {r.get('sync_index')}"
              f" chunk {r.get('trigger', 0) // 8192 if r.get('trigger') is not None else None}")


if __name__ == "__main__":
    main()
