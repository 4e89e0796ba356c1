#!/usr/bin/env python
"""Times the soft-output SIC pass (mimo_rx_sic_soft) on the bench's C3 batch: 64 synthetic
captures, 4x4 MMSE, 2048-pt FFT, 64-QAM, max_out 1000, symbol-major output.

Per form (int8 LLRs + idx, int8 LLRs only, fp32 LLRs + idx): one warm-up, then `--reps`
launches timed with HIP events on the receiver's stream, repeated `--rounds` times (median and
spread reported). Each launch is the table kernel plus the symbol kernel, as a caller pays it.
In the same process the two-pass composition it replaces is timed the same way:
mimo_rx_sic_detect (z + idx) followed by mimo_rx_soft_demap int8 on that z. The composition's
LLRs carry the wrong weights (the linear nu, not nu_sic), but its bytes and work are the same;
its two launches are also timed apart, and `fused_over_two_pass` is the fused int8 + idx time
over the composition's.

Algorithmic bytes per launch: every symbol of every frame slot is read once (8 B) and its
2b LLR values (1 or 4 B each) and index (1 B) written; the two-pass form adds z written (8 B) and
read again (8 B). The tables' own traffic is left out. Rows the decode did not write are written
as zeros but not read by the SIC kernels: bytes_touched counts the reads of written rows only.
Writes one JSON file (default profiles/r09/sic_soft_c3.json) and prints it.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--pid", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="batch steps timed for ms_per_step")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "sic_soft_c3.json"))
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
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=_lib.DET_MMSE, qam_order=qam), stream=sh)
    m_occ = rx.M_occ
    syn.generate(iq, L, L, F, stream=sh)
    torch.cuda.synchronize()
    layout = _lib.LAYOUT_SYMBOL_MAJOR
    out_sym = torch.zeros((F, pid, N, m_occ), dtype=torch.complex64, device=dev)
    torch.cuda.synchronize()

    def step():
        rx.process(iq, L, L, F, max_out=pid, out_sym=out_sym, stream=sh, out_layout=layout)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def rounds(fn):
        fn()
        torch.cuda.synchronize()
        ms = [timed(fn, args.reps) for _ in range(args.rounds)]
        return {"ms_per_launch": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

    for _ in range(3):          # (the second identical call captures the batch graph)
        step()
    ms_step = timed(step, args.steps)
    res = rx.results()
    synced = sum(r["status"] == _lib.FRAME_OK for r in res)

    n_sym = F * pid * N * m_occ
    nb = 2 * soft.qam_bits(qam)
    z_sym = torch.empty((F, pid, N, m_occ), dtype=torch.complex64, device=dev)
    z_idx = torch.empty((F, pid, N, m_occ), dtype=torch.uint8, device=dev)
    llr8 = torch.empty((F, pid, N, m_occ, nb), dtype=torch.int8, device=dev)
    result = {
        "config": {"M": M, "cp": cp, "streams": N, "access_codes": nac, "qam": qam,
                   "detector": "mmse", "captures": F, "max_out": pid, "out_layout": "symbol",
                   "reps": args.reps, "rounds": args.rounds},
        "device": torch.cuda.get_device_name(dev),
        "frames_synced": synced,
        "symbols": n_sym,
        "ms_per_step": ms_step,
        "forms": {},
    }
    written_rows = sum(min(r["n_sym"], pid) for r in res if r["status"] == _lib.FRAME_OK)
    n_read = written_rows * N * m_occ
    result["symbols_in_written_rows"] = n_read

    def form(name, fn, read, written, read_skips):
        """read / written: bytes per symbol; read_skips: of `read`, the bytes per symbol that
        are not read on rows the decode did not write."""
        r = rounds(fn)
        nbytes = n_sym * (read + written)
        touched = nbytes - (n_sym - n_read) * read_skips
        r.update({"bytes_read": n_sym * read, "bytes_written": n_sym * written,
                  "bytes_moved": nbytes,
                  "tb_per_s": nbytes / (r["ms_per_launch"] * 1e-3) / 1e12,
                  "bytes_touched": touched,
                  "tb_per_s_touched": touched / (r["ms_per_launch"] * 1e-3) / 1e12,
                  "fraction_of_step": r["ms_per_launch"] / ms_step})
        result["forms"][name] = r

    kw = dict(max_out=pid, out_layout=layout, stream=sh)

    def detect():
        rx.sic_detect(out_sym, z_sym, z_idx, **kw)

    def demap():
        rx.soft_demap(z_sym, llr8, fmt=_lib.LLR_I8, llr_scale=0.05, **kw)

    def two_pass():
        detect()
        demap()

    form("sic_soft_int8_idx", lambda: rx.sic_soft(out_sym, llr8, None, z_idx, fmt=_lib.LLR_I8,
                                                  llr_scale=0.05, **kw), 8, nb + 1, 8)
    form("sic_soft_int8_only", lambda: rx.sic_soft(out_sym, llr8, None, None, fmt=_lib.LLR_I8,
                                                   llr_scale=0.05, **kw), 8, nb, 8)
    # the composition and its parts (soft_demap reads every row of z, written or not)
    form("two_pass_sic_detect_then_soft_demap_int8", two_pass, 16, 9 + nb, 8)
    form("sic_detect_sym_idx", detect, 8, 9, 8)
    form("soft_demap_int8_of_z", demap, 8, nb, 0)
    llr32 = torch.empty((F, pid, N, m_occ, nb), dtype=torch.float32, device=dev)
    form("sic_soft_fp32_idx", lambda: rx.sic_soft(out_sym, llr32, None, z_idx, fmt=_lib.LLR_F32,
                                                  llr_scale=0.05, **kw), 8, 4 * nb + 1, 8)
    del llr32
    torch.cuda.synchronize()
    fm = result["forms"]
    result["fused_over_two_pass"] = (fm["sic_soft_int8_idx"]["ms_per_launch"] /
                                     fm["two_pass_sic_detect_then_soft_demap_int8"]["ms_per_launch"])
    result["fused_over_sum_of_parts"] = fm["sic_soft_int8_idx"]["ms_per_launch"] / (
        fm["sic_detect_sym_idx"]["ms_per_launch"] + fm["soft_demap_int8_of_z"]["ms_per_launch"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
