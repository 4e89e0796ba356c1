#!/usr/bin/env python
"""Times the layered tree-search pass (mimo_rx_lord_soft) on the bench's C3 batch, the batch of
bench_pic.py (64 synthetic captures at 30 dB, 4x4 MMSE, 2048-pt FFT, 64-QAM, max_out 1000,
symbol-major output), and measures its LLRs against the linear detector's on noisier batches.
Nothing is asserted: every figure is recorded as measured.

Timing, per form of mimo_rx_lord_soft (int8 LLRs + idx, int8 LLRs only, fp32 LLRs + idx) with
`--lord-reps` launches per round, and for mimo_rx_pic_soft with NULL priors (int8 + idx),
mimo_rx_sic_soft_fb int8 + idx and mimo_rx_soft_demap int8 beside them in the same process with
`--reps`: one warm-up, then the launches timed with HIP events on the receiver's stream,
repeated `--rounds` times (median and spread). Each launch is the table kernel plus the symbol
kernel, as a caller pays it.

Quality, on `--loop-frames` captures of `--loop-pid` symbols at `--loop-snr-db` (plateau
threshold 0.85; rate 1/2 on the first SNR, rate 3/4 on the last), for mimo_rx_lord_soft and for
mimo_rx_pic_soft with NULL priors: the generalised mutual information per bit of the int8 LLRs,
then info-bit errors and rows in error after one mimo_fec_siso pass. One codeword per (symbol,
stream) row: random info bits through the code's linearity, as in bench_pic.py.

`--bench-json` and `--bench-parent-json` name files that hold the JSON line of one
`bench.py --gpus 1 --steps 20 --warmup 5` run of this build and of the parent commit's; both
are copied into the result. Writes one JSON file (default profiles/r15/lord_c3.json) and prints it.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _last_json_line(path):
    with open(path) as fh:
        lines = [l for l in fh.read().splitlines() if l.strip().startswith("{")]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--pid", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lord-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="batch steps timed for ms_per_step")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--snr-db", type=float, default=30.0)
    ap.add_argument("--llr-scale", type=float, default=4.0)
    ap.add_argument("--loop-frames", type=int, default=8)
    ap.add_argument("--loop-pid", type=int, default=48)
    ap.add_argument("--loop-snr-db", default="18,22", help="SNR of the rate 1/2 and 3/4 loops")
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--bench-json", default=None)
    ap.add_argument("--bench-parent-json", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "lord_c3.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from rub_mimo_amd import _lib, fec, soft
    from rub_mimo_amd.receiver import Receiver, RxParams, Synthesizer, SynthParams

    M, cp, N, nac, qam = 2048, 152, 4, 20, 64
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.Stream(dev)      # the receiver's launch stream; the events time it
    sh = stream.cuda_stream
    layout = _lib.LAYOUT_SYMBOL_MAJOR
    nb = 2 * soft.qam_bits(qam)
    sc = args.llr_scale
    result = {"device": torch.cuda.get_device_name(dev)}

    def batch(F, pid, snr_db, threshold=None):
        sp = SynthParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid=pid,
                         qam_order=qam, seed=args.seed, snr_db=snr_db)
        syn = Synthesizer(sp)
        L = sp.max_frame_len()
        iq = torch.empty((F, N, L), dtype=torch.complex64, device=dev)
        kw = {} if threshold is None else {"plateau_threshold": threshold}
        rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                               detector=_lib.DET_MMSE, qam_order=qam, **kw), stream=sh)
        tx_idx = torch.zeros((F, N, pid, rx.M_occ), dtype=torch.uint8, device=dev)
        syn.generate(iq, L, L, F, tx_idx=tx_idx, stream=sh)
        out_sym = torch.zeros((F, pid, N, rx.M_occ), dtype=torch.complex64, device=dev)
        torch.cuda.synchronize()
        step = lambda: rx.process(iq, L, L, F, max_out=pid, out_sym=out_sym, stream=sh,
                                  out_layout=layout)
        return rx, tx_idx, out_sym, step

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def rounds(fn, reps=None):
        fn()
        torch.cuda.synchronize()
        ms = [timed(fn, reps or args.reps) for _ in range(args.rounds)]
        return {"ms_per_launch": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

    # ---- timing on the C3 batch ----
    if not args.skip_timing:
        F, pid = args.frames, args.pid
        rx, tx_idx, out_sym, step = batch(F, pid, args.snr_db)
        m_occ = rx.M_occ
        for _ in range(3):          # (the second identical call captures the batch graph)
            step()
        ms_step = timed(step, args.steps)
        res = rx.results()
        kw = dict(max_out=pid, out_layout=layout, stream=sh)
        z_idx = torch.empty((F, pid, N, m_occ), dtype=torch.uint8, device=dev)
        llr8 = torch.empty((F, pid, N, m_occ, nb), dtype=torch.int8, device=dev)
        forms = {}

        def form(name, fn, reps=None):
            r = rounds(fn, reps)
            r["fraction_of_step"] = r["ms_per_launch"] / ms_step
            forms[name] = r

        form("soft_demap_int8", lambda: rx.soft_demap(out_sym, llr8, fmt=_lib.LLR_I8,
                                                      llr_scale=sc, **kw))
        form("sic_soft_fb_int8_idx", lambda: rx.sic_soft_fb(out_sym, llr8, None, z_idx,
                                                            fmt=_lib.LLR_I8, llr_scale=sc, **kw))
        form("pic_int8_null_priors_idx", lambda: rx.pic_soft(
            out_sym, llr8, None, None, z_idx, fmt=_lib.LLR_I8, llr_scale=sc, **kw))
        form("lord_int8_idx", lambda: rx.lord_soft(
            out_sym, llr8, z_idx, fmt=_lib.LLR_I8, llr_scale=sc, **kw), args.lord_reps)
        form("lord_int8_only", lambda: rx.lord_soft(
            out_sym, llr8, None, fmt=_lib.LLR_I8, llr_scale=sc, **kw), args.lord_reps)
        llr32 = torch.empty((F, pid, N, m_occ, nb), dtype=torch.float32, device=dev)
        form("lord_fp32_idx", lambda: rx.lord_soft(
            out_sym, llr32, z_idx, fmt=_lib.LLR_F32, llr_scale=sc, **kw), args.lord_reps)
        torch.cuda.synchronize()
        result["timing"] = {
            "config": {"M": M, "cp": cp, "streams": N, "access_codes": nac, "qam": qam,
                       "detector": "mmse", "captures": F, "max_out": pid, "out_layout": "symbol",
                       "snr_db": args.snr_db, "llr_scale": sc, "reps": args.reps,
                       "lord_reps": args.lord_reps, "rounds": args.rounds},
            "frames_synced": sum(r["status"] == _lib.FRAME_OK for r in res),
            "symbols": F * pid * N * m_occ,
            "ms_per_step": ms_step,
            "forms": forms,
            "lord_over_pic_null": (forms["lord_int8_idx"]["ms_per_launch"] /
                                   forms["pic_int8_null_priors_idx"]["ms_per_launch"]),
        }
        del rx, tx_idx, out_sym, z_idx, llr8, llr32
        torch.cuda.empty_cache()

    # ---- the loop ----
    snrs = [float(v) for v in args.loop_snr_db.split(",")]
    loops = {}
    for rate, name, snr in () if args.skip_loop else ((fec.R12, "1/2", snrs[0]),
                                                      (fec.R34, "3/4", snrs[-1])):
        F, pid = args.loop_frames, args.loop_pid
        rx, tx_idx, out_sym, step = batch(F, pid, snr, 0.85)
        m_occ = rx.M_occ
        step()
        res = rx.results()
        n_out = torch.tensor([min(r["n_sym"], pid) if r["status"] == _lib.FRAME_OK else 0
                              for r in res], device=dev)
        n_c = m_occ * nb
        rows = F * pid * N
        live = (torch.arange(pid, device=dev)[None, :] < n_out[:, None])[:, :, None] \
            .expand(F, pid, N).reshape(rows)
        code = fec.Fec(rate, n_c)
        pA, pB = fec.positions(rate, n_c)
        posA = torch.from_numpy(pA[pA >= 0]).to(dev)
        posB = torch.from_numpy(pB[pB >= 0]).to(dev)
        keepA = torch.from_numpy(np.flatnonzero(pA >= 0)).to(dev)
        keepB = torch.from_numpy(np.flatnonzero(pB >= 0)).to(dev)
        T = code.steps
        gen = torch.Generator(device=dev)
        gen.manual_seed(args.seed)
        info = torch.randint(0, 2, (rows, code.n_info), dtype=torch.uint8, device=dev,
                             generator=gen)
        u = torch.zeros((rows, T + 6), dtype=torch.uint8, device=dev)
        u[:, 6:6 + code.n_info] = info
        at = lambda d: u[:, 6 - d:6 - d + T]
        A = at(0) ^ at(2) ^ at(3) ^ at(5) ^ at(6)
        B = at(0) ^ at(1) ^ at(2) ^ at(3) ^ at(6)
        c = torch.zeros((rows, n_c), dtype=torch.uint8, device=dev)
        c[:, posA] = A[:, keepA]
        c[:, posB] = B[:, keepB]
        shifts = torch.arange(nb - 1, -1, -1, device=dev, dtype=torch.int32)
        sent = tx_idx.permute(0, 2, 1, 3).to(torch.int32)                     # [F][pid][N][M_occ]
        x = ((sent[..., None] >> shifts) & 1).to(torch.uint8).reshape(rows, n_c)
        flip = (x ^ c) == 1
        llr8 = torch.empty((rows, n_c), dtype=torch.int8, device=dev)
        dec_in = torch.empty((rows, n_c), dtype=torch.int8, device=dev)
        ext = torch.zeros((rows, n_c), dtype=torch.int8, device=dev)
        il = torch.empty((rows, code.min_info_pitch()), dtype=torch.int8, device=dev)
        kw = dict(max_out=pid, out_layout=layout, stream=sh, fmt=_lib.LLR_I8, llr_scale=sc)
        runs = {}
        with torch.cuda.stream(stream):
            for tag in ("lord", "pic_null_priors"):
                if tag == "lord":
                    rx.lord_soft(out_sym, llr8, None, **kw)
                else:
                    rx.pic_soft(out_sym, llr8, None, **kw)
                v = llr8.to(torch.float64) / sc
                lo = torch.nn.functional.softplus(torch.where(x == 1, v, -v))[live]
                gmi = 1.0 - float(lo.mean()) / 0.6931471805599453
                torch.where(flip, -llr8, llr8, out=dec_in)
                ext.zero_()
                code.siso(dec_in, rows, ext, None, il, None, fec.SISO_EXT, stream=sh)
                bad = ((il[:, :code.n_info] < 0) != (info == 1)) & live[:, None]
                runs[tag] = {"info_bit_errors": int(bad.sum()),
                             "rows_in_error": int(bad.any(dim=1).sum()),
                             "gmi_per_bit_detector_int8": gmi}
        loops[name] = {"snr_db": snr, "captures": F, "max_out": pid, "llr_scale": sc,
                       "frames_synced": int((n_out > 0).sum()), "rows": int(live.sum()),
                       "info_bits": int(live.sum()) * code.n_info, "n_c": n_c, "runs": runs}
        del rx, tx_idx, out_sym, llr8, dec_in, ext
        torch.cuda.empty_cache()
    if loops:
        result["quality"] = loops

    if args.bench_json:
        result["bench_py"] = _last_json_line(args.bench_json)
    if args.bench_parent_json:
        result["bench_py_parent"] = _last_json_line(args.bench_parent_json)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
