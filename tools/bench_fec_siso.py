#!/usr/bin/env python
"""Times the soft-output (max-log-MAP) decoder (mimo_fec_siso) beside the Viterbi decoder
(mimo_fec_decode) on the bench's C3 batch, the batch of bench_fec.py: 64 synthetic captures at
30 dB, 4x4 MMSE, 2048-pt FFT, 64-QAM, max_out 1000, symbol-major output. A codeword is one row
of the LLR buffer (one stream's symbol, M_occ * 6 values), so the batch is captures * max_out * 4
rows of mimo_rx_soft_demap's int8 LLRs at llr_scale 4.

Timing, per rate (1/2, 2/3, 3/4): mimo_fec_decode, then mimo_fec_siso with d_out only (APP),
with d_out, bits, info LLRs and metric (APP), and with d_out only (EXT). One warm-up, then
`--reps` launches timed with HIP events on the receiver's stream, repeated `--rounds` times
(median and spread reported). Per case: ms per launch, rows per second, the multiple of the
Viterbi time, and wave-cycles per trellis step = ms * clock * waves in the grid / (rows * T), at
the device's maximum clock of 2.4 GHz (`--clock-ghz`; the clock under load is lower, so are the
cycles). The d_out-only APP case at rate 1/2 again for other persistent-grid sizes (`--waves`,
waves per CU through RMIMO_FEC_WAVES, read at a handle's first call).

Correction run: the synthesiser sends random indices, so the code's linearity is used as in
bench_fec.py (the LLR is negated wherever transmitted bit ^ codeword bit is 1). Per rate, over
the rows the decode wrote: info-bit errors and rows in error of mimo_fec_siso's d_bits beside
mimo_fec_decode's (they differ only through ties), and over the coded positions the code uses:
hard-decision errors of the input LLR, of the APP, and the positions the APP corrects and breaks
relative to the input's sign (an LLR or APP of 0 counts as bit 0). Recorded as measured.

`--bench-json` and `--bench-parent-json` name files that hold the JSON line of one
`bench.py --gpus 1 --steps 20 --warmup 5` run of this build and of the parent commit's; both
are copied into the result. Writes one JSON file (default profiles/r13/fec_siso_c3.json) and
prints it.
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--snr-db", type=float, default=30.0)
    ap.add_argument("--llr-scale", type=float, default=4.0)
    ap.add_argument("--waves", default="8,16,32", help="waves-per-CU grid sizes to time")
    ap.add_argument("--clock-ghz", type=float, default=2.4,
                    help="clock the wave-cycle figure assumes (the MI355X maximum)")
    ap.add_argument("--skip-correction", action="store_true", help="timing only")
    ap.add_argument("--bench-json", default=None)
    ap.add_argument("--bench-parent-json", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "fec_siso_c3.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from rub_mimo_amd import _lib, fec, soft
    from rub_mimo_amd.receiver import Receiver, RxParams, Synthesizer, SynthParams

    M, cp, N, nac, qam, pid, F = 2048, 152, 4, 20, 64, args.pid, args.frames
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.Stream(dev)      # the receiver's launch stream; the events time it
    sh = stream.cuda_stream
    sp = SynthParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid=pid,
                     qam_order=qam, seed=args.seed, snr_db=args.snr_db)
    syn = Synthesizer(sp)
    L = sp.max_frame_len()
    iq = torch.empty((F, N, L), dtype=torch.complex64, device=dev)
    rx = Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                           detector=_lib.DET_MMSE, qam_order=qam), stream=sh)
    m_occ = rx.M_occ
    tx_idx = torch.zeros((F, N, pid, m_occ), dtype=torch.uint8, device=dev)
    syn.generate(iq, L, L, F, tx_idx=tx_idx, stream=sh)
    torch.cuda.synchronize()
    layout = _lib.LAYOUT_SYMBOL_MAJOR
    out_sym = torch.zeros((F, pid, N, m_occ), dtype=torch.complex64, device=dev)
    for _ in range(3):
        rx.process(iq, L, L, F, max_out=pid, out_sym=out_sym, stream=sh, out_layout=layout)
    res = rx.results()
    synced = sum(r["status"] == _lib.FRAME_OK for r in res)

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

    nb = 2 * soft.qam_bits(qam)
    n_c = m_occ * nb
    rows_f = pid * N                                   # rows per capture
    n_rows = F * rows_f
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    clock_hz = args.clock_ghz * 1e9
    llr8 = torch.empty((F, pid, N, m_occ, nb), dtype=torch.int8, device=dev)
    rx.soft_demap(out_sym, llr8, max_out=pid, out_layout=layout, stream=sh, fmt=_lib.LLR_I8,
                  llr_scale=args.llr_scale)
    torch.cuda.synchronize()
    out8 = torch.empty((n_rows, n_c), dtype=torch.int8, device=dev)
    metric = torch.empty(n_rows, dtype=torch.int32, device=dev)

    result = {
        "config": {"M": M, "cp": cp, "streams": N, "access_codes": nac, "qam": qam,
                   "detector": "mmse", "captures": F, "max_out": pid, "out_layout": "symbol",
                   "snr_db": args.snr_db, "llr_scale": args.llr_scale, "reps": args.reps,
                   "rounds": args.rounds},
        "device": torch.cuda.get_device_name(dev),
        "compute_units": n_cu,
        "assumed_clock_hz": clock_hz,
        "frames_synced": synced,
        "rows": n_rows,
        "n_c": n_c,
        "rates": {},
    }
    names = {fec.R12: "1/2", fec.R23: "2/3", fec.R34: "3/4"}

    def figures(r, f, wpc):
        s = r["ms_per_launch"] * 1e-3
        r.update({"steps": f.steps, "waves_per_cu": wpc, "rows_per_s": n_rows / s,
                  "wave_cycles_per_step": s * clock_hz * min(n_cu * wpc, n_rows) /
                  (n_rows * f.steps)})
        return r

    def time_rate(rate, wpc=None, only=None):
        """the four cases of one rate on one handle (`only`: just that case)"""
        if wpc is None:
            os.environ.pop("RMIMO_FEC_WAVES", None)
        else:
            os.environ["RMIMO_FEC_WAVES"] = str(wpc)
        f = fec.Fec(rate, n_c)
        bp, ip = f.min_pitch(), f.min_info_pitch()
        bits = torch.empty((n_rows, bp), dtype=torch.uint8, device=dev)
        info = torch.empty((n_rows, ip), dtype=torch.int8, device=dev)
        cases = {
            "viterbi": lambda: f.decode(llr8, n_rows, bits, bp, metric, stream=sh),
            "siso_app_out": lambda: f.siso(llr8, n_rows, out8, mode=fec.SISO_APP, stream=sh),
            "siso_app_all": lambda: f.siso(llr8, n_rows, out8, bits, info, metric, fec.SISO_APP,
                                           bp, ip, stream=sh),
            "siso_ext_out": lambda: f.siso(llr8, n_rows, out8, mode=fec.SISO_EXT, stream=sh),
        }
        w = 16 if wpc is None else wpc
        got = {k: figures(rounds(fn), f, w) for k, fn in cases.items() if only in (None, k)}
        os.environ.pop("RMIMO_FEC_WAVES", None)
        if "viterbi" in got:
            for k, r in got.items():
                r["times_viterbi"] = r["ms_per_launch"] / got["viterbi"]["ms_per_launch"]
        return got

    for rate in fec.RATES:
        result["rates"][names[rate]] = time_rate(rate)
    result["grid_sweep_rate_1/2_app_out"] = {
        str(w): time_rate(fec.R12, int(w), "siso_app_out")["siso_app_out"]
        for w in args.waves.split(",") if w}

    # ---- correction run: one capture's rows at a time ----
    shifts = torch.arange(nb - 1, -1, -1, device=dev, dtype=torch.int32)
    bit_w = torch.arange(7, -1, -1, device=dev, dtype=torch.int32)
    n_out = [min(r["n_sym"], pid) if r["status"] == _lib.FRAME_OK else 0 for r in res]
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    flipped = torch.empty((rows_f, n_c), dtype=torch.int8, device=dev)
    app = torch.empty((rows_f, n_c), dtype=torch.int8, device=dev)
    corr = {}
    for rate in () if args.skip_correction else fec.RATES:
        f = fec.Fec(rate, n_c)
        T = f.steps
        pA, pB = fec.positions(rate, n_c)
        keepA = torch.from_numpy(np.flatnonzero(pA >= 0)).to(dev)
        keepB = torch.from_numpy(np.flatnonzero(pB >= 0)).to(dev)
        posA = torch.from_numpy(pA[pA >= 0]).to(dev)
        posB = torch.from_numpy(pB[pB >= 0]).to(dev)
        used = torch.cat([posA, posB])
        bp = f.min_pitch()
        vbits = torch.empty((rows_f, bp), dtype=torch.uint8, device=dev)
        sbits = torch.empty((rows_f, bp), dtype=torch.uint8, device=dev)
        a = {k: 0 for k in ("rows", "info_bits", "coded_bits", "viterbi_info_errors",
                            "viterbi_rows_in_error", "siso_info_errors", "siso_rows_in_error",
                            "info_bits_that_differ", "input_coded_errors", "app_coded_errors",
                            "app_corrects", "app_breaks")}

        def unpack(b, n):
            d = ((b[:n].to(torch.int32)[..., None] >> bit_w) & 1)
            return d.reshape(n, -1)[:, :f.n_info]

        with torch.cuda.stream(stream):
            for fr in range(F):
                n = n_out[fr] * N
                if n == 0:
                    continue
                sent = tx_idx[fr, :, :n_out[fr]].permute(1, 0, 2).to(torch.int32)
                x = ((sent[..., None] >> shifts) & 1).to(torch.uint8).reshape(n, n_c)
                v = llr8[fr, :n_out[fr]].reshape(n, n_c)
                info = torch.randint(0, 2, (n, f.n_info), dtype=torch.uint8, device=dev,
                                     generator=gen)
                u = torch.zeros((n, T + 6), dtype=torch.uint8, device=dev)
                u[:, 6:6 + f.n_info] = info
                at = lambda d: u[:, 6 - d:6 - d + T]
                A = at(0) ^ at(2) ^ at(3) ^ at(5) ^ at(6)
                B = at(0) ^ at(1) ^ at(2) ^ at(3) ^ at(6)
                c = torch.zeros((n, n_c), dtype=torch.uint8, device=dev)
                c[:, posA] = A[:, keepA]
                c[:, posB] = B[:, keepB]
                w = flipped[:n]
                torch.where((x ^ c) == 1, -v, v, out=w)
                f.decode(w, n, vbits, bp, None, stream=sh)
                f.siso(w, n, app, sbits, None, None, fec.SISO_APP, bp, stream=sh)
                dv, ds = unpack(vbits, n), unpack(sbits, n)
                bad_v, bad_s = dv != info, ds != info
                cw = c[:, used] == 1
                in_bad = (w[:, used] < 0) != cw
                app_bad = (app[:n][:, used] < 0) != cw
                a["rows"] += n
                a["info_bits"] += n * f.n_info
                a["coded_bits"] += n * f.n_tx
                a["viterbi_info_errors"] += int(bad_v.sum())
                a["viterbi_rows_in_error"] += int(bad_v.any(dim=1).sum())
                a["siso_info_errors"] += int(bad_s.sum())
                a["siso_rows_in_error"] += int(bad_s.any(dim=1).sum())
                a["info_bits_that_differ"] += int((dv != ds).sum())
                a["input_coded_errors"] += int(in_bad.sum())
                a["app_coded_errors"] += int(app_bad.sum())
                a["app_corrects"] += int((in_bad & ~app_bad).sum())
                a["app_breaks"] += int((~in_bad & app_bad).sum())
        a["share_of_coded_positions_corrected"] = a["app_corrects"] / max(a["coded_bits"], 1)
        corr[names[rate]] = a
    result["correction_soft_demap"] = corr

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
