#!/usr/bin/env python
"""Times the K = 7 Viterbi decoder (mimo_fec_decode) on the bench's C3 batch, the batch of
bench_sic_soft_fb.py: 64 synthetic captures at 30 dB, 4x4 MMSE, 2048-pt FFT, 64-QAM, max_out
1000, symbol-major output. A codeword is one row of the LLR buffer (one stream's symbol,
M_occ * 6 values), so the batch is captures * max_out * 4 rows.

Timing: mimo_rx_soft_demap's int8 LLRs at llr_scale 4 are decoded per rate (1/2, 2/3, 3/4): one
warm-up, then `--reps` launches timed with HIP events on the receiver's stream, repeated
`--rounds` times (median and spread reported). Per rate: ms per launch, rows per second, info
Gbit/s, and wave-cycles per trellis step = ms * clock * waves in the grid / (rows * T), at the
device's maximum clock of 2.4 GHz (`--clock-ghz`; the clock under load is lower, so are the cycles).
The same at rate 1/2 for other persistent-grid sizes (`--waves`, waves per CU through
RMIMO_FEC_WAVES, read at a handle's first decode).

Errors: the synthesiser sends random indices, so the code's linearity is used. Per row, x the
transmitted bits, c the encoding of randomly chosen info bits: the LLR is negated on the device
wherever x ^ c is 1 (int8 LLRs of the soft passes are never -128), and the decoder must return
the chosen info bits. Per soft pass (mimo_rx_soft_demap, mimo_rx_sic_soft, mimo_rx_sic_soft_fb)
and rate, over the rows the decode wrote: info-bit errors after decoding beside the uncoded bit
errors of the same rows at the positions the code uses (hard decision of the LLR: bit 1 where it
is negative).

`--bench-json` and `--bench-parent-json` name files that hold the JSON line of one
`bench.py --gpus 1 --steps 20 --warmup 5` run of this build and of the parent commit's; both
are copied into the result. Writes one JSON file (default profiles/r12/fec_c3.json) and prints
it.
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
    ap.add_argument("--steps", type=int, default=10, help="batch steps timed for ms_per_step")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--snr-db", type=float, default=30.0)
    ap.add_argument("--llr-scale", type=float, default=4.0)
    ap.add_argument("--waves", default="8,32", help="other waves-per-CU grid sizes to time")
    ap.add_argument("--clock-ghz", type=float, default=2.4,
                    help="clock the wave-cycle figure assumes (the MI355X maximum)")
    ap.add_argument("--bench-json", default=None)
    ap.add_argument("--bench-parent-json", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "fec_c3.json"))
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

    nb = 2 * soft.qam_bits(qam)
    n_c = m_occ * nb
    rows_f = pid * N                                   # rows per capture
    n_rows = F * rows_f
    props = torch.cuda.get_device_properties(dev)
    n_cu = props.multi_processor_count
    clock_hz = args.clock_ghz * 1e9
    llr8 = torch.empty((F, pid, N, m_occ, nb), dtype=torch.int8, device=dev)
    z_idx = torch.empty((F, pid, N, m_occ), dtype=torch.uint8, device=dev)
    kw = dict(max_out=pid, out_layout=layout, stream=sh)
    sc = args.llr_scale
    rx.soft_demap(out_sym, llr8, fmt=_lib.LLR_I8, llr_scale=sc, **kw)
    torch.cuda.synchronize()

    result = {
        "config": {"M": M, "cp": cp, "streams": N, "access_codes": nac, "qam": qam,
                   "detector": "mmse", "captures": F, "max_out": pid, "out_layout": "symbol",
                   "snr_db": args.snr_db, "llr_scale": sc, "reps": args.reps,
                   "rounds": args.rounds},
        "device": torch.cuda.get_device_name(dev),
        "compute_units": n_cu,
        "assumed_clock_hz": clock_hz,
        "frames_synced": synced,
        "rows": n_rows,
        "n_c": n_c,
        "ms_per_step": ms_step,
        "live_capture_rows_per_s": 20e6 / (M + cp) * N,
        "rates": {},
    }
    names = {fec.R12: "1/2", fec.R23: "2/3", fec.R34: "3/4"}

    def time_decode(rate, waves_per_cu=None):
        if waves_per_cu is None:
            os.environ.pop("RMIMO_FEC_WAVES", None)
        else:
            os.environ["RMIMO_FEC_WAVES"] = str(waves_per_cu)
        f = fec.Fec(rate, n_c)
        pitch = f.min_pitch()
        bits = torch.empty((n_rows, pitch), dtype=torch.uint8, device=dev)
        metric = torch.empty(n_rows, dtype=torch.int32, device=dev)
        r = rounds(lambda: f.decode(llr8, n_rows, bits, pitch, metric, stream=sh))
        os.environ.pop("RMIMO_FEC_WAVES", None)
        s = r["ms_per_launch"] * 1e-3
        wpc = 16 if waves_per_cu is None else waves_per_cu
        r.update({"steps": f.steps, "n_info": f.n_info, "waves_per_cu": wpc,
                  "rows_per_s": n_rows / s,
                  "info_gbit_per_s": n_rows * f.n_info / s / 1e9,
                  "wave_cycles_per_step": s * clock_hz * min(n_cu * wpc, n_rows) /
                  (n_rows * f.steps),
                  "fraction_of_step": r["ms_per_launch"] / ms_step,
                  "times_live_capture_rate": n_rows / s / result["live_capture_rows_per_s"]})
        return r

    for rate in fec.RATES:
        result["rates"][names[rate]] = time_decode(rate)
    result["grid_sweep_rate_1/2"] = {str(w): time_decode(fec.R12, int(w))
                                     for w in args.waves.split(",") if w}

    # ---- coded and uncoded errors per soft pass and rate, one capture's rows at a time ----
    shifts = torch.arange(nb - 1, -1, -1, device=dev, dtype=torch.int32)
    n_out = [min(r["n_sym"], pid) if r["status"] == _lib.FRAME_OK else 0 for r in res]
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    codes = {}
    for rate in fec.RATES:
        f = fec.Fec(rate, n_c)
        pA, pB = fec.positions(rate, n_c)
        codes[rate] = dict(
            f=f, pitch=f.min_pitch(),
            keepA=torch.from_numpy(np.flatnonzero(pA >= 0)).to(dev),
            keepB=torch.from_numpy(np.flatnonzero(pB >= 0)).to(dev),
            pA=torch.from_numpy(pA[pA >= 0]).to(dev), pB=torch.from_numpy(pB[pB >= 0]).to(dev),
            bits=torch.empty((rows_f, f.min_pitch()), dtype=torch.uint8, device=dev))
    bit_w = torch.arange(7, -1, -1, device=dev, dtype=torch.int32)
    flipped = torch.empty((rows_f, n_c), dtype=torch.int8, device=dev)

    def encode_dev(info, k):
        f = k["f"]
        T = f.steps
        u = torch.zeros((info.shape[0], T + 6), dtype=torch.uint8, device=dev)
        u[:, 6:6 + f.n_info] = info
        at = lambda d: u[:, 6 - d:6 - d + T]
        A = at(0) ^ at(2) ^ at(3) ^ at(5) ^ at(6)
        B = at(0) ^ at(1) ^ at(2) ^ at(3) ^ at(6)
        row = torch.zeros((info.shape[0], n_c), dtype=torch.uint8, device=dev)
        row[:, k["pA"]] = A[:, k["keepA"]]
        row[:, k["pB"]] = B[:, k["keepB"]]
        return row

    def errors():
        """info-bit errors after decoding and uncoded errors at the used positions, per rate,
        over the written rows of the LLRs now in llr8"""
        acc = {names[r]: {"coded_errors": 0, "info_bits": 0, "uncoded_errors": 0,
                          "coded_bits": 0, "rows": 0, "rows_in_error": 0} for r in fec.RATES}
        with torch.cuda.stream(stream):
            for fr in range(F):
                n = n_out[fr]
                if n == 0:
                    continue
                sent = tx_idx[fr, :, :n].permute(1, 0, 2).to(torch.int32)     # [n][N][M_occ]
                x = ((sent[..., None] >> shifts) & 1).to(torch.uint8).reshape(n * N, n_c)
                v = llr8[fr, :n].reshape(n * N, n_c)
                for rate in fec.RATES:
                    k, a = codes[rate], acc[names[rate]]
                    f = k["f"]
                    info = torch.randint(0, 2, (n * N, f.n_info), dtype=torch.uint8, device=dev,
                                         generator=gen)
                    c = encode_dev(info, k)
                    w = flipped[:n * N]
                    torch.where((x ^ c) == 1, -v, v, out=w)
                    f.decode(w, n * N, k["bits"], k["pitch"], None, stream=sh)
                    dec = ((k["bits"][:n * N].to(torch.int32)[..., None] >> bit_w) & 1)
                    dec = dec.reshape(n * N, -1)[:, :f.n_info]
                    bad = dec != info
                    used = torch.cat([k["pA"], k["pB"]])
                    a["coded_errors"] += int(bad.sum())
                    a["rows_in_error"] += int(bad.any(dim=1).sum())
                    a["info_bits"] += n * N * f.n_info
                    a["uncoded_errors"] += int(((w[:, used] < 0) != (c[:, used] == 1)).sum())
                    a["coded_bits"] += n * N * f.n_tx
                    a["rows"] += n * N
        return acc

    result["errors"] = {"soft_demap": errors()}
    rx.sic_soft(out_sym, llr8, None, z_idx, fmt=_lib.LLR_I8, llr_scale=sc, **kw)
    torch.cuda.synchronize()
    result["errors"]["sic_soft"] = errors()
    rx.sic_soft_fb(out_sym, llr8, None, z_idx, fmt=_lib.LLR_I8, llr_scale=sc, **kw)
    torch.cuda.synchronize()
    result["errors"]["sic_soft_fb"] = errors()

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
