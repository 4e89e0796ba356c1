#!/usr/bin/env python
"""Times the soft-feedback SIC pass (mimo_rx_sic_soft_fb) on the bench's C3 batch, the batch of
bench_sic_soft.py: 64 synthetic captures at 30 dB, 4x4 MMSE, 2048-pt FFT, 64-QAM, max_out
1000, symbol-major output.

Per form (int8 LLRs + idx, int8 LLRs only, fp32 LLRs + idx) of mimo_rx_sic_soft_fb, and for
mimo_rx_sic_soft int8 + idx beside them in the same process: one warm-up, then `--reps`
launches timed with HIP events on the receiver's stream, repeated `--rounds` times (median and
spread reported). Each launch is the table kernel plus the symbol kernel, as a caller pays it.
`fb_over_sic_soft` is the int8 + idx time of the new call over mimo_rx_sic_soft's.

Then the generalised mutual information per bit (sic.llr_gmi's definition, evaluated on the
device) of three int8 outputs at `--gmi-scale` against the synthesiser's transmitted indices,
over the rows the decode wrote: mimo_rx_soft_demap (the linear detector), mimo_rx_sic_soft and
mimo_rx_sic_soft_fb. The int8 value q stands for the LLR q / scale: at the default scale 4 the
step is 0.25 and the clamp +-31.75.

`--bench-json` and `--bench-parent-json` name files that hold the JSON line of one
`bench.py --gpus 1 --steps 20 --warmup 5` run of this build and of the parent commit's; both
are copied into the result, to show the batch step beside them.
Writes one JSON file (default profiles/r11/sic_soft_fb_c3.json) and prints it.
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="batch steps timed for ms_per_step")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--snr-db", type=float, default=30.0)
    ap.add_argument("--gmi-scale", type=float, default=4.0)
    ap.add_argument("--bench-json", default=None)
    ap.add_argument("--bench-parent-json", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "sic_soft_fb_c3.json"))
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
    z_idx = torch.empty((F, pid, N, m_occ), dtype=torch.uint8, device=dev)
    llr8 = torch.empty((F, pid, N, m_occ, nb), dtype=torch.int8, device=dev)
    result = {
        "config": {"M": M, "cp": cp, "streams": N, "access_codes": nac, "qam": qam,
                   "detector": "mmse", "captures": F, "max_out": pid, "out_layout": "symbol",
                   "snr_db": args.snr_db, "reps": args.reps, "rounds": args.rounds},
        "device": torch.cuda.get_device_name(dev),
        "frames_synced": synced,
        "symbols": n_sym,
        "ms_per_step": ms_step,
        "forms": {},
    }
    kw = dict(max_out=pid, out_layout=layout, stream=sh)

    def form(name, fn):
        r = rounds(fn)
        r["fraction_of_step"] = r["ms_per_launch"] / ms_step
        result["forms"][name] = r

    form("sic_soft_int8_idx", lambda: rx.sic_soft(out_sym, llr8, None, z_idx, fmt=_lib.LLR_I8,
                                                  llr_scale=0.05, **kw))
    form("sic_soft_fb_int8_idx", lambda: rx.sic_soft_fb(out_sym, llr8, None, z_idx,
                                                        fmt=_lib.LLR_I8, llr_scale=0.05, **kw))
    form("sic_soft_fb_int8_only", lambda: rx.sic_soft_fb(out_sym, llr8, None, None,
                                                         fmt=_lib.LLR_I8, llr_scale=0.05, **kw))
    llr32 = torch.empty((F, pid, N, m_occ, nb), dtype=torch.float32, device=dev)
    form("sic_soft_fb_fp32_idx", lambda: rx.sic_soft_fb(out_sym, llr32, None, z_idx,
                                                        fmt=_lib.LLR_F32, llr_scale=0.05, **kw))
    del llr32
    torch.cuda.synchronize()
    fm = result["forms"]
    result["fb_over_sic_soft"] = (fm["sic_soft_fb_int8_idx"]["ms_per_launch"] /
                                  fm["sic_soft_int8_idx"]["ms_per_launch"])

    # GMI per bit of the three int8 outputs against the transmitted indices
    sc = args.gmi_scale
    shifts = torch.arange(nb - 1, -1, -1, device=dev, dtype=torch.int32)

    def gmi():
        torch.cuda.synchronize()
        tot, cnt = 0.0, 0
        for f, r in enumerate(res):
            n = min(r["n_sym"], pid) if r["status"] == _lib.FRAME_OK else 0
            if n == 0:
                continue
            sent = tx_idx[f, :, :n].permute(1, 0, 2).to(torch.int32)          # [n][N][M_occ]
            bits = (sent[..., None] >> shifts) & 1
            v = llr8[f, :n].to(torch.float64) / sc
            tot += float(torch.nn.functional.softplus(torch.where(bits == 1, v, -v)).sum())
            cnt += v.numel()
        return 1.0 - tot / cnt / 0.6931471805599453

    g = {"llr_scale": sc, "snr_db": args.snr_db}
    rx.soft_demap(out_sym, llr8, fmt=_lib.LLR_I8, llr_scale=sc, **kw)
    g["soft_demap"] = gmi()
    rx.sic_soft(out_sym, llr8, None, z_idx, fmt=_lib.LLR_I8, llr_scale=sc, **kw)
    g["sic_soft"] = gmi()
    sent_all = tx_idx.permute(0, 2, 1, 3)
    nrow = torch.tensor([min(r["n_sym"], pid) if r["status"] == _lib.FRAME_OK else 0
                         for r in res], device=dev)
    rows = (torch.arange(pid, device=dev)[None, :] < nrow[:, None])[:, :, None, None]
    g["sic_soft_symbol_errors"] = int(((z_idx != sent_all) & rows).sum())
    rx.sic_soft_fb(out_sym, llr8, None, z_idx, fmt=_lib.LLR_I8, llr_scale=sc, **kw)
    g["sic_soft_fb"] = gmi()
    g["sic_soft_fb_symbol_errors"] = int(((z_idx != sent_all) & rows).sum())
    g["symbols_in_written_rows"] = int(nrow.sum()) * N * m_occ
    result["gmi_per_bit_int8"] = g
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
