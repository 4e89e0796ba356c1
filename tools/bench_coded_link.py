#!/usr/bin/env python
"""Times the device encoder (mimo_fec_encode_rows) at the C3 x 64 shape and runs the detector /
decoder loop of bench_pic.py on frames that carry encoded payloads. Nothing is asserted: every
figure is recorded as measured.

Encoder: 256 000 rows (64 captures x 4 streams x 1000 symbols) of n_c = 12 288 (M_occ 2048,
64-QAM), rates 1/2, 2/3 and 3/4, both output forms (0/1 bytes; QAM indices at b = 3), perm NULL
and a seeded random perm. One warm-up, then `--reps` launches timed with HIP events on one
stream, repeated `--rounds` times (median and spread). Bytes moved per launch are the packed info
bytes read plus the output bytes written (the inverse position map, 24 KiB, stays in cache and is
not counted). The first two rows of every form are compared with the numpy model. The int8 soft
demap (mimo_rx_soft_demap) is timed in the same process on the C3 batch as the yardstick of "one
pass over the same rows". `--bench-full-json` names a file with the JSON line of one
`bench.py --gpus 1 --full` run on the same box; its roofline block (the decode's achieved HBM
rate and the rate of the decode's memory pattern alone) is copied beside the encoder's rates.

Loop: bench_pic.py's, unchanged in shape (`--loop-frames` captures of `--loop-pid` symbols, 4x4
MMSE, 64-QAM, plateau threshold 0.85, rate 1/2 at 18 dB and rate 3/4 at 22 dB, three passes of
mimo_rx_pic_soft -> mimo_fec_siso (extrinsic) -> priors, at prior_scale = llr_scale and
llr_scale / 0.7). One codeword per (stream, symbol) row, made by the device encoder in QAM form.
Two forms from the same info bits, codewords, seed, channels and noise:
  encoded_payload: the frames carry the codewords (mimo_synth_frames_payload); the detector's
    LLRs go to the decoder as they are;
  sign_flip: the frames carry the synthesiser's hash-drawn bits x (mimo_synth_frames) and the
    LLRs are flipped by x ^ c, bench_pic.py's form.
Per pass: info-bit errors, rows in error, and the GMI per bit of the detector's int8 LLRs.

`--bench-json` and `--bench-parent-json` name files that hold the JSON line of one
`bench.py --gpus 1 --steps 20 --warmup 5` run of this build and of the parent commit's; both are
copied into the result. Writes one JSON file (default profiles/r16/coded_link_c3.json).
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
    ap.add_argument("--bench-full-json", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "coded_link_c3.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from rub_mimo_amd import _lib, fec, soft
    from rub_mimo_amd.receiver import Receiver, RxParams, Synthesizer, SynthParams

    M, cp, N, nac, qam = 2048, 152, 4, 20, 64
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.Stream(dev)
    sh = stream.cuda_stream
    layout = _lib.LAYOUT_SYMBOL_MAJOR
    b = soft.qam_bits(qam)
    nb = 2 * b
    sc = args.llr_scale
    result = {"device": torch.cuda.get_device_name(dev)}

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

    def receiver(pid, threshold=None):
        kw = {} if threshold is None else {"plateau_threshold": threshold}
        return Receiver(RxParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid_max=pid,
                                 detector=_lib.DET_MMSE, qam_order=qam, **kw), stream=sh)

    def synth(pid, snr_db):
        sp = SynthParams(M=M, cp_len=cp, num_streams=N, num_access_codes=nac, pid=pid,
                         qam_order=qam, seed=args.seed, snr_db=snr_db)
        return Synthesizer(sp), sp.max_frame_len()

    def pack(info, pitch):
        """[rows][n_info] 0/1 -> [rows][pitch] uint8, MSB first (the d_bits format)."""
        rows, n = info.shape
        full = torch.zeros((rows, 8 * pitch), dtype=torch.uint8, device=dev)
        full[:, :n] = info
        w = torch.tensor([128, 64, 32, 16, 8, 4, 2, 1], dtype=torch.uint8, device=dev)
        return (full.reshape(rows, pitch, 8) * w).sum(dim=2, dtype=torch.int32).to(torch.uint8)

    # ---- timing at the C3 x 64 shape ----
    if not args.skip_timing:
        F, pid = args.frames, args.pid
        rows, n_c = F * N * pid, M * nb
        gen = torch.Generator(device=dev)
        gen.manual_seed(args.seed)
        rng = np.random.default_rng(args.seed)
        out_bits = torch.empty((rows, n_c), dtype=torch.uint8, device=dev)
        out_qam = torch.empty((rows, n_c // nb), dtype=torch.uint8, device=dev)
        enc = {}
        for rate, rname in ((fec.R12, "1/2"), (fec.R23, "2/3"), (fec.R34, "3/4")):
            T, n_info, ntx = fec.geometry(rate, n_c)
            pitch = fec.min_pitch(n_info)
            info = torch.randint(0, 256, (rows, pitch), dtype=torch.uint8, device=dev,
                                 generator=gen)
            head = info[:2].cpu().numpy()
            for pname, perm in (("perm_null", None),
                                ("perm_random", rng.permutation(n_c)[:ntx].astype(np.uint16))):
                code = fec.Fec(rate, n_c, perm)
                for fname, form, qb, out in (("bits", fec.ENC_BITS, 0, out_bits),
                                             ("qam_b3", fec.ENC_QAM, b, out_qam)):
                    r = rounds(lambda: code.encode_rows(info, rows, out, form=form, qam_bits=qb,
                                                        bits_pitch=pitch, stream=sh))
                    moved = rows * ((n_info + 7) // 8 + out.shape[1])
                    r["bytes_moved"] = moved
                    r["gb_per_s"] = moved / (r["ms_per_launch"] * 1e-3) / 1e9
                    r["coded_bits_per_s"] = rows * ntx / (r["ms_per_launch"] * 1e-3)
                    r["first_rows_equal_model"] = bool(np.array_equal(
                        out[:2].cpu().numpy(),
                        fec.encode_rows(rate, n_c, head, perm, form=form, qam_bits=qb)))
                    enc["rate %s %s %s" % (rname, fname, pname)] = r
        del out_bits, out_qam, info
        torch.cuda.empty_cache()
        # the yardstick: the int8 soft demap over the same rows, on the C3 batch
        syn, L = synth(pid, args.snr_db)
        rx = receiver(pid)
        iq = torch.empty((F, N, L), dtype=torch.complex64, device=dev)
        syn.generate(iq, L, L, F, stream=sh)
        out_sym = torch.zeros((F, pid, N, rx.M_occ), dtype=torch.complex64, device=dev)
        torch.cuda.synchronize()
        for _ in range(3):          # (the second identical call captures the batch graph)
            rx.process(iq, L, L, F, max_out=pid, out_sym=out_sym, stream=sh, out_layout=layout)
        res = rx.results()
        llr8 = torch.empty((F, pid, N, rx.M_occ, nb), dtype=torch.int8, device=dev)
        demap = rounds(lambda: rx.soft_demap(out_sym, llr8, max_out=pid, out_layout=layout,
                                             stream=sh, fmt=_lib.LLR_I8, llr_scale=sc))
        demap["bytes_moved"] = rows * M * (8 + nb)
        demap["gb_per_s"] = demap["bytes_moved"] / (demap["ms_per_launch"] * 1e-3) / 1e9
        demap["frames_synced"] = sum(r["status"] == _lib.FRAME_OK for r in res)
        result["timing"] = {
            "config": {"rows": rows, "n_c": n_c, "captures": F, "streams": N, "max_out": pid,
                       "M_occ": M, "qam": qam, "reps": args.reps, "rounds": args.rounds},
            "encoder": enc, "soft_demap_int8": demap,
            "counters": "not taken: the rates below are event times over counted bytes",
        }
        del rx, iq, out_sym, llr8
        torch.cuda.empty_cache()

    # ---- the loop ----
    snrs = [float(v) for v in args.loop_snr_db.split(",")]
    loops = {}
    for rate, name, snr in () if args.skip_loop else ((fec.R12, "1/2", snrs[0]),
                                                      (fec.R34, "3/4", snrs[-1])):
        F, pid = args.loop_frames, args.loop_pid
        n_c, rows = M * nb, F * pid * N
        code = fec.Fec(rate, n_c)
        gen = torch.Generator(device=dev)
        gen.manual_seed(args.seed)
        # payload order [F][N][pid]; the loop's rows are symbol-major, [F][pid][N]
        info_p = torch.randint(0, 2, (F, N, pid, code.n_info), dtype=torch.uint8, device=dev,
                               generator=gen)
        info = info_p.permute(0, 2, 1, 3).reshape(rows, code.n_info)
        tx_pay = torch.empty((F, N, pid, M), dtype=torch.uint8, device=dev)
        packed = pack(info_p.reshape(rows, code.n_info), code.min_pitch())
        torch.cuda.synchronize()
        code.encode_rows(packed, rows, tx_pay, form=fec.ENC_QAM, qam_bits=b, stream=sh)
        torch.cuda.synchronize()
        shifts = torch.arange(nb - 1, -1, -1, device=dev, dtype=torch.int32)

        def bits_of(idx):               # [F][N][pid][M] indices -> [rows][n_c] in the loop's order
            v = idx.permute(0, 2, 1, 3).to(torch.int32)
            return ((v[..., None] >> shifts) & 1).to(torch.uint8).reshape(rows, n_c)

        syn, L = synth(pid, snr)
        forms = {}
        for fname in ("encoded_payload", "sign_flip"):
            rx = receiver(pid, 0.85)
            iq = torch.empty((F, N, L), dtype=torch.complex64, device=dev)
            tx_idx = torch.zeros((F, N, pid, M), dtype=torch.uint8, device=dev)
            if fname == "encoded_payload":
                syn.generate_payload(iq, L, L, F, tx_pay, stream=sh)
                tx_idx.copy_(tx_pay)
            else:
                syn.generate(iq, L, L, F, tx_idx=tx_idx, stream=sh)
            out_sym = torch.zeros((F, pid, N, M), dtype=torch.complex64, device=dev)
            torch.cuda.synchronize()
            rx.process(iq, L, L, F, max_out=pid, out_sym=out_sym, stream=sh, out_layout=layout)
            res = rx.results()
            n_out = torch.tensor([min(r["n_sym"], pid) if r["status"] == _lib.FRAME_OK else 0
                                  for r in res], device=dev)
            live = (torch.arange(pid, device=dev)[None, :] < n_out[:, None])[:, :, None] \
                .expand(F, pid, N).reshape(rows)
            with torch.cuda.stream(stream):
                c = bits_of(tx_pay)
                x = bits_of(tx_idx)
                flip = (x ^ c) == 1
            llr8 = torch.empty((rows, n_c), dtype=torch.int8, device=dev)
            dec_in = torch.empty((rows, n_c), dtype=torch.int8, device=dev)
            ext = torch.zeros((rows, n_c), dtype=torch.int8, device=dev)
            prior = torch.empty((rows, n_c), dtype=torch.int8, device=dev)
            il = torch.empty((rows, code.min_info_pitch()), dtype=torch.int8, device=dev)
            kw = dict(max_out=pid, out_layout=layout, stream=sh, fmt=_lib.LLR_I8, llr_scale=sc)
            runs = {}
            with torch.cuda.stream(stream):
                for tag, ps in (("prior_scale=llr_scale", sc),
                                ("prior_scale=llr_scale/0.7", sc / 0.7)):
                    passes, p = [], None
                    for _ in range(3):
                        rx.pic_soft(out_sym, llr8, p, prior_scale=ps, **kw)
                        v = llr8.to(torch.float64) / sc
                        lo = torch.nn.functional.softplus(torch.where(x == 1, v, -v))[live]
                        gmi = 1.0 - float(lo.mean()) / 0.6931471805599453
                        torch.where(flip, -llr8, llr8, out=dec_in)
                        ext.zero_()
                        code.siso(dec_in, rows, ext, None, il, None, fec.SISO_EXT, stream=sh)
                        bad = ((il[:, :code.n_info] < 0) != (info == 1)) & live[:, None]
                        passes.append({"info_bit_errors": int(bad.sum()),
                                       "rows_in_error": int(bad.any(dim=1).sum()),
                                       "gmi_per_bit_detector_int8": gmi})
                        torch.where(flip, -ext, ext, out=prior)
                        p = prior
                    runs[tag] = passes
            forms[fname] = {"frames_synced": int((n_out > 0).sum()), "rows": int(live.sum()),
                            "info_bits": int(live.sum()) * code.n_info,
                            "flipped_llrs": int(flip.sum()), "runs": runs}
            del rx, iq, out_sym, llr8, dec_in, ext, prior, flip, x, c
            torch.cuda.empty_cache()
        loops[name] = {"snr_db": snr, "captures": F, "max_out": pid, "llr_scale": sc, "n_c": n_c,
                       "forms": forms}
    if loops:
        result["loop"] = loops

    if args.bench_full_json:
        full = _last_json_line(args.bench_full_json)
        result["bench_py_full_roofline"] = full.get("roofline")
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
