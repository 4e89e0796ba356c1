// rub_mimo_amd/csrc/engine_stages.cpp -- workspace growth and the three stage drivers both
// receive paths share: run_sync (S&C + plateau), run_estimate (search, LS, weights) and
// run_decode (replay decode + EVM). Each fills kernel arguments, launches, and marks the stage
// timer; every input of a call is an argument.
#include "engine_internal.hpp"

namespace mimo {

// Per-frame arrays grow with F; the per-chunk trigger records grow with F * chunks. A
// growing single-frame record array (streaming capture) keeps its earlier records: chunks
// already final are never recomputed, and trig[] is untouched when only the capture grows.
int ensure_workspace(mimo_rx *h, uint32_t F, uint64_t chunks) {
  Workspace &w = h->ws;
  if (F > w.rec_frames) {
    HIPCHK(w.grow(w.trig, F));
    HIPCHK(w.grow(w.keys, (size_t)F * h->N * h->n_slots));
    HIPCHK(w.grow(w.info, F));
    HIPCHK(w.grow(w.G, (size_t)F * h->M * h->N * h->N));
    HIPCHK(w.grow(w.W, (size_t)F * h->M * h->N * h->N));
    HIPCHK(w.grow(w.gain, (size_t)F * h->M));
    HIPCHK(w.grow(w.nvp, (size_t)F * h->N * h->N * ((h->M + 255) / 256)));   // ls_combine blocks
    HIPCHK(w.grow(w.evm_out, (size_t)F * h->N * 3));
    HIPCHK(w.grow(w.evm_chunk, (size_t)F * kEvmChunks * h->N * 3));
    HIPCHK(w.grow(w.evm_cnt, F));
    HIPCHK(w.grow(w.nrec, F));
    HIPCHK(hipMemset(w.evm_cnt.p, 0, sizeof(uint32_t) * F));
    w.rec_frames = F;
    HIPCHK(w.grow(w.rec, (size_t)F * w.rec_stride));
  }
  if (chunks > w.rec_stride) {
    const uint64_t nc = std::max<uint64_t>(chunks, w.rec_stride * 2);
    ScRecord *np = nullptr;
    HIPCHK(hipMalloc(&np, sizeof(ScRecord) * (size_t)w.rec_frames * nc));
    // frame 0's records survive: the streaming execute path (one frame) never recomputes a
    // final chunk, whatever batch sizes the handle ran before
    if (w.rec.p && w.rec_stride)
      HIPCHK(hipMemcpy(np, w.rec.p, sizeof(ScRecord) * w.rec_stride, hipMemcpyDeviceToDevice));
    w.rec.adopt(np, (size_t)w.rec_frames * nc);
    w.gen++;
    w.rec_stride = nc;
  }
  return MIMO_OK;
}

// Decision band of the fp64 S&C metric: a first-order bound on |y_fp32 - y| for the oracle's
// sequential fp32 sums (framing.cc:626-637), for y <= 1 (|P| <= R always):
//   |dy| <= 2 sqrt(2) (M/2 + 2) u sqrt(y) + 2 (M + 1) u y + 4 u y,   u = 2^-24,
// with a 25% margin for the neglected O((M u)^2) terms. Outside the band the fp64 decision
// equals the oracle's; inside it the sample is recomputed exactly.
double sc_band(uint32_t M) {
  const double u = 0x1p-24;
  return 1.25 * u * (std::sqrt(2.0) * (M + 4.0) + 2.0 * M + 6.0);
}

// with q.fpc > 1 frames per capture the stream walk assigns F * fpc frame slots
int run_sync(mimo_rx *h, const Capture &c, uint32_t F, const SyncRequest &q, hipStream_t s) {
  const uint64_t K = sc_chunk_len(h->cp);
  const uint64_t nchunks = (c.frame_len + K - 1) / K, chunk_lo = q.chunk_lo;
  const uint32_t fpc = q.fpc;
  const bool stream = fpc > 1;
  Workspace &w = h->ws;
  int rc = ensure_workspace(h, F * fpc, nchunks);
  if (rc) return rc;
  FillArgs fa{};
  auto add_fill = [&fa](void *p, uint64_t bytes, uint32_t v) {
    fa.p[fa.count] = reinterpret_cast<uint32_t *>(p);
    fa.n[fa.count] = bytes / 4;
    fa.v[fa.count] = v;
    fa.count++;
  };
  if (q.reset_trig) add_fill(w.trig.p, sizeof(unsigned long long) * F, 0xFFFFFFFFu);
  // the search's argmax keys, zeroed here instead of by a memset ahead of the search
  if (q.zero_keys) add_fill(w.keys.p, sizeof(unsigned long long) * F * fpc * h->N * h->n_slots, 0u);
  if (stream) {
    HIPCHK(w.grow(w.cand, (size_t)F * nchunks));
    HIPCHK(w.grow(w.certfail, F));
    add_fill(w.cand.p, sizeof(unsigned long long) * F * nchunks, 0xFFFFFFFFu);
    add_fill(w.certfail.p, sizeof(unsigned long long) * F, 0u);
  }
  if (chunk_lo >= nchunks) launch_fill(fa, s);
  if (chunk_lo < nchunks) {
    ScArgs a{};
    set_capture(a, c);
    a.N = h->N; a.M = h->M; a.cp = h->cp;
    a.thr = h->thr;
    a.band = sc_band(h->M);
    a.diag = (uint32_t)diag_env().sc_diag;
    a.chunk_len = K; a.chunk_lo = chunk_lo; a.chunk_hi = nchunks;
    a.trig = w.trig.p; a.rec = w.rec.p; a.rec_stride = w.rec_stride;
    a.cand = stream ? w.cand.p : nullptr;
    a.no_skip = stream ? 1 : 0;
    if (!w.n_exact.p) {
      HIPCHK(w.grow(w.n_exact, 1));
      HIPCHK(hipMemsetAsync(w.n_exact.p, 0, sizeof(unsigned long long), s));
    }
    a.n_exact = w.n_exact.p;
    if (!w.queue.p) HIPCHK(w.grow(w.queue, 3));
    add_fill(w.queue.p, 3 * sizeof(uint32_t), 0u);
    a.queue = w.queue.p;
    a.hot_count = w.queue.p + 1;
    // screened path where the geometry allows it (else the per-chunk item kernel): one hot item
    // per listed chunk
    const bool screen = sc_screen_ok(h->M);
    const uint64_t n_list = (nchunks - chunk_lo) * (uint64_t)F;
    const uint32_t hot_cap = screen ? (uint32_t)n_list : 8 * F + 32;
    HIPCHK(w.grow(w.hot, hot_cap));
    a.nchunks = nchunks;
    if (screen) {
      const size_t nf = (size_t)F * nchunks;
      HIPCHK(w.grow(w.scr_flag, nf));
      HIPCHK(w.grow(w.scr_min, nf));
      HIPCHK(w.grow(w.scr_max, nf));
      add_fill(w.scr_flag.p, sizeof(uint32_t) * nf, 0u);
      add_fill(w.scr_min.p, sizeof(unsigned long long) * nf, 0xFFFFFFFFu);
      add_fill(w.scr_max.p, sizeof(unsigned long long) * nf, 0u);
      a.fmin = w.scr_min.p;
      a.fmax = w.scr_max.p;
    }
    a.hot = w.hot.p;
    a.hot_cap = hot_cap;
    launch_fill(fa, s);   // trigger words, queue heads and screen flags in one launch
    if ((rc = diag_sc_prof_arm(h, screen, s, &a.prof))) return rc;
    hipEvent_t e = h->timer.begin(s);
    if (screen) {
      ScreenArgs sa{};
      set_capture(sa, c);
      sa.N = h->N; sa.M = h->M;
      sa.thr_screen = h->thr - 0.01;
      sa.chunk_len = K; sa.chunk_lo = chunk_lo; sa.nchunks = nchunks;
      sa.flag = w.scr_flag.p; sa.fmin = w.scr_min.p; sa.fmax = w.scr_max.p;
      sa.count = a.hot_count; sa.hot = a.hot; sa.cap = a.hot_cap;
      // batches: every capture starts at its (first) framesync's origin; the streaming execute's
      // capture may begin mid-stream after a trim (its history is not empty)
      sa.empty_history = q.reset_trig ? 1u : 0u;
      if (a.diag & 32) a.diag |= 16;   // diagnostics: finalize as a separate kernel
      // Two phases for one frame per capture: the first chunks of every capture (a
      // frame's S0 plateau sits near its capture's start), then the rest only for captures with
      // no trigger yet. A trigger found in phase 1 is the capture's first (every earlier chunk
      // was evaluated) and phase 2 evaluates exactly the chunks one pass would have for the
      // others, so results are those of one pass; the screen's reads of antenna 0 past the
      // trigger of a synced capture are skipped. RMIMO_SC_PHASES=1: one pass.
      // Phase 1 ends one chunk past the S0 pair of a frame that starts its capture as the
      // reference's tx_worker lays frames out (main.cc:937-1153: SL (N nac + 1) + u zeros,
      // u < SL, then the two S0 symbols), the M-sample metric delay included.
      const uint64_t s0_end = (uint64_t)h->SL * ((uint64_t)h->N * h->nac + 4) + h->M;
      const uint64_t c1 = (!stream && chunk_lo == 0 && !diag_env().sc_one_phase && nchunks >= 16)
                              ? std::min<uint64_t>(nchunks, std::max<uint64_t>(2, (s0_end + K - 1) / K + 1))
                              : nchunks;
      sa.chunk_hi = c1;
      launch_sc_screen(sa, F, s);
      ScArgs a1 = a;
      if (c1 < nchunks) a1.snap = w.queue.p + 2;   // phase-1 items: done after this launch
      launch_sc_exact(a1, s);   // resolves and finalises its items itself
      if (a.diag & 32) launch_sc_finalize(a, s);
      if (c1 < nchunks) {
        sa.chunk_lo = c1;
        sa.chunk_hi = nchunks;
        sa.trig = w.trig.p;
        launch_sc_screen(sa, F, s);
        ScArgs a2 = a;
        a2.item_lo = w.queue.p + 2;
        launch_sc_exact(a2, s);
        if (a.diag & 32) launch_sc_finalize(a2, s);
      }
    } else {
      launch_sc(a, F, h->n_cu, s);
      launch_sc_hot(a, s);
    }
    if ((rc = diag_sc_count(h, F, nchunks, screen, hot_cap, s))) return rc;
    h->timer.end(0, e, s);
    if ((rc = diag_sc_prof_report(h, screen, s))) return rc;
  }
  PlateauArgs pa{};
  set_capture(pa, c);
  pa.trig = w.trig.p; pa.rec = w.rec.p; pa.rec_stride = w.rec_stride; pa.chunk_len = K;
  pa.N = h->N; pa.M = h->M; pa.SL = h->SL; pa.thr = h->thr; pa.win_len = h->win_len;
  pa.band = sc_band(h->M);
  pa.info = w.info.p;
  pa.fpc = fpc; pa.nchunks = nchunks;
  pa.cand = stream ? w.cand.p : nullptr;
  pa.certfail = stream ? w.certfail.p : nullptr;
  pa.ref_starts = q.ref_starts;
  pa.ref_stride = q.ref_stride ? q.ref_stride : fpc;
  hipEvent_t e = h->timer.begin(s);
  if (stream) launch_stream_walk(pa, F, s);
  else launch_plateau(pa, F, s);
  h->timer.end(1, e, s);
  HIPCHK(hipGetLastError());
  return MIMO_OK;
}

int run_estimate(mimo_rx *h, const Capture &c, uint32_t F, bool keys_zeroed, CfoBatchArgs *cfo,
                 float *corr_trace, hipStream_t s) {
  Workspace &w = h->ws;
  if (!keys_zeroed)
    HIPCHK(hipMemsetAsync(w.keys.p, 0, sizeof(unsigned long long) * F * h->N * h->n_slots, s));
  SearchArgs sa{};
  set_capture(sa, c);
  sa.N = h->N; sa.M = h->M; sa.SL = h->SL; sa.n_slots = h->n_slots;
  sa.lagc = h->lagc; sa.n_lagc = h->n_lagc;
  sa.codespec = h->codes.codespec.p; sa.vscale = h->vscale.p;
  sa.codespec_w = h->codes.codespec_w.p;
  sa.info = w.info.p; sa.keys = w.keys.p; sa.tw = h->tw;
  sa.corr_trace = corr_trace;
  LsArgs la{};
  set_capture(la, c);
  la.N = h->N; la.M = h->M; la.nac = h->nac; la.n_slots = h->n_slots;
  la.keys = w.keys.p; la.s1sign = h->s1sign.p; la.occ_index = h->occ.p;
  la.s1sign_w = h->s1sign_w.p;
  la.keep_bias = h->keep_bias; la.scale = h->ls_scale; la.info = w.info.p;
  la.n_groups = (h->nac + kLsCodesPerGroup - 1) / kLsCodesPerGroup;
  la.n_nvp = h->N * h->N * ((h->M + 255) / 256);
  la.G = w.G.p; la.nv_part = w.nvp.p; la.tw = h->tw;
  // opt-in CFO stage 2 after the search: the residual from the data prefixes
  auto cfo_stage2 = [&](int rot_window) {
    cfo->keys = w.keys.p; cfo->n_slots = h->n_slots; cfo->rot_window = rot_window;
    launch_cfo_batch(*cfo, F, 2, s);
  };
  if (h->search_ls) {
    // LS straight from the windows (ls_window_kernel) after a search that only finds the keys
    // (the CFO's stage 2 between them, its residual rotating each code's term in the LS
    // kernel) where that kernel has an instance, unless RMIMO_LS_FORM=terms: the search of slot
    // pairs with the LS terms fused in, then the fixed-order combine (ls_combine_q_kernel), the
    // parity tests' reference for the window form
    const bool ls_win = !diag_env().ls_terms && ls_window_supported(h->log2M, h->nac, cfo != nullptr);
    if (!ls_win) {
      HIPCHK(w.grow(w.lsq, (size_t)F * h->N * h->N * h->nac * h->M));
      sa.s1sign = h->s1sign.p; sa.lsq = w.lsq.p; sa.nac = h->nac;
      la.lsq = w.lsq.p;
    }
    sa.xcd_order = 1;
    sa.cfo_part = (cfo && cfo->fold) ? cfo->part : nullptr;   // folded CFO: derotating loads
    hipEvent_t e = h->timer.begin(s);
    launch_search_ls(sa, h->log2F, h->log2M, F, s);   // (window form: keys only, sa.lsq null)
    h->timer.end(2, e, s);
    if (cfo) {
      cfo_stage2(0);
      la.cfo_part = cfo->part;
      if (ls_win) la.cfo_fold = cfo->fold;
    }
    e = h->timer.begin(s);
    if (!ls_win) launch_ls_combine_q(la, F, s);
    else if (!launch_ls_window(la, h->log2M, F, s))   // (its own first check is ls_win's)
      return fail(MIMO_ERR_UNSUPPORTED, "ls_window_kernel: no instance for this geometry");
    h->timer.end(3, e, s);
  } else {
    hipEvent_t e = h->timer.begin(s);
    launch_search(sa, h->log2F, F, s);
    h->timer.end(2, e, s);
    if (cfo) cfo_stage2(1);   // before a separate LS pass: the whole window in place
    HIPCHK(w.grow(w.lspart, (size_t)F * h->N * h->N * la.n_groups * 3 * h->M));
    la.part = w.lspart.p;
    e = h->timer.begin(s);
    launch_ls(la, h->log2M, F, s);
    h->timer.end(3, e, s);
  }
  WeightArgs wa{};
  wa.N = h->N; wa.M = h->M; wa.M_occ = h->M_occ; wa.nac = h->nac; wa.SL = h->SL;
  wa.n_slots = h->n_slots; wa.detector = h->det; wa.noise_var = h->noise_var;
  wa.nv_norm = h->nv_norm; wa.occ_index = h->occ.p; wa.G = w.G.p; wa.W = w.W.p;
  wa.gain = w.gain.p; wa.nv_part = w.nvp.p; wa.n_nvp = la.n_nvp; wa.keys = w.keys.p;
  wa.win_len = h->win_len;
  wa.info = w.info.p;
  hipEvent_t e = h->timer.begin(s);
  launch_weights(wa, F, s);
  h->timer.end(4, e, s);
  HIPCHK(hipGetLastError());
  return MIMO_OK;
}

int run_decode(mimo_rx *h, const Capture &c, uint32_t F, const DecodeRequest &q, hipStream_t s) {
  Workspace &w = h->ws;
  const uint32_t max_out = q.max_out;
  int rc = ensure_workspace(h, F, 0);
  if (rc || max_out == 0) return rc;
  DecodeArgs d{};
  set_capture(d, c);
  d.N = h->N; d.M = h->M; d.cp = h->cp; d.SL = h->SL; d.M_occ = h->M_occ;
  d.detector = h->det; d.siso_tx = h->siso_tx; d.siso_rx = h->siso_rx; d.dn = h->dn;
  d.occ_index = h->occ.p; d.W = w.W.p; d.gain = w.gain.p; d.G = w.G.p; d.info = w.info.p;
  d.max_out = max_out; d.out_sym = q.out_sym; d.out_idx = q.out_idx;
  if (q.layout == MIMO_LAYOUT_SYMBOL_MAJOR) {   // [F][max_out][N][M_occ]
    d.o_ts = h->M_occ;
    d.o_ss = (uint64_t)h->N * h->M_occ;
  } else {                                     // [F][N][max_out][M_occ]
    d.o_ts = (uint64_t)max_out * h->M_occ;
    d.o_ss = h->M_occ;
  }
  d.ref_mode = q.ref_mode; d.ref_idx = q.ref_idx; d.ref_seed = q.ref_seed;
  d.frame_id0 = q.frame_id0;
  d.qam = h->qam; d.tw = h->tw;
  d.n_frames = F; d.n_cu = h->n_cu;
  d.n_caps = q.n_caps ? q.n_caps : F; d.n_refs = F;
  d.all_occ = (h->M_occ == h->M) ? 1 : 0;
  if ((rc = diag_dec_prof_arm(h, s, &d.prof))) return rc;
  hipEvent_t e = h->timer.begin(s);
  d.nrec = w.nrec.p;
  d.cpe = h->cfo ? (q.cfo_fold_part ? 2 : 1) : 0;
  d.cfo_part = q.cfo_fold_part;
  d.rec_stride = max_out;
  if (decode_split_accepts(d, h->log2M)) {
    // [F][group][N][M] complex64 spectra of the 8x8 split decode (one symbol group)
    if (w.grow(w.spec, (size_t)F * split_group_symbols(max_out) * h->N * h->M) != hipSuccess)
      return fail(MIMO_ERR_NOMEM, "split decode scratch");
    d.spec = w.spec.p;
    d.rec_stride = std::max(d.rec_stride, split_plan(max_out, h->log2M, nullptr, nullptr));
  }
  HIPCHK(w.grow(w.evm_part, (size_t)F * d.rec_stride * h->N * 3 * kMaxEvmParts));
  d.evm_part = w.evm_part.p;
  bool per_frame = false;
  int path = MIMO_DECODE_NONE;
  const uint32_t parts = launch_decode(d, h->log2M, F, s, &per_frame, &path);
  h->timer.end(5, e, s);
  h->last_decode_path = path;
  h->last_cfo_mode = !h->cfo ? 0 : (path == MIMO_DECODE_STREAM && decode_stream_cpe(d) ? 2 : 1);
  if ((rc = diag_cfo_frames(h, F, s))) return rc;
  if (!parts)   // run_batch widens every sc16 batch the streaming decode does not take
    return fail(MIMO_ERR_UNSUPPORTED, "no decode kernel takes this configuration");
  if ((rc = diag_dec_prof_report(h, s))) return rc;
  EvmArgs ea{};
  ea.N = h->N; ea.max_out = max_out; ea.parts = parts; ea.info = w.info.p;
  ea.evm_part = w.evm_part.p;
  ea.rec_stride = d.rec_stride;
  ea.evm_out = w.evm_out.p;
  ea.chunk_part = w.evm_chunk.p;
  ea.counter = w.evm_cnt.p;
  ea.nrec = per_frame ? w.nrec.p : nullptr;
  // per workgroup segment (streaming, residue-class), not per chunk x range
  ea.few = (path == MIMO_DECODE_STREAM) ? 1 : 0;
  e = h->timer.begin(s);
  launch_evm(ea, F, s);
  h->timer.end(6, e, s);
  HIPCHK(hipGetLastError());
  return MIMO_OK;
}

}  // namespace mimo
