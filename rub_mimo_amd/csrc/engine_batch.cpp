// rub_mimo_amd/csrc/engine_batch.cpp -- mimo_rx_process_batch: n_frames device-resident
// captures, every stage launched once for the whole batch on one stream, no host
// synchronisation (the bench's step); its HIP-graph cache, the batch getters and the soft
// output passes over the last batch.
#include "engine_internal.hpp"

static void drop_graph(mimo_rx *h, mimo_rx::GraphEntry &g) {
  if (g.exec) {   // a replay may still be in flight on its stream
    (void)hipStreamSynchronize(g.stream ? g.stream : h->stream);
    (void)hipGraphExecDestroy(g.exec);
  }
  g = mimo_rx::GraphEntry{};
}

void mimo::invalidate_graph(mimo_rx *h) {
  for (auto &g : h->graphs) drop_graph(h, g);
}

// ---------------- batched device frames ----------------
static uint32_t batch_fpc(const mimo_batch *b) {
  return b->frames_per_capture > 1 ? b->frames_per_capture : 1u;
}

// what decode_stream_accepts / decode_split_accepts look at, to ask ahead of the launch whether
// the streaming or the split decode would take this batch
static DecodeArgs decode_probe(const mimo_rx *h, const mimo_batch *b, int sc16) {
  DecodeArgs probe{};
  probe.N = h->N; probe.detector = h->det;
  probe.all_occ = (h->M_occ == h->M) ? 1 : 0;
  probe.n_caps = b->n_frames; probe.n_refs = b->n_frames * batch_fpc(b); probe.qam = h->qam;
  probe.ref_mode = b->ref_mode; probe.ref_idx = reinterpret_cast<const uint8_t *>(b->d_ref_idx);
  probe.stride = b->stride; probe.max_out = b->max_out_syms; probe.M_occ = h->M_occ;
  probe.out_sym = reinterpret_cast<float2 *>(b->d_out_sym);
  probe.out_idx = reinterpret_cast<uint8_t *>(b->d_out_idx);
  probe.sc16 = sc16;
  return probe;
}

// The opt-in CFO folds into the loads (no scratch passes) where the fused search + LS (wave
// form) and the streaming decode's CPE variant run: fc32 input (read in place or widened),
// reference indices from HBM, both or neither output. Elsewhere the scratch passes remain.
static bool cfo_folds(const mimo_rx *h, const mimo_batch *b, bool widened) {
  if (!h->cfo || !h->search_ls) return false;
  if (b->sample_format == MIMO_SAMPLE_SC16 && !widened) return false;
  if (b->ref_mode != 1 || (!b->d_out_sym) != (!b->d_out_idx)) return false;
  return decode_stream_accepts(decode_probe(h, b, 0), h->log2M, b->n_frames * batch_fpc(b));
}

// opt-in CFO stage 1 over capture c: the coarse estimate per synced frame at its trigger into
// h->ws.cfo_eps (allocated by the caller), nothing derotated (out null, fold 0) until the caller
// says where
static CfoBatchArgs cfo_stage1(const mimo_rx *h, const Capture &c) {
  CfoBatchArgs ca{};
  ca.iq = c.iq; ca.out = nullptr; ca.stride = c.stride; ca.frame_len = c.frame_len;
  ca.len = h->win_len + 64; ca.win = h->win_len; ca.N = h->N; ca.M = h->M; ca.cp = h->cp; ca.SL = h->SL;
  ca.n_codes = h->N * h->nac; ca.n_data = h->pid + 2; ca.info = h->ws.info.p;
  ca.part = h->ws.cfo_eps.p;
  return ca;
}

static DecodeRequest decode_request(const mimo_batch *b, const double *cfo_fold_part) {
  DecodeRequest q{};
  q.max_out = b->max_out_syms; q.layout = b->out_layout;
  q.out_sym = reinterpret_cast<float2 *>(b->d_out_sym);
  q.out_idx = reinterpret_cast<uint8_t *>(b->d_out_idx);
  q.ref_mode = b->ref_mode; q.ref_seed = b->ref_seed; q.frame_id0 = b->frame_id0;
  q.ref_idx = reinterpret_cast<const uint8_t *>(b->d_ref_idx);
  q.n_caps = b->n_frames; q.cfo_fold_part = cfo_fold_part;
  return q;
}

// One batch, launched on s. Everything a stage reads of this batch travels in c and the
// request aggregates, nothing in the handle, so an early return leaves no state behind.
static int run_batch(mimo_rx *h, const mimo_batch *b, hipStream_t s) {
  Workspace &w = h->ws;
  const uint32_t fpc = batch_fpc(b), slots = b->n_frames * fpc;
  const bool front = b->stages != MIMO_STAGES_DECODE, decode = b->stages != MIMO_STAGES_FRONT;
  Capture c{reinterpret_cast<const float2 *>(b->d_iq), b->stride, b->frame_len, 0, 1.0f};
  bool widened = false;
  if (b->sample_format == MIMO_SAMPLE_SC16) {
    // sc16 wire input: read in place by S&C, the fused search + LS and the streaming decode
    // where the configuration takes them; otherwise widened once into an internal fc32 batch
    const DecodeArgs probe = decode_probe(h, b, 1);
    const bool fused = sc_screen_ok(h->M) && h->search_ls && !h->cfo &&
                       (decode_stream_accepts(probe, h->log2M, slots) ||
                        decode_split_accepts(probe, h->log2M));
    if (fused) {
      c.sc16 = 1;
      c.scale = b->sc16_scale;
    } else {
      if (front) {   // (a DECODE call reads what this batch's front half widened)
        const size_t need = (size_t)b->n_frames * h->N * b->stride;
        if (w.grow(w.wide, need) != hipSuccess) return fail(MIMO_ERR_NOMEM, "sc16 widening buffer");
        hipEvent_t e = h->timer.begin(s);
        const bool ok = launch_sc16_to_fc32(b->d_iq, b->stride, w.wide.p, b->stride,
                                            b->n_frames * h->N, b->frame_len, b->sc16_scale, s);
        h->timer.end(0, e, s);     // timed with the S&C stage (one extra launch)
        if (!ok) return fail(MIMO_ERR_ARG, "sc16 widening: bad geometry");
      }
      c.iq = w.wide.p;
      widened = true;
    }
  } else if (b->sample_format != MIMO_SAMPLE_FC32) {
    return fail(MIMO_ERR_ARG, "mimo_batch.sample_format must be MIMO_SAMPLE_FC32 or _SC16");
  }
  // The decode half of a batch whose front half this handle ran last. (Nothing checks that
  // yet: a token handed from the FRONT call to its DECODE call would be verified here, and
  // ws.gen is what it would compare.)
  if (!front) return run_decode(h, c, slots, decode_request(b, nullptr), s);
  SyncRequest sq{};
  sq.reset_trig = true;
  sq.zero_keys = true;
  sq.fpc = fpc;
  sq.ref_starts = fpc > 1 ? b->d_ref_starts : nullptr;
  sq.ref_stride = b->ref_stride;
  int rc = run_sync(h, c, b->n_frames, sq, s);
  if (rc) return rc;
  CfoBatchArgs ca{};
  const bool fold = cfo_folds(h, b, widened);
  if (fold) {
    // opt-in CFO, folded: estimates only (stage 1 here, stage 2 after the search); the
    // search + LS loads and the decode derotate by them, no scratch capture
    if (w.grow(w.cfo_eps, cfo_batch_part_doubles(slots)) != hipSuccess)
      return fail(MIMO_ERR_NOMEM, "cfo estimate allocation failed");
    ca = cfo_stage1(h, c);
    ca.fold = 1;
    launch_cfo_batch(ca, slots, 1, s);
  } else if (h->cfo) {
    // opt-in CFO, stage 1: the window derotated into a scratch capture that search, LS,
    // weights and decode read (S&C ran on the raw samples: |P| and R do not depend on a
    // frequency offset)
    const size_t need = (size_t)b->n_frames * h->N * b->stride;
    if (w.grow(w.cfo_iq, need) != hipSuccess ||
        w.grow(w.cfo_eps, cfo_batch_part_doubles(slots)) != hipSuccess)
      return fail(MIMO_ERR_NOMEM, "cfo scratch allocation failed");
    ca = cfo_stage1(h, c);
    ca.out = w.cfo_iq.p;
    launch_cfo_batch(ca, slots, 1, s);
    c.iq = w.cfo_iq.p;
  }
  rc = run_estimate(h, c, slots, true, h->cfo ? &ca : nullptr, nullptr, s);
  if (rc) return rc;
  if (h->cfo && !fold && h->search_ls)   // stage 2's data-region derotation
    launch_cfo_batch_rot2(ca, slots, s);
  return decode ? run_decode(h, c, slots, decode_request(b, fold ? ca.part : nullptr), s) : MIMO_OK;
}

// The whole batch (every launch and memset run_batch issues) is captured into a HIP graph once a
// call repeats the previous call's arguments, and replayed from then on: the grid shapes depend
// only on the configuration and F (S&C items and hot items are pulled from device-side queues),
// so the graph stays valid while the workspace it points into has not moved: an entry carries
// the ws.gen it was made at. Not used while stage timing or a diagnostic counter is on.
static bool same_batch(const mimo_batch &x, const mimo_batch &y) {
  return x.d_iq == y.d_iq && x.stride == y.stride && x.frame_len == y.frame_len &&
         x.n_frames == y.n_frames && x.max_out_syms == y.max_out_syms &&
         x.d_out_sym == y.d_out_sym && x.d_out_idx == y.d_out_idx && x.ref_mode == y.ref_mode &&
         x.d_ref_idx == y.d_ref_idx && x.ref_seed == y.ref_seed && x.frame_id0 == y.frame_id0 &&
         batch_fpc(&x) == batch_fpc(&y) && x.d_ref_starts == y.d_ref_starts &&
         x.ref_stride == y.ref_stride && x.sample_format == y.sample_format &&
         x.sc16_scale == y.sc16_scale && x.out_layout == y.out_layout && x.stages == y.stages;
}

extern "C" {

int mimo_rx_process_batch(mimo_rx *h, const mimo_batch *b, void *hip_stream) {
  if (!h || !b || !b->d_iq) return fail(MIMO_ERR_ARG, "null argument");
  if (b->n_frames == 0) return MIMO_OK;
  if (b->stride < b->frame_len) return fail(MIMO_ERR_ARG, "stride < frame_len");
  if (b->ref_mode == 1 && !b->d_ref_idx) return fail(MIMO_ERR_ARG, "ref_mode 1 needs d_ref_idx");
  if (b->out_layout != MIMO_LAYOUT_STREAM_MAJOR && b->out_layout != MIMO_LAYOUT_SYMBOL_MAJOR)
    return fail(MIMO_ERR_ARG, "mimo_batch.out_layout must be MIMO_LAYOUT_STREAM_MAJOR or _SYMBOL_MAJOR");
  if (batch_fpc(b) > 64)
    return fail(MIMO_ERR_ARG, "frames_per_capture must be at most 64");
  if (b->stages > MIMO_STAGES_DECODE) return fail(MIMO_ERR_ARG, "mimo_batch.stages must be 0, 1 or 2");
  if (b->stages != MIMO_STAGES_ALL && h->cfo)
    return fail(MIMO_ERR_UNSUPPORTED, "split stages with cfo_correct");
  // the unfolded CFO stages derotate each frame's window into one scratch capture per
  // capture: back-to-back frames' windows overlap there, so that combination is refused (the
  // folded form has no scratch)
  if (h->cfo && batch_fpc(b) > 1 && !cfo_folds(h, b, b->sample_format == MIMO_SAMPLE_SC16))
    return fail(MIMO_ERR_UNSUPPORTED, "cfo_correct with frames_per_capture > 1 needs the folded "
                                      "CFO path (fc32 C2/C3-type geometry, ref_mode 1)");
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
  // the cache entry of this batch: same arguments, stream and workspace generation
  mimo_rx::GraphEntry *hit = nullptr;
  for (auto &g : h->graphs)
    if (g.used && same_batch(g.key, *b) && g.stream == s && g.gen == h->ws.gen) hit = &g;
  int rc = MIMO_OK;
  if (diag_env().no_graph || h->timer.on) {
    rc = run_batch(h, b, s);
  } else if (hit && hit->exec) {
    hit->used = ++h->graph_tick;
    HIPCHK(hipGraphLaunch(hit->exec, s));
  } else if (hit) {
    // second identical call: workspace and one-time kernel attributes are settled; capture
    hit->used = ++h->graph_tick;
    hipGraph_t g = nullptr;
    hipGraphExec_t ex = nullptr;
    HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
    rc = run_batch(h, b, s);
    // kept only if the capture succeeded and the workspace did not move under it
    bool ok = hipStreamEndCapture(s, &g) == hipSuccess && g && !rc && hit->gen == h->ws.gen;
    ok = ok && hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) == hipSuccess;
    if (g) (void)hipGraphDestroy(g);
    if (ok) {
      hit->exec = ex;
      HIPCHK(hipGraphLaunch(hit->exec, s));
    } else {
      (void)hipGetLastError();
      *hit = mimo_rx::GraphEntry{};
      if (!rc) rc = run_batch(h, b, s);   // not captured: run directly
    }
  } else {
    rc = run_batch(h, b, s);
    // a workspace reallocation makes every earlier capture stale
    for (auto &g : h->graphs)
      if (g.used && g.gen != h->ws.gen) drop_graph(h, g);
    if (rc == MIMO_OK) {
      mimo_rx::GraphEntry *slot = &h->graphs[0];   // an empty or the least recently used slot
      for (auto &g : h->graphs)
        if (g.used < slot->used) slot = &g;
      drop_graph(h, *slot);
      slot->key = *b;
      slot->stream = s;
      slot->gen = h->ws.gen;
      slot->used = ++h->graph_tick;
    }
  }
  if (rc) return rc;
  h->last_frames = b->n_frames * batch_fpc(b);
  h->last_max_out = b->max_out_syms;
  h->last_layout = b->out_layout;
  return MIMO_OK;
}

int mimo_rx_batch_results(mimo_rx *h, mimo_frame_result *out, uint32_t F) {
  if (!h || !out) return fail(MIMO_ERR_ARG, "null argument");
  if (F > h->last_frames) return fail(MIMO_ERR_ARG, "more frames than the last batch");
  std::vector<FrameInfo> inf(F);
  std::vector<double> ev((size_t)F * h->N * 3);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(inf.data(), h->ws.info.p, sizeof(FrameInfo) * F, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ev.data(), h->ws.evm_out.p, sizeof(double) * ev.size(), hipMemcpyDeviceToHost));
  for (uint32_t f = 0; f < F; f++) {
    mimo_frame_result &r = out[f];
    std::memset(&r, 0, sizeof(r));
    const FrameInfo &I = inf[f];
    const bool synced = I.status == MIMO_FRAME_OK || I.status == MIMO_FRAME_INCOMPLETE;
    const uint64_t o = I.origin;   // positions as the framesync started at origin reports them
    r.status = I.status;
    r.n_sym = (I.status == 0) ? I.n_sym : 0;
    r.trigger = synced ? I.trigger - o : I.trigger;
    r.sync_index = synced ? I.sync_index - o : 0;
    r.num_samples_processed = I.nsp;
    r.noise_var = I.noise_var;
    r.cfo_eps = h->cfo ? I.cfo_eps : 0.0f;
    r.origin = o;
    r.capture = I.cap;
    r.ref_frame = I.ref;
    for (uint32_t s = 0; s < h->N; s++) {
      r.plateau_start[s] = synced ? I.plateau_start[s] - o : 0;
      r.plateau_end[s] = synced ? I.plateau_end[s] - o : 0;
      if (inf[f].status == 0) {
        r.evm_num[s] = ev[((size_t)f * h->N + s) * 3 + 0];
        r.evm_den[s] = ev[((size_t)f * h->N + s) * 3 + 1];
        r.errors[s] = (uint64_t)ev[((size_t)f * h->N + s) * 3 + 2];
      }
    }
  }
  return MIMO_OK;
}

int mimo_rx_batch_corr(mimo_rx *h, uint32_t *corr, uint32_t *s0, uint32_t F) {
  if (!h) return fail(MIMO_ERR_ARG, "null handle");
  if (F > h->last_frames) return fail(MIMO_ERR_ARG, "more frames than the last batch");
  HIPCHK(hipDeviceSynchronize());
  return copy_corr(h, F, corr, s0);
}

int mimo_rx_batch_G(mimo_rx *h, float *G, uint32_t F) {
  if (!h || !G) return fail(MIMO_ERR_ARG, "null argument");
  if (F > h->last_frames) return fail(MIMO_ERR_ARG, "more frames than the last batch");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(G, h->ws.G.p, sizeof(float2) * (size_t)F * h->M * h->N * h->N,
                   hipMemcpyDeviceToHost));
  return MIMO_OK;
}

int mimo_rx_batch_W(mimo_rx *h, float *W, uint32_t F) {
  if (!h || !W) return fail(MIMO_ERR_ARG, "null argument");
  if (F > h->last_frames) return fail(MIMO_ERR_ARG, "more frames than the last batch");
  HIPCHK(hipDeviceSynchronize());
  for (uint32_t f = 0; f < F; f++) {
    int rc = copy_W(h, f, W + (size_t)f * h->M * h->N * h->N * 2);
    if (rc) return rc;
  }
  return MIMO_OK;
}

int mimo_rx_batch_gain(mimo_rx *h, float *gain, uint32_t F) {
  if (!h || !gain) return fail(MIMO_ERR_ARG, "null argument");
  if (F > h->last_frames) return fail(MIMO_ERR_ARG, "more frames than the last batch");
  if (F == 0) return MIMO_OK;
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipDeviceSynchronize());
  std::vector<float> tmp((size_t)F * h->M);
  HIPCHK(hipMemcpy(tmp.data(), h->ws.gain.p, sizeof(float) * tmp.size(), hipMemcpyDeviceToHost));
  for (uint32_t f = 0; f < F; f++)
    for (uint32_t k = 0; k < h->M; k++)
      if (h->occ_index[k] >= 0)
        gain[(size_t)f * h->M_occ + h->occ_index[k]] = tmp[(size_t)f * h->M + k];
  return MIMO_OK;
}

// ---------------- soft output: post-detection MSE and max-log LLRs (soft_kernels.hip) -------
// the MSE of the last batch's F frame slots into h->nu, on stream s
static int launch_batch_mse(mimo_rx *h, uint32_t F, hipStream_t s) {
  if (h->nu.ensure((size_t)F * h->N * h->M_occ) != hipSuccess)
    return fail(MIMO_ERR_NOMEM, "post-detection MSE buffer");
  MseArgs m{};
  m.N = h->N; m.M = h->M; m.M_occ = h->M_occ;
  m.occ_index = h->occ.p; m.G = h->ws.G.p; m.W = h->ws.W.p; m.gain = h->ws.gain.p;
  m.info = h->ws.info.p;
  m.nu = h->nu.p;
  if (!launch_mse(m, F, s)) return fail(MIMO_ERR_UNSUPPORTED, "no MSE kernel for this stream count");
  HIPCHK(hipGetLastError());
  return MIMO_OK;
}

int mimo_rx_soft_demap(mimo_rx *h, const mimo_soft_demap *a, void *hip_stream) {
  if (!h || !a || !a->d_sym || !a->d_llr) return fail(MIMO_ERR_ARG, "null argument");
  if (((uintptr_t)a->d_sym & 15u) || ((uintptr_t)a->d_llr & 15u))
    return fail(MIMO_ERR_ARG, "d_sym and d_llr must be 16-byte aligned");
  if (!std::isfinite(a->llr_scale) || !(a->llr_scale > 0.0f))
    return fail(MIMO_ERR_ARG, "llr_scale must be finite and positive");
  if (a->format != MIMO_LLR_I8 && a->format != MIMO_LLR_F32)
    return fail(MIMO_ERR_ARG, "mimo_soft_demap.format must be MIMO_LLR_I8 or _F32");
  if (a->out_layout != MIMO_LAYOUT_STREAM_MAJOR && a->out_layout != MIMO_LAYOUT_SYMBOL_MAJOR)
    return fail(MIMO_ERR_ARG, "mimo_soft_demap.out_layout must be MIMO_LAYOUT_STREAM_MAJOR or _SYMBOL_MAJOR");
  if (h->last_frames == 0) return fail(MIMO_ERR_STATE, "no batch has run on this handle");
  if (h->det == MIMO_DET_SISO)
    return fail(MIMO_ERR_UNSUPPORTED, "soft output with the SISO detector");
  if (a->n_frames != h->last_frames || a->max_out_syms != h->last_max_out)
    return fail(MIMO_ERR_ARG, "n_frames and max_out_syms must be the last batch's");
  const uint64_t rows = (uint64_t)a->n_frames * h->N * a->max_out_syms;
  if (rows >= 0xFFFFFFFFull) return fail(MIMO_ERR_ARG, "too many symbol rows");
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
  int rc = launch_batch_mse(h, a->n_frames, s);
  if (rc) return rc;
  SoftArgs k{};
  k.sym = reinterpret_cast<const float2 *>(a->d_sym);
  k.llr = a->d_llr;
  k.total = rows * h->M_occ;
  k.rows = (uint32_t)rows;
  k.N = h->N; k.M_occ = h->M_occ; k.max_out = a->max_out_syms;
  k.symbol_major = a->out_layout == MIMO_LAYOUT_SYMBOL_MAJOR;
  k.f32 = a->format == MIMO_LLR_F32;
  k.bits = h->qam.b;
  k.qam_scale = h->qam.scale;
  k.llr_scale = a->llr_scale;
  k.info = h->ws.info.p;
  k.nu = h->nu.p;
  if (!launch_soft_demap(k, s)) return fail(MIMO_ERR_UNSUPPORTED, "no soft demapper for this QAM order");
  HIPCHK(hipGetLastError());
  return MIMO_OK;
}

int mimo_rx_batch_mse(mimo_rx *h, float *mse, uint32_t F) {
  if (!h || !mse) return fail(MIMO_ERR_ARG, "null argument");
  if (h->last_frames == 0) return fail(MIMO_ERR_STATE, "no batch has run on this handle");
  if (h->det == MIMO_DET_SISO)
    return fail(MIMO_ERR_UNSUPPORTED, "post-detection MSE with the SISO detector");
  if (F > h->last_frames) return fail(MIMO_ERR_ARG, "more frames than the last batch");
  if (F == 0) return MIMO_OK;
  HIPCHK(hipDeviceSynchronize());
  int rc = launch_batch_mse(h, h->last_frames, h->stream);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(mse, h->nu.p, sizeof(float) * (size_t)F * h->N * h->M_occ,
                   hipMemcpyDeviceToHost));
  return MIMO_OK;
}

int mimo_rx_get_stage_times(mimo_rx *h, double *ms, uint32_t *launches) {
  if (!h) return fail(MIMO_ERR_ARG, "null handle");
  for (int i = 0; i < MIMO_NUM_STAGES; i++) {
    if (ms) ms[i] = 0.0;
    if (launches) launches[i] = 0;
  }
  for (auto &e : h->timer.ev) {
    HIPCHK(hipEventSynchronize(e.second.second));
    float t = 0.0f;
    HIPCHK(hipEventElapsedTime(&t, e.second.first, e.second.second));
    if (ms) ms[e.first] += t;
    if (launches) launches[e.first] += 1;
    (void)hipEventDestroy(e.second.first);
    (void)hipEventDestroy(e.second.second);
  }
  h->timer.ev.clear();
  return MIMO_OK;
}

}  // extern "C"
