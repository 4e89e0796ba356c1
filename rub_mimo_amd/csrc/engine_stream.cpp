// rub_mimo_amd/csrc/engine_stream.cpp -- mimo_rx_execute: the reference's streaming
// framesync::execute (framing.cc:471-506) over host chunks of any size. Samples are appended
// to a device capture buffer, the S&C kernels run over the new chunks only, and the channel
// estimate + replay decode run once the window [sync_index - SL, sync_index - SL + ACB + TX)
// is complete; decoded symbols are handed to the callback one OFDM symbol at a time
// (framing.cc:587). Also the DEBUG_LOG writers.
#include "engine_internal.hpp"

extern "C" {

static int grow_capture(mimo_rx *h, uint64_t need) {
  if (need <= h->cap_len && h->capbuf.p) return MIMO_OK;
  // 1.5x growth in 16 K steps (the streaming capture is trimmed while seeking, so its size
  // follows what is held plus one piece, not the stream length)
  uint64_t nc = std::max<uint64_t>(need, h->cap_len + h->cap_len / 2);
  nc = std::max<uint64_t>((nc + 16383) / 16384 * 16384, 1 << 16);
  float2 *np = nullptr;
  HIPCHK(hipMalloc(&np, sizeof(float2) * nc * h->N));
  if (h->capbuf.p && h->total) {
    HIPCHK(hipMemcpy2DAsync(np, sizeof(float2) * nc, h->capbuf.p, sizeof(float2) * h->cap_len,
                            sizeof(float2) * h->total, h->N, hipMemcpyDeviceToDevice, h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  h->capbuf.adopt(np, nc * h->N);
  h->cap_len = nc;
  return MIMO_OK;
}

// DEBUG_LOG: the search metric of every lag as the reference's corr_<rx>_<ac>.dat files, one
// float per window index over [0, ACB - M): S0's lags at [0, SL) (corr_<rx>_0), access code
// ac's at SL (ac + 1) + [0, SL) (framing.cc:716-737), zeros elsewhere
static int write_corr_logs(mimo_rx *h) {
  const size_t per = (size_t)h->n_slots * h->SL;
  std::vector<float> tr((size_t)h->N * per);
  HIPCHK(hipMemcpy(tr.data(), h->dbg_corr.p, sizeof(float) * tr.size(), hipMemcpyDeviceToHost));
  const size_t len = h->acb - h->M;
  std::vector<float> out(len);
  for (uint32_t ch = 0; ch < h->N; ch++)
    for (uint32_t slot = 0; slot < h->n_slots; slot++) {
      std::fill(out.begin(), out.end(), 0.0f);
      const size_t at = (size_t)h->SL * slot;
      for (uint32_t i = 0; i < h->SL && at + i < len; i++) out[at + i] = tr[ch * per + (size_t)slot * h->SL + i];
      const std::string fn = h->dbg_dir + "/corr_" + std::to_string(ch + 1) + "_" +
                             std::to_string(slot) + ".dat";
      FILE *fp = fopen(fn.c_str(), "wb");
      if (!fp) return fail(MIMO_ERR_ARG, "cannot open " + fn);
      const size_t w = fwrite(out.data(), sizeof(float), len, fp);
      fclose(fp);
      if (w != len) return fail(MIMO_ERR_ARG, "short write " + fn);
    }
  return MIMO_OK;
}

static int finish_estimate(mimo_rx *h) {
  // channel estimate + replay decode of the complete window; callbacks per OFDM symbol
  const Capture c{h->capbuf.p, h->cap_len, h->total, 0, 1.0f};   // fc32, whatever batches ran
  // the window is complete: the device frame record says so (the plateau kernel saw it
  // incomplete when the trigger fired)
  h->sinfo.status = MIMO_FRAME_OK;
  HIPCHK(hipMemcpyAsync(h->ws.info.p, &h->sinfo, sizeof(FrameInfo), hipMemcpyHostToDevice,
                        h->stream));
  float *corr_trace = nullptr;
  if (!h->dbg_dir.empty()) {
    HIPCHK(h->dbg_corr.ensure((size_t)h->N * h->n_slots * h->SL));
    HIPCHK(hipMemsetAsync(h->dbg_corr.p, 0, sizeof(float) * h->N * h->n_slots * h->SL, h->stream));
    corr_trace = h->dbg_corr.p;
  }
  int rc = run_estimate(h, c, 1, false, nullptr, corr_trace, h->stream);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(&h->sinfo, h->ws.info.p, sizeof(FrameInfo), hipMemcpyDeviceToHost,
                        h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (!h->dbg_dir.empty() && (rc = write_corr_logs(h))) return rc;
  const uint32_t n_sym = h->sinfo.n_sym;
  const size_t per = (size_t)h->N * h->M_occ;
  if (n_sym) {
    HIPCHK(h->symbuf.ensure(per * n_sym));
    DecodeRequest q{};
    q.max_out = n_sym;
    q.out_sym = h->symbuf.p;
    q.layout = MIMO_LAYOUT_STREAM_MAJOR;             // symbuf is [N][n_sym][M_occ]
    if ((rc = run_decode(h, c, 1, q, h->stream))) return rc;
    h->symhost.resize(per * n_sym);
    HIPCHK(hipMemcpyAsync(h->symhost.data(), h->symbuf.p, sizeof(float2) * per * n_sym,
                          hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  } else {
    h->symhost.clear();
  }
  h->have_est = true;
  h->last_frames = 1;
  h->last_max_out = n_sym;
  if (h->cb) {
    std::vector<const float *> ptr(h->N);
    for (uint32_t s = 0; s < n_sym; s++) {
      for (uint32_t t = 0; t < h->N; t++)
        ptr[t] = reinterpret_cast<const float *>(h->symhost.data() +
                                                 ((size_t)t * n_sym + s) * h->M_occ);
      h->cb(ptr.data(), h->N, h->M_occ, h->user);
    }
  }
  return MIMO_OK;
}

// Bounded streaming memory. The reference holds a window ring of ACB + TX samples
// (framing.cc:387-388, 639-651) and constant-size S&C filter state, so an unsynchronised stream
// costs it nothing. Here the device capture keeps, while seeking, only what a later trigger can
// still reach: the S&C history of the next chunk's work item (its halo and M samples of
// filter history) and, in front of it, room for a plateau run and the window's leading SL.
// Samples before a drop point D (a multiple of the chunk length, so the chunk grid stays
// aligned) are dropped only when every antenna has a proven metric zero (y <= threshold in
// the oracle's fp32, certified in fp64 with the decision band) in [D + SL + M, next item): no
// plateau run then reaches back past it, so every run start, sync index and window start of
// a later trigger lie inside the kept samples. A run that never ends (pathological input)
// postpones the drop and the capture grows, as before.
__global__ void trim_probe_kernel(const float2 *x, uint64_t stride, uint32_t M, int64_t lo,
                                  int64_t hi, double thr, double band, uint32_t *ok) {
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  const float2 *r = x + (uint64_t)s * stride;
  const int64_t span = hi - lo;
  bool zero = false;
  if (span > 0) {
    const int64_t q = hi - 1 - (span * (int64_t)lane) / 64;   // 64 positions spread over [lo, hi)
    double pr = 0.0, pi = 0.0, z = 0.0;
    const int64_t h = M / 2;
    for (int64_t k = q - (int64_t)M + 1; k <= q; k++) {
      const float2 v = r[k];
      z += (double)v.x * v.x + (double)v.y * v.y;
      if (k > q - h) {
        const float2 d = r[k - h];
        pr += (double)d.x * v.x + (double)d.y * v.y;
        pi += (double)d.x * v.y - (double)d.y * v.x;
      }
    }
    const double R = 0.5 * z;
    // the fp64 metric clears the threshold by more than the fp32 error band: the oracle's y
    // is not above the threshold either
    // an all-zero window (R = 0, so P = 0: an idle radio or zero padding) is the oracle's 0/0,
    // which compares false: not above the threshold either
    zero = R == 0.0 || pr * pr + pi * pi < (thr - band) * R * R;
  }
  const unsigned long long b = __ballot(zero);
  if (lane == 0) ok[s] = b ? 1u : 0u;
}

static int maybe_trim(mimo_rx *h) {
  const uint64_t K = sc_chunk_len(h->cp);
  const uint64_t H = kScSpan - K;                     // halo of an S&C item
  const uint64_t c_lo = h->total / K;                 // the next S&C starts at this chunk
  const uint64_t need = H + 2 * (uint64_t)h->SL + 2 * (uint64_t)h->M + K;
  if (c_lo * K < need + K) return MIMO_OK;            // nothing to drop yet
  const uint64_t D = (c_lo * K - need) / K * K;
  // high-water mark: only once the droppable prefix reaches half a window (pieces are half a
  // window too), so a probe and its host round trip come once per half window of stream, not
  // once per S&C chunk, and the capture stays within about a window plus the S&C reach
  if (D < std::max<uint64_t>(K, h->win_len / 2)) return MIMO_OK;
  const int64_t lo = (int64_t)(D + h->SL + h->M), hi = (int64_t)(c_lo * K - H);
  if (hi - lo < (int64_t)K / 2) return MIMO_OK;
  // the probe's span moves only when the S&C reaches a new chunk: a caller feeding small pieces
  // pays one probe (and its host round trip) per chunk of stream, not one per call. (The stream
  // position of that chunk, not its capture-relative index: a trim re-bases the capture.)
  const uint64_t c_abs = h->origin + c_lo * K;
  if (c_abs == h->trim_clo) return MIMO_OK;
  h->trim_clo = c_abs;
  HIPCHK(h->probe.ensure(h->N));
  hipLaunchKernelGGL(trim_probe_kernel, dim3(h->N), dim3(64), 0, h->stream, h->capbuf.p,
                     h->cap_len, h->M, lo, hi, h->thr, sc_band(h->M), h->probe.p);
  HIPCHK(hipGetLastError());
  std::vector<uint32_t> ok(h->N);
  HIPCHK(hipMemcpyAsync(ok.data(), h->probe.p, sizeof(uint32_t) * h->N, hipMemcpyDeviceToHost,
                        h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (uint32_t a = 0; a < h->N; a++)
    if (!ok[a]) return MIMO_OK;                       // a run may reach back: keep everything
  // move [D, total) to the front in pieces of D samples (each piece's source is read before
  // any later piece writes over it: copies on one stream run in order; one piece when D >= keep)
  const uint64_t keep = h->total - D;
  for (uint64_t o = 0; o < keep; o += D) {
    const uint64_t m = std::min<uint64_t>(D, keep - o);
    HIPCHK(hipMemcpy2DAsync(h->capbuf.p + o, sizeof(float2) * h->cap_len,
                            h->capbuf.p + D + o, sizeof(float2) * h->cap_len,
                            sizeof(float2) * m, h->N, hipMemcpyDeviceToDevice, h->stream));
  }
  h->origin += D;
  h->total = keep;
  return MIMO_OK;
}

// At the trigger: nothing before the window start (base) is read again -- the S&C is done and
// the search, LS and decode read [base, base + ACB + TX) -- so the capture is re-based there
// into a buffer sized for the window (positions of the frame record shift with it).
static int rebase_to_window(mimo_rx *h, uint64_t piece) {
  const int64_t D = h->sinfo.base;
  if (D <= 0) return MIMO_OK;
  const uint64_t keep = h->total - (uint64_t)D;
  uint64_t nc = std::max<uint64_t>(keep, h->win_len + piece + 64);
  nc = (nc + 16383) / 16384 * 16384;
  float2 *np = nullptr;
  HIPCHK(hipMalloc(&np, sizeof(float2) * nc * h->N));
  if (keep)
    HIPCHK(hipMemcpy2DAsync(np, sizeof(float2) * nc, h->capbuf.p + D, sizeof(float2) * h->cap_len,
                            sizeof(float2) * keep, h->N, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->capbuf.adopt(np, nc * h->N);
  h->cap_len = nc;
  h->origin += (uint64_t)D;
  h->total = keep;
  FrameInfo &I = h->sinfo;   // (unsigned fields wrap consistently: getters add origin back)
  I.base -= D;
  I.trigger -= (uint64_t)D;
  I.sync_index -= (uint64_t)D;
  for (uint32_t a = 0; a < h->N; a++) {
    I.plateau_start[a] -= (uint64_t)D;
    I.plateau_end[a] -= (uint64_t)D;
  }
  return MIMO_OK;
}

// one piece of an execute call (at most a window's worth of samples)
static int execute_piece(mimo_rx *h, const float *const *iq, uint64_t off, uint64_t n,
                         uint64_t call_end, uint64_t piece) {
  if (h->state == MIMO_STATE_SEEK_PLATEAU && h->total) {
    int rc = maybe_trim(h);
    if (rc) return rc;
  }
  const uint64_t old_total = h->total;
  int rc = grow_capture(h, old_total + n);
  if (rc) return rc;
  for (uint32_t s = 0; s < h->N; s++)
    HIPCHK(hipMemcpyAsync(h->capbuf.p + (size_t)s * h->cap_len + old_total,
                          reinterpret_cast<const float2 *>(iq[s]) + off, sizeof(float2) * n,
                          hipMemcpyHostToDevice, h->stream));
  h->total = old_total + n;
  if (h->state == MIMO_STATE_SEEK_PLATEAU) {
    const uint64_t K = sc_chunk_len(h->cp);
    rc = ensure_workspace(h, 1, (h->total + K - 1) / K);
    if (rc) return rc;
    if (old_total == 0 && h->origin == 0)
      HIPCHK(hipMemsetAsync(h->ws.trig.p, 0xFF, sizeof(unsigned long long), h->stream));
    // re-run the partially filled chunk; earlier chunks are final (y[n] uses x[<=n] only)
    SyncRequest q{};
    q.chunk_lo = old_total / K;
    q.fpc = 1;
    rc = run_sync(h, Capture{h->capbuf.p, h->cap_len, h->total, 0, 1.0f}, 1, q, h->stream);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(&h->sinfo, h->ws.info.p, sizeof(FrameInfo), hipMemcpyDeviceToHost,
                          h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!h->dbg_fsc.empty()) {
      // DEBUG_LOG: y of every sample this piece processed while seeking, through the trigger
      const uint64_t hi = h->sinfo.status == MIMO_FRAME_NO_SYNC ? h->total : h->sinfo.trigger + 1;
      if (hi > old_total) {
        const uint64_t cnt = hi - old_total;
        HIPCHK(h->dbg_y.ensure(cnt * h->N));
        launch_sc_trace(h->capbuf.p, h->cap_len, h->N, h->M, (int64_t)old_total, (int64_t)hi,
                        h->dbg_y.p, h->stream);
        HIPCHK(hipGetLastError());
        std::vector<float> y(cnt * h->N);
        HIPCHK(hipMemcpyAsync(y.data(), h->dbg_y.p, sizeof(float) * y.size(),
                              hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (uint32_t a = 0; a < h->N; a++)
          if (fwrite(y.data() + (size_t)a * cnt, sizeof(float), cnt, h->dbg_fsc[a]) != cnt)
            return fail(MIMO_ERR_ARG, "short write of an f_sc debug file");
      }
    }
    if (h->sinfo.status == MIMO_FRAME_NO_SYNC) {
      h->nsp = h->origin + h->total;
      return MIMO_OK;
    }
    h->have_sync = true;
    h->state = MIMO_STATE_SAVE_ACCESS_CODES;
    rc = rebase_to_window(h, piece);
    if (rc) return rc;
  }
  // SAVE_ACCESS_CODES (framing.cc:639-651): estimate_channel runs at window sample n_e =
  // base + ACB + TX; a call that continues past it consumes one more sample in STATE_MIMO
  // (framing.cc:494-503)
  const uint64_t n_e = (uint64_t)h->sinfo.base + h->win_len;   // capture-relative
  if (n_e < h->total) {
    h->nsp = h->origin + n_e + ((h->origin + n_e + 1 < call_end) ? 2 : 1);
    rc = finish_estimate(h);
    if (rc) return rc;
    h->state = MIMO_STATE_MIMO;
  } else {
    h->nsp = h->origin + h->total;
  }
  return MIMO_OK;
}

int mimo_rx_execute(mimo_rx *h, const float *const *iq, uint32_t n_ant, uint64_t n,
                    int32_t *state_out) {
  if (!h || (!iq && n)) return fail(MIMO_ERR_ARG, "null argument");
  if (n_ant != h->N) return fail(MIMO_ERR_ARG, "n_ant must equal num_streams");
  if (h->state == MIMO_STATE_MIMO) {   // framing.cc:494-503: consume one sample and break
    if (n) h->nsp += 1;
    if (state_out) *state_out = h->state;
    return MIMO_OK;
  }
  // long calls are taken a window at a time, so the capture stays bounded whatever the
  // caller's chunking (results are those of one call: the S&C is chunk-exact)
  const uint64_t call_end = h->origin + h->total + n;
  const uint64_t piece = std::max<uint64_t>(h->win_len / 2, 2 * sc_chunk_len(h->cp));
  for (uint64_t off = 0; off < n && h->state != MIMO_STATE_MIMO; off += piece) {
    const int rc = execute_piece(h, iq, off, std::min<uint64_t>(piece, n - off), call_end, piece);
    if (rc) return rc;
  }
  if (state_out) *state_out = h->state;
  return MIMO_OK;
}

}  // extern "C"
