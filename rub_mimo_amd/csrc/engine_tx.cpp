// rub_mimo_amd/csrc/engine_tx.cpp -- the transmitter (framegen), the synthetic-capture
// generator and the subcarrier-type / m-sequence helpers of include/mimo_rx.h.
#include "engine_internal.hpp"

extern "C" {

// ---------------- transmitter ----------------
int mimo_tx_create(uint32_t M, uint32_t cp, uint32_t N, uint32_t nac, const uint8_t *p,
                   const uint8_t *s0_bits, const uint8_t *s1_bits, mimo_tx **out) {
  if (!p || !s0_bits || !s1_bits || !out) return fail(MIMO_ERR_ARG, "null argument");
  const int l2 = ilog2(M);
  if (l2 < 6 || l2 > 12) return fail(MIMO_ERR_UNSUPPORTED, "M must be a power of two in [64, 4096]");
  if (N == 0 || N > MIMO_MAX_STREAMS || cp == 0 || cp > M / 2 || nac == 0)
    return fail(MIMO_ERR_ARG, "bad framegen parameters");
  uint32_t n0, n1, n2;
  int rc = validate_sctype(p, M, &n0, &n1, &n2);
  if (rc) return rc;
  mimo_tx *h = new mimo_tx();
  h->M = M; h->cp = cp; h->SL = M + cp; h->N = N; h->nac = nac; h->M_occ = n1 + n2;
  h->log2M = l2;
  h->dn = 1.0f / sqrtf((float)h->M_occ);   // framing.cc:115
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return fail(MIMO_ERR_HIP, "hipStreamCreate failed");
  }
  rc = get_twiddles(&h->tw);
  if (!rc) rc = build_codes(h->codes, M, N, nac, p, s0_bits, s1_bits, l2 + 1, false, h->stream);
  if (rc) { mimo_tx_destroy(h); return rc; }
  const uint32_t n_slots = N * nac + 1;
  std::vector<float2> all((size_t)n_slots * M);
  std::vector<int32_t> occ;
  for (uint32_t i = 0; i < M; i++) if (p[i] != MIMO_SC_NULL) occ.push_back((int32_t)i);
  if (hipMemcpy(all.data(), h->codes.code_time.p, sizeof(float2) * all.size(),
                hipMemcpyDeviceToHost) != hipSuccess ||
      h->occ_list.ensure(occ.size()) != hipSuccess ||
      hipMemcpy(h->occ_list.p, occ.data(), sizeof(int32_t) * occ.size(),
                hipMemcpyHostToDevice) != hipSuccess) {
    mimo_tx_destroy(h);
    return fail(MIMO_ERR_HIP, "framegen table upload failed");
  }
  h->s0.assign(all.begin(), all.begin() + M);
  // regroup slot-major (slot = 1 + code*N + t) into per-stream [t][code*M + i]
  h->s1.resize((size_t)N * nac * M);
  for (uint32_t c = 0; c < nac; c++)
    for (uint32_t t = 0; t < N; t++)
      std::memcpy(h->s1.data() + ((size_t)t * nac + c) * M,
                  all.data() + (size_t)(1 + c * N + t) * M, sizeof(float2) * M);
  *out = h;
  return MIMO_OK;
}

int mimo_tx_destroy(mimo_tx *h) {
  if (!h) return MIMO_OK;
  if (h->stream) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamDestroy(h->stream);
  }
  delete h;
  return MIMO_OK;
}

int mimo_tx_get_codes(mimo_tx *h, float *s0, float *s1) {
  if (!h) return fail(MIMO_ERR_ARG, "null handle");
  if (s0) std::memcpy(s0, h->s0.data(), sizeof(float2) * h->s0.size());
  if (s1) std::memcpy(s1, h->s1.data(), sizeof(float2) * h->s1.size());
  return MIMO_OK;
}

int mimo_tx_write_sync_words(mimo_tx *h, float *const *tx, uint32_t *n_written) {
  // framing.cc:169-208: S0 (CP + body) on stream 0, then nac x N TDMA slots of S1
  if (!h || !tx) return fail(MIMO_ERR_ARG, "null argument");
  const uint32_t M = h->M, cp = h->cp, total = (h->nac * h->N + 1) * h->SL;
  for (uint32_t s = 0; s < h->N; s++) std::memset(tx[s], 0, sizeof(float2) * total);
  uint32_t idx = 0;
  auto put = [&](uint32_t s, const float2 *code) {
    std::memcpy(reinterpret_cast<float2 *>(tx[s]) + idx, code + M - cp, sizeof(float2) * cp);
    idx += cp;
    std::memcpy(reinterpret_cast<float2 *>(tx[s]) + idx, code, sizeof(float2) * M);
    idx += M;
  };
  put(0, h->s0.data());
  for (uint32_t ac = 0; ac < h->nac; ac++)
    for (uint32_t s = 0; s < h->N; s++) put(s, h->s1.data() + ((size_t)s * h->nac + ac) * M);
  if (n_written) *n_written = idx;
  return MIMO_OK;
}

int mimo_tx_assemble_mimo_packet(mimo_tx *h, float *const *tx, const float *const *in,
                                 uint32_t *n_written) {
  if (!h || !tx || !in) return fail(MIMO_ERR_ARG, "null argument");
  const size_t per = h->M_occ;
  HIPCHK(h->din.ensure(per * h->N));
  HIPCHK(h->dout.ensure((size_t)h->SL * h->N));
  for (uint32_t t = 0; t < h->N; t++)
    HIPCHK(hipMemcpyAsync(h->din.p + t * per, in[t], sizeof(float2) * per, hipMemcpyHostToDevice,
                          h->stream));
  TxSymArgs a{};
  a.N = h->N; a.M = h->M; a.cp = h->cp; a.M_occ = h->M_occ; a.dn = h->dn; a.gain = 1.0f;
  a.occ_list = h->occ_list.p; a.in = h->din.p; a.n_sym = 1; a.out = h->dout.p; a.tw = h->tw;
  a.qam = make_qam(4);
  launch_tx_symbols(a, h->log2M, 1, h->stream);
  HIPCHK(hipGetLastError());
  for (uint32_t t = 0; t < h->N; t++)
    HIPCHK(hipMemcpyAsync(tx[t], h->dout.p + (size_t)t * h->SL, sizeof(float2) * h->SL,
                          hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (n_written) *n_written = h->SL;
  return MIMO_OK;
}

// ---------------- synthetic captures ----------------
static uint64_t synth_offset(const mimo_synth_config *c, uint64_t frame_id) {
  const uint64_t SL = c->M + c->cp_len;
  if (c->offset >= 0) return (uint64_t)c->offset;
  // ref_hash5(seed, DOM_OFFSET, frame, 0, 0) % SL on the host (same mixer as the kernels)
  auto mix = [](uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  };
  uint64_t hh = mix(c->seed ^ ((uint64_t)DOM_OFFSET * 0xD6E8FEB86659FD93ull));
  hh = mix(hh ^ frame_id);
  hh = mix(hh ^ 0ull);
  hh = mix(hh ^ 0ull);
  return hh % SL;
}

int mimo_synth_frame_len(const mimo_synth_config *c, uint64_t frame_id, uint64_t *len) {
  if (!c || !len) return fail(MIMO_ERR_ARG, "null argument");
  const uint64_t SL = c->M + c->cp_len;
  *len = SL * (2ull * c->num_streams * c->num_access_codes + 2 + c->pid + c->tail_syms) +
         synth_offset(c, frame_id);
  return MIMO_OK;
}

// the synthesiser: the data symbols are the caller's indices (idx_in) or the hash draw, which
// tx_idx (optional) receives
static int synth_frames(const mimo_synth_config *c, uint64_t frame_id0, uint32_t n_frames,
                        void *d_out, uint64_t stride, uint64_t frame_len, void *d_tx_idx,
                        const void *d_idx_in, void *d_H, void *hip_stream) {
  if (!c || !d_out || !c->p || !c->s0_bits || !c->s1_bits)
    return fail(MIMO_ERR_ARG, "null argument");
  const int l2 = ilog2(c->M);
  if (l2 < 6 || l2 > 12) return fail(MIMO_ERR_UNSUPPORTED, "M must be a power of two in [64, 4096]");
  const uint32_t N = c->num_streams;
  if (N == 0 || N > MIMO_MAX_STREAMS) return fail(MIMO_ERR_ARG, "bad num_streams");
  if (stride < frame_len) return fail(MIMO_ERR_ARG, "stride < frame_len");
  uint32_t n0, n1, n2;
  int rc = validate_sctype(c->p, c->M, &n0, &n1, &n2);
  if (rc) return rc;
  const uint32_t M_occ = n1 + n2, SL = c->M + c->cp_len;
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : nullptr;
  Codes codes;
  rc = build_codes(codes, c->M, N, c->num_access_codes, c->p, c->s0_bits, c->s1_bits, l2 + 1,
                   false, s);
  if (rc) return rc;
  float2 *tw = nullptr;
  rc = get_twiddles(&tw);
  if (rc) return rc;
  std::vector<int32_t> occ;
  for (uint32_t i = 0; i < c->M; i++) if (c->p[i] != MIMO_SC_NULL) occ.push_back((int32_t)i);
  DevBuf<int32_t> docc;
  HIPCHK(docc.ensure(occ.size()));
  HIPCHK(hipMemcpy(docc.p, occ.data(), sizeof(int32_t) * occ.size(), hipMemcpyHostToDevice));
  // frames in groups so the TX scratch stays bounded (~1 GiB)
  const uint64_t per_frame = (uint64_t)N * std::max<uint32_t>(c->pid, 1) * SL;
  uint32_t group = (uint32_t)std::max<uint64_t>(1, (128ull << 20) / per_frame);
  group = std::min(group, n_frames);
  DevBuf<float2> scratch;
  HIPCHK(scratch.ensure(per_frame * group));
  const Qam qam = make_qam(c->qam_order);
  const float nstd = (float)std::sqrt(0.0625 * std::pow(10.0, -(double)c->snr_db / 10.0));
  for (uint32_t f0 = 0; f0 < n_frames; f0 += group) {
    const uint32_t nf = std::min(group, n_frames - f0);
    if (c->pid) {
      TxSymArgs a{};
      a.N = N; a.M = c->M; a.cp = c->cp_len; a.M_occ = M_occ;
      a.dn = 1.0f / sqrtf((float)M_occ); a.gain = 0.25f;
      a.occ_list = docc.p; a.in = nullptr; a.n_sym = c->pid; a.seed = c->seed;
      a.frame_id0 = frame_id0 + f0; a.qam = qam;
      const size_t idx0 = (size_t)f0 * N * c->pid * M_occ;
      a.tx_idx = d_tx_idx ? reinterpret_cast<uint8_t *>(d_tx_idx) + idx0 : nullptr;
      a.idx_in = d_idx_in ? reinterpret_cast<const uint8_t *>(d_idx_in) + idx0 : nullptr;
      a.out = scratch.p; a.tw = tw;
      launch_tx_symbols(a, l2, nf, s);
    }
    MixArgs m{};
    m.N = N; m.M = c->M; m.cp = c->cp_len; m.SL = SL; m.nac = c->num_access_codes;
    m.pid = c->pid; m.seed = c->seed; m.frame_id0 = frame_id0 + f0; m.offset = c->offset;
    m.identity = c->identity_channel; m.nstd = nstd; m.code_time = codes.code_time.p;
    m.tx_data = scratch.p;
    m.out = reinterpret_cast<float2 *>(d_out) + (size_t)f0 * N * stride;
    m.stride = stride; m.frame_len = frame_len;
    m.H_out = d_H ? reinterpret_cast<float2 *>(d_H) + (size_t)f0 * N * N : nullptr;
    launch_mix(m, nf, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
  }
  return MIMO_OK;
}

int mimo_synth_frames(const mimo_synth_config *c, uint64_t frame_id0, uint32_t n_frames,
                      void *d_out, uint64_t stride, uint64_t frame_len, void *d_tx_idx,
                      void *d_H, void *hip_stream) {
  return synth_frames(c, frame_id0, n_frames, d_out, stride, frame_len, d_tx_idx, nullptr, d_H,
                      hip_stream);
}

int mimo_synth_frames_payload(const mimo_synth_config *c, uint64_t frame_id0, uint32_t n_frames,
                              void *d_out, uint64_t stride, uint64_t frame_len,
                              const void *d_tx_idx, void *d_H, void *hip_stream) {
  if (c && c->pid && !d_tx_idx) return fail(MIMO_ERR_ARG, "d_tx_idx is null with pid > 0");
  return synth_frames(c, frame_id0, n_frames, d_out, stride, frame_len, nullptr, d_tx_idx, d_H,
                      hip_stream);
}

// ---------------- helpers ----------------
int mimo_sctype_default(uint8_t *p, uint32_t M) {   // framing.cc:949-954
  if (!p) return fail(MIMO_ERR_ARG, "null argument");
  for (uint32_t i = 0; i < M; i++) p[i] = MIMO_SC_DATA;
  return MIMO_OK;
}

int mimo_sctype_liquid(uint8_t *p, uint32_t M) {    // framing.cc:956-997
  if (!p) return fail(MIMO_ERR_ARG, "null argument");
  const uint32_t M2 = M / 2;
  uint32_t G = std::max<uint32_t>(M / 10, 2);
  const uint32_t P = (M > 34) ? 8 : 4, P2 = P / 2;
  for (uint32_t i = 0; i < M; i++) p[i] = MIMO_SC_NULL;
  for (uint32_t i = 1; i + G < M2; i++) {
    const uint8_t v = (((i + P2) % P) == 0) ? MIMO_SC_PILOT : MIMO_SC_DATA;
    p[i] = v;
    p[M - i] = v;
  }
  return MIMO_OK;
}

int mimo_sctype_validate(const uint8_t *p, uint32_t M, uint32_t *a, uint32_t *b, uint32_t *c) {
  if (!p || !a || !b || !c) return fail(MIMO_ERR_ARG, "null argument");
  return validate_sctype(p, M, a, b, c);
}

int mimo_msequence_draw_bits(uint32_t m, uint32_t g, uint32_t a, uint32_t count, uint8_t *out) {
  // liquid msequence_create / msequence_generate_symbol(ms,1)
  if (!out || m < 2 || m > 31) return fail(MIMO_ERR_ARG, "bad msequence parameters");
  uint32_t gg = g >> 1, v = 0;
  for (uint32_t i = 0; i < m; i++) { v = (v << 1) | (a & 1u); a >>= 1; }
  const uint32_t n = (1u << m) - 1u;
  for (uint32_t i = 0; i < count; i++) {
    const uint32_t b = (uint32_t)__builtin_parity(v & gg);
    v = ((v << 1) | b) & n;
    out[i] = (uint8_t)b;
  }
  return MIMO_OK;
}

}  // extern "C"
