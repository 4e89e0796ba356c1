// rub_mimo_amd/csrc/engine.cpp -- host side of librub_mimo_amd.so, the C-ABI of
// include/mimo_rx.h: the handles' life cycle (device tables, code construction), the
// configuration setters, the plain getters, and the device / memcpy helpers. The stage
// drivers, the batch and streaming paths, the transmitter and the diagnostics live in the
// other engine_*.cpp files (see engine_internal.hpp).
#include <mutex>

#include "engine_internal.hpp"

namespace {

thread_local std::string g_err;

// twiddle table tw[k] = exp(-2 pi i k / kTwN), shared by all handles (device 0 of the caller)
std::mutex g_tw_mu;
float2 *g_tw = nullptr;
int g_tw_dev = -1;

}  // namespace

namespace mimo {

// the one error slot of a thread, for every host translation unit
int host_fail(int code, const char *msg) {
  g_err = msg;
  return code;
}

int get_twiddles(float2 **out) {
  std::lock_guard<std::mutex> lk(g_tw_mu);
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  if (!g_tw || g_tw_dev != dev) {
    std::vector<float2> h(kTwN);
    for (int k = 0; k < kTwN; k++) {
      const double a = -2.0 * M_PI * (double)k / (double)kTwN;
      h[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    float2 *d = nullptr;
    HIPCHK(hipMalloc(&d, sizeof(float2) * kTwN));
    HIPCHK(hipMemcpy(d, h.data(), sizeof(float2) * kTwN, hipMemcpyHostToDevice));
    g_tw = d;
    g_tw_dev = dev;
  }
  *out = g_tw;
  return MIMO_OK;
}

Qam make_qam(uint32_t order) {
  Qam q;
  uint32_t b = 0;
  while ((1u << (2 * b)) < order) b++;
  q.b = b;
  q.L = 1u << b;
  const double e = 2.0 * ((double)q.L * q.L - 1.0) / 3.0;
  q.scale = (float)(1.0 / std::sqrt(e));
  q.inv_scale = (float)std::sqrt(e);
  return q;
}

int validate_sctype(const uint8_t *p, uint32_t M, uint32_t *n0, uint32_t *n1, uint32_t *n2) {
  uint32_t a = 0, b = 0, c = 0;
  for (uint32_t i = 0; i < M; i++) {
    if (p[i] == MIMO_SC_NULL) a++;
    else if (p[i] == MIMO_SC_PILOT) b++;
    else if (p[i] == MIMO_SC_DATA) c++;
    else return fail(MIMO_ERR_SCTYPE, "invalid subcarrier type " + std::to_string(p[i]));
  }
  *n0 = a; *n1 = b; *n2 = c;
  return MIMO_OK;
}

int build_codes(Codes &c, uint32_t M, uint32_t N, uint32_t nac, const uint8_t *p,
                const uint8_t *s0_bits, const uint8_t *s1_bits, int log2F, bool spectra,
                hipStream_t s) {
  const uint32_t n_slots = N * nac + 1;
  uint32_t n0, n1, n2;
  int rc = validate_sctype(p, M, &n0, &n1, &n2);
  if (rc) return rc;
  uint32_t m_s0 = 0;
  for (uint32_t i = 0; i < M; i += 2)
    if (p[i] != MIMO_SC_NULL) m_s0++;
  if (m_s0 == 0) return fail(MIMO_ERR_SCTYPE, "ofdmframe_init_S0: no subcarriers enabled");
  DevBuf<uint8_t> dp, d0, d1;
  HIPCHK(dp.ensure(M));
  HIPCHK(d0.ensure(M));
  HIPCHK(d1.ensure((size_t)N * nac * M));
  HIPCHK(hipMemcpyAsync(dp.p, p, M, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d0.p, s0_bits, M, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d1.p, s1_bits, (size_t)N * nac * M, hipMemcpyHostToDevice, s));
  HIPCHK(c.code_time.ensure((size_t)n_slots * M));
  const uint32_t F = 1u << log2F;
  if (spectra) HIPCHK(c.codespec.ensure((size_t)n_slots * F));
  if (spectra && F >= 1024) HIPCHK(c.codespec_w.ensure((size_t)n_slots * F));
  CodesArgs a{};
  a.M = M; a.N = N; a.nac = nac; a.n_slots = n_slots;
  a.p = dp.p; a.s0_bits = d0.p; a.s1_bits = d1.p;
  a.dn_s0 = (float)std::sqrt(1.0 / (double)(float)m_s0);   // framing.cc:1100
  a.dn_s1 = (float)std::sqrt(1.0 / (double)(float)M);      // framing.cc:1228
  a.code_time = c.code_time.p;
  a.codespec = spectra ? c.codespec.p : nullptr;
  a.codespec_w = (spectra && F >= 1024) ? c.codespec_w.p : nullptr;
  int rc2 = get_twiddles(const_cast<float2 **>(&a.tw));
  if (rc2) return rc2;
  launch_codes(a, ilog2(M), log2F, s);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s));  // the staging buffers die with this scope
  return MIMO_OK;
}

int copy_W(mimo_rx *h, uint32_t f, float *W) {
  const size_t n = (size_t)h->M * h->N * h->N;
  std::vector<float2> tmp(n);
  HIPCHK(hipMemcpy(tmp.data(), h->ws.W.p + (size_t)f * n, sizeof(float2) * n,
                   hipMemcpyDeviceToHost));
  float2 *o = reinterpret_cast<float2 *>(W);
  for (uint32_t t = 0; t < h->N; t++)
    for (uint32_t r = 0; r < h->N; r++)
      for (uint32_t k = 0; k < h->M; k++)
        o[((size_t)k * h->N + t) * h->N + r] = tmp[((size_t)t * h->N + r) * h->M + k];
  return MIMO_OK;
}

int copy_corr(mimo_rx *h, uint32_t F, uint32_t *corr, uint32_t *s0) {
  std::vector<unsigned long long> k((size_t)F * h->N * h->n_slots);
  HIPCHK(hipMemcpy(k.data(), h->ws.keys.p, sizeof(unsigned long long) * k.size(),
                   hipMemcpyDeviceToHost));
  auto idx = [](unsigned long long v) -> uint32_t {
    return v ? (0xFFFFFFFFu - (uint32_t)(v & 0xFFFFFFFFull)) : 0u;
  };
  for (uint32_t f = 0; f < F; f++)
    for (uint32_t r = 0; r < h->N; r++) {
      const unsigned long long *kk = k.data() + ((size_t)f * h->N + r) * h->n_slots;
      if (s0) s0[f * h->N + r] = idx(kk[0]);
      if (corr)
        for (uint32_t ac = 0; ac + 1 < h->n_slots; ac++)
          corr[((size_t)f * h->N + r) * (h->n_slots - 1) + ac] = idx(kk[1 + ac]);
    }
  return MIMO_OK;
}

}  // namespace mimo

extern "C" {

const char *mimo_last_error(void) { return g_err.c_str(); }
const char *mimo_version(void) { return "rub_mimo_amd 0.1.0 (gfx950)"; }

static void close_debug_files(mimo_rx *h) {
  for (FILE *f : h->dbg_fsc)
    if (f) fclose(f);
  h->dbg_fsc.clear();
}

int mimo_rx_create(const mimo_rx_config *cfg, void *hip_stream, mimo_rx **out) {
  if (!cfg || !out || !cfg->p || !cfg->s0_bits || !cfg->s1_bits)
    return fail(MIMO_ERR_ARG, "mimo_rx_create: null argument");
  *out = nullptr;
  const int l2 = ilog2(cfg->M);
  if (l2 < 6 || l2 > 12) return fail(MIMO_ERR_UNSUPPORTED, "M must be a power of two in [64, 4096]");
  const uint32_t N = cfg->num_streams;
  if (!(N == 1 || N == 2 || N == 4 || N == 8))
    return fail(MIMO_ERR_UNSUPPORTED, "num_streams must be 1, 2, 4 or 8");
  if (cfg->cp_len == 0 || cfg->cp_len > cfg->M / 2)
    return fail(MIMO_ERR_ARG, "cp_len must be in [1, M/2]");
  if (cfg->num_access_codes == 0) return fail(MIMO_ERR_ARG, "num_access_codes must be > 0");
  if (cfg->detector < 0 || cfg->detector > 3) return fail(MIMO_ERR_ARG, "bad detector");
  if ((cfg->detector == MIMO_DET_ZF2) && N != 2)
    return fail(MIMO_ERR_ARG, "the reference invert() is 2x2 only (framing.cc:1346)");
  if (cfg->detector == MIMO_DET_SISO && (cfg->siso_tx >= N || cfg->siso_rx >= N))
    return fail(MIMO_ERR_ARG, "siso_tx/siso_rx out of range");
  const uint32_t q = cfg->qam_order;
  if (!(q == 4 || q == 16 || q == 64 || q == 256))
    return fail(MIMO_ERR_ARG, "qam_order must be 4, 16, 64 or 256");
  mimo_rx *h = new mimo_rx();
  h->M = cfg->M; h->cp = cfg->cp_len; h->SL = h->M + h->cp; h->N = N;
  h->nac = cfg->num_access_codes; h->pid = cfg->pid_max;
  h->log2M = l2;
  h->p.assign(cfg->p, cfg->p + h->M);
  int rc = validate_sctype(h->p.data(), h->M, &h->M_null, &h->M_pilot, &h->M_data);
  if (rc) { delete h; return rc; }
  h->M_occ = h->M_pilot + h->M_data;
  if (h->M_occ == 0) { delete h; return fail(MIMO_ERR_SCTYPE, "no occupied subcarriers"); }
  h->occ_index.resize(h->M);
  std::vector<int8_t> sign((size_t)N * h->nac * h->M);
  for (uint32_t i = 0, j = 0; i < h->M; i++) h->occ_index[i] = (h->p[i] != MIMO_SC_NULL) ? (int32_t)j++ : -1;
  for (uint32_t t = 0; t < N; t++)
    for (uint32_t c = 0; c < h->nac; c++)
      for (uint32_t i = 0; i < h->M; i++) {
        const size_t o = ((size_t)t * h->nac + c) * h->M + i;
        sign[o] = (h->p[i] == MIMO_SC_NULL) ? 0 : ((cfg->s1_bits[o] & 1) ? 1 : -1);
      }
  h->det = cfg->detector;
  h->noise_var = cfg->noise_var;
  h->keep_bias = cfg->keep_identity_bias ? 1 : 0;
  h->siso_tx = cfg->siso_tx; h->siso_rx = cfg->siso_rx;
  h->thr = cfg->plateau_threshold;
  h->cfo = cfg->cfo_correct != 0;
  h->qam = make_qam(q);
  h->acb = (uint64_t)h->SL * (h->nac * N + 4);     // framing.cc:284
  h->txl = (uint64_t)h->pid * h->SL;               // framing.cc:285
  h->win_len = h->acb + h->txl;
  h->dn = 1.0f / sqrtf((float)h->M_occ);           // framing.cc:330
  h->ls_scale = h->dn / (float)h->nac;             // framing.cc:821
  h->nv_norm = (h->nac >= 2) ? ((double)h->dn * (double)h->dn /
                                ((double)h->M_occ * N * N * (h->nac - 1)))
                             : 0.0;
  // search transform. Fused search + LS (search_ls_kernel): two slots per transform,
  // F >= 2 SL + M - 1, up to 16384. Otherwise F >= SL + M - 1 lags+taps, capped at 8192 (then
  // several lag chunks per slot) and a separate LS pass.
  uint32_t F = 1;
  while (F < 2 * h->SL + h->M - 1 || F < 2 * h->M) F <<= 1;
  h->search_ls = F <= 16384 && search_ls_supported(ilog2(F), ilog2(h->M));
  if (!h->search_ls) {
    F = 1;
    while (F < h->SL + h->M - 1) F <<= 1;
    if (F > 8192) F = 8192;
    if (F < 2 * h->M) F = 2 * h->M;
  }
  h->F = F; h->log2F = ilog2(F);
  h->lagc = F - h->M + 1;
  h->n_lagc = (h->SL + h->lagc - 1) / h->lagc;
  h->n_slots = N * h->nac + 1;
  if (hip_stream) {
    h->stream = (hipStream_t)hip_stream;
  } else {
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
      delete h;
      return fail(MIMO_ERR_HIP, "hipStreamCreate failed");
    }
    h->own_stream = true;
  }
  {
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        ncu > 0)
      h->n_cu = (uint32_t)ncu;
  }
  rc = get_twiddles(&h->tw);
  if (!rc) rc = build_codes(h->codes, h->M, N, h->nac, h->p.data(), cfg->s0_bits, cfg->s1_bits,
                            h->log2F, true, h->stream);
  if (rc) { mimo_rx_destroy(h); return rc; }
  uint32_t m_s0 = 0;
  for (uint32_t i = 0; i < h->M; i += 2) if (h->p[i] != MIMO_SC_NULL) m_s0++;
  std::vector<float> vs(h->n_slots);
  const double FF = (double)F * (double)F, MM = (double)h->M * (double)h->M;
  vs[0] = (float)((double)m_s0 / (MM * FF));
  for (uint32_t sl = 1; sl < h->n_slots; sl++) vs[sl] = (float)(1.0 / ((double)h->M * FF));
  // ls_window_kernel's sign table (512 <= M <= 4096): thread lt's 8 subcarriers lt + (M/8) e
  // adjacent
  if (ls_window_supported(h->log2M, h->nac, false)) {
    const uint32_t T = h->M / 8;
    std::vector<int8_t> sw(sign.size());
    for (size_t row = 0; row < (size_t)N * h->nac; row++)
      for (uint32_t lt = 0; lt < T; lt++)
        for (uint32_t e = 0; e < 8; e++) sw[row * h->M + 8 * lt + e] = sign[row * h->M + lt + T * e];
    if (h->s1sign_w.ensure(sw.size()) != hipSuccess ||
        hipMemcpy(h->s1sign_w.p, sw.data(), sw.size(), hipMemcpyHostToDevice) != hipSuccess) {
      mimo_rx_destroy(h);
      return fail(MIMO_ERR_HIP, "table upload failed");
    }
  }
  if (h->vscale.ensure(h->n_slots) != hipSuccess || h->s1sign.ensure(sign.size()) != hipSuccess ||
      h->occ.ensure(h->M) != hipSuccess ||
      hipMemcpy(h->vscale.p, vs.data(), sizeof(float) * vs.size(), hipMemcpyHostToDevice) !=
          hipSuccess ||
      hipMemcpy(h->s1sign.p, sign.data(), sign.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->occ.p, h->occ_index.data(), sizeof(int32_t) * h->M, hipMemcpyHostToDevice) !=
          hipSuccess) {
    mimo_rx_destroy(h);
    return fail(MIMO_ERR_HIP, "table upload failed");
  }
  *out = h;
  return MIMO_OK;
}

int mimo_rx_destroy(mimo_rx *h) {
  if (!h) return MIMO_OK;
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  close_debug_files(h);
  for (auto &e : h->timer.ev) {
    (void)hipEventDestroy(e.second.first);
    (void)hipEventDestroy(e.second.second);
  }
  for (auto &g : h->graphs)
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return MIMO_OK;
}

// ---------------- configuration setters ----------------
int mimo_rx_set_callback(mimo_rx *h, mimo_rx_symbol_cb cb, void *user) {
  if (!h) return fail(MIMO_ERR_ARG, "null handle");
  h->cb = cb;
  h->user = user;
  return MIMO_OK;
}

int mimo_rx_set_siso(mimo_rx *h, uint32_t tx, uint32_t rx) {
  if (!h || tx >= h->N || rx >= h->N) return fail(MIMO_ERR_ARG, "siso index out of range");
  if (tx != h->siso_tx || rx != h->siso_rx) invalidate_graph(h);
  h->siso_tx = tx;
  h->siso_rx = rx;
  return MIMO_OK;
}

int mimo_rx_set_grid_cus(mimo_rx *h, uint32_t n_cu) {
  if (!h) return fail(MIMO_ERR_ARG, "null handle");
  int dev = 0, ncu = 0;
  if (n_cu == 0 && hipGetDevice(&dev) == hipSuccess &&
      hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0)
    n_cu = (uint32_t)ncu;
  if (n_cu == 0) return fail(MIMO_ERR_ARG, "no CU count");
  h->n_cu = n_cu;
  return MIMO_OK;
}

int mimo_rx_set_timing(mimo_rx *h, int enable) {
  if (!h) return fail(MIMO_ERR_ARG, "null handle");
  h->timer.on = enable != 0;
  return MIMO_OK;
}

int mimo_rx_set_debug_log(mimo_rx *h, const char *dir) {
  if (!h) return fail(MIMO_ERR_ARG, "null handle");
  close_debug_files(h);
  h->dbg_dir.clear();
  if (!dir || !dir[0]) return MIMO_OK;
  h->dbg_dir = dir;
  for (uint32_t a = 0; a < h->N; a++) {   // framing.cc:390-402: f_sc_<k>.dat, k from 1
    const std::string fn = h->dbg_dir + "/f_sc_" + std::to_string(a + 1) + ".dat";
    FILE *f = fopen(fn.c_str(), "wb");
    if (!f) {
      close_debug_files(h);
      h->dbg_dir.clear();
      return fail(MIMO_ERR_ARG, "cannot open " + fn);
    }
    h->dbg_fsc.push_back(f);
  }
  return MIMO_OK;
}

// ---------------- streaming state and plain getters ----------------
int mimo_rx_reset(mimo_rx *h) {
  // framing.cc:461-464 only rewinds the state; here the receiver re-arms on a fresh capture
  // (documented deviation: the reference keeps stale S&C filter history and accumulates
  // sync_index across resets).
  if (!h) return fail(MIMO_ERR_ARG, "null handle");
  HIPCHK(hipStreamSynchronize(h->stream));
  h->state = MIMO_STATE_SEEK_PLATEAU;
  h->total = 0;
  h->origin = 0;
  h->trim_clo = ~0ull;
  h->nsp = 0;
  h->have_sync = false;
  h->have_est = false;
  return MIMO_OK;
}

int mimo_rx_get_state(const mimo_rx *h, int32_t *st) {
  if (!h || !st) return fail(MIMO_ERR_ARG, "null argument");
  *st = h->state;
  return MIMO_OK;
}

int mimo_rx_get_sync_index(const mimo_rx *h, uint64_t *out) {
  if (!h || !out) return fail(MIMO_ERR_ARG, "null argument");
  *out = h->have_sync ? h->origin + h->sinfo.sync_index : 0;
  return MIMO_OK;
}

int mimo_rx_get_num_samples_processed(const mimo_rx *h, uint64_t *out) {
  if (!h || !out) return fail(MIMO_ERR_ARG, "null argument");
  *out = h->nsp;
  return MIMO_OK;
}

int mimo_rx_get_plateau(const mimo_rx *h, uint32_t s, uint64_t *start, uint64_t *end) {
  if (!h || s >= h->N) return fail(MIMO_ERR_ARG, "bad stream");
  if (start) *start = h->have_sync ? h->origin + h->sinfo.plateau_start[s] : 0;
  if (end) *end = h->have_sync ? h->origin + h->sinfo.plateau_end[s] : 0;
  return MIMO_OK;
}

int mimo_rx_get_m_occ(const mimo_rx *h, uint32_t *m) {
  if (!h || !m) return fail(MIMO_ERR_ARG, "null argument");
  *m = h->M_occ;
  return MIMO_OK;
}

int mimo_rx_get_G(mimo_rx *h, float *G) {
  if (!h || !G) return fail(MIMO_ERR_ARG, "null argument");
  const size_t n = (size_t)h->M * h->N * h->N;
  if (!h->have_est) {   // framing.cc:302-319 identity on occupied carriers
    std::memset(G, 0, sizeof(float2) * n);
    for (uint32_t k = 0; k < h->M; k++)
      if (h->p[k] != MIMO_SC_NULL)
        for (uint32_t r = 0; r < h->N; r++) G[2 * ((k * h->N + r) * h->N + r)] = 1.0f;
    return MIMO_OK;
  }
  HIPCHK(hipMemcpy(G, h->ws.G.p, sizeof(float2) * n, hipMemcpyDeviceToHost));
  return MIMO_OK;
}

int mimo_rx_get_W(mimo_rx *h, float *W) {
  if (!h || !W) return fail(MIMO_ERR_ARG, "null argument");
  if (!h->have_est) return mimo_rx_get_G(h, W);  // W also starts as identity
  return copy_W(h, 0, W);
}

int mimo_rx_get_gain(mimo_rx *h, float *gain) {
  if (!h || !gain) return fail(MIMO_ERR_ARG, "null argument");
  if (!h->have_est) {
    for (uint32_t j = 0; j < h->M_occ; j++) gain[j] = 1.0f;
    return MIMO_OK;
  }
  std::vector<float> tmp(h->M);
  HIPCHK(hipMemcpy(tmp.data(), h->ws.gain.p, sizeof(float) * h->M, hipMemcpyDeviceToHost));
  for (uint32_t k = 0; k < h->M; k++)
    if (h->occ_index[k] >= 0) gain[h->occ_index[k]] = tmp[k];
  return MIMO_OK;
}

int mimo_rx_get_noise_var(mimo_rx *h, float *out) {
  if (!h || !out) return fail(MIMO_ERR_ARG, "null argument");
  *out = h->have_est ? h->sinfo.noise_var : h->noise_var;
  return MIMO_OK;
}

int mimo_rx_get_corr(mimo_rx *h, uint32_t *corr, uint32_t *s0) {
  if (!h) return fail(MIMO_ERR_ARG, "null handle");
  if (!h->have_est) {
    if (corr) std::memset(corr, 0, sizeof(uint32_t) * h->N * (h->n_slots - 1));
    if (s0) std::memset(s0, 0, sizeof(uint32_t) * h->N);
    return MIMO_OK;
  }
  return copy_corr(h, 1, corr, s0);
}

int mimo_rx_get_stream_capacity(const mimo_rx *h, uint64_t *samples, uint64_t *held) {
  if (!h) return fail(MIMO_ERR_ARG, "null handle");
  if (samples) *samples = h->capbuf.p ? h->cap_len : 0;
  if (held) *held = h->total;
  return MIMO_OK;
}

int mimo_rx_get_decode_path(const mimo_rx *h, int32_t *path) {
  if (!h || !path) return fail(MIMO_ERR_ARG, "null argument");
  *path = h->last_decode_path;
  return MIMO_OK;
}

int mimo_rx_get_cfo_mode(const mimo_rx *h, int32_t *mode) {
  if (!h || !mode) return fail(MIMO_ERR_ARG, "null argument");
  *mode = h->last_cfo_mode;
  return MIMO_OK;
}

int mimo_rx_get_sc_exact_count(mimo_rx *h, uint64_t *out) {
  if (!h || !out) return fail(MIMO_ERR_ARG, "null argument");
  *out = 0;
  if (!h->ws.n_exact.p) return MIMO_OK;
  unsigned long long v = 0;
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(&v, h->ws.n_exact.p, sizeof(v), hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(h->ws.n_exact.p, 0, sizeof(v)));
  *out = v;
  return MIMO_OK;
}

// ---------------- host, device and memcpy helpers ----------------
float mimo_invert2(float *W, const float *G) {   // framing.cc:1344-1367 on host data
  const float2 *g = reinterpret_cast<const float2 *>(G);
  float2 *w = reinterpret_cast<float2 *>(W);
  auto mul = [](float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
  };
  const float2 p0 = mul(g[0], g[3]), p1 = mul(g[1], g[2]);
  const float2 det = make_float2(p0.x - p1.x, p0.y - p1.y);
  const float2 di = make_float2(det.x, -det.y), ndi = make_float2(-det.x, det.y);
  w[0] = mul(di, g[3]);
  w[3] = mul(di, g[0]);
  w[2] = mul(ndi, g[2]);
  w[1] = mul(ndi, g[1]);
  return 1.0f / (det.x * det.x + det.y * det.y);
}

int mimo_dev_alloc(void **ptr, size_t bytes) {
  if (!ptr) return fail(MIMO_ERR_ARG, "null argument");
  HIPCHK(hipMalloc(ptr, bytes));
  return MIMO_OK;
}
int mimo_dev_free(void *ptr) {
  HIPCHK(hipFree(ptr));
  return MIMO_OK;
}
int mimo_memcpy_h2d(void *dst, const void *src, size_t bytes, void *s) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)s));
  HIPCHK(hipStreamSynchronize((hipStream_t)s));
  return MIMO_OK;
}
int mimo_memcpy_d2h(void *dst, const void *src, size_t bytes, void *s) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)s));
  HIPCHK(hipStreamSynchronize((hipStream_t)s));
  return MIMO_OK;
}
int mimo_memcpy_d2d(void *dst, const void *src, size_t bytes, void *s) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)s));
  HIPCHK(hipStreamSynchronize((hipStream_t)s));
  return MIMO_OK;
}
int mimo_memset_d(void *dst, int value, size_t bytes, void *s) {
  HIPCHK(hipMemsetAsync(dst, value, bytes, (hipStream_t)s));
  return MIMO_OK;
}
int mimo_ingest_sc16(const void *src, uint64_t src_stride, void *dst, uint64_t dst_stride,
                     uint32_t n_arrays, uint64_t n, float scale, void *s) {
  if (n == 0 || n_arrays == 0) return MIMO_OK;
  if (!src || !dst) return fail(MIMO_ERR_ARG, "mimo_ingest_sc16: null buffer");
  if (n_arrays > 1 && (src_stride < n || dst_stride < n))
    return fail(MIMO_ERR_ARG, "mimo_ingest_sc16: stride shorter than a row");
  if (!launch_sc16_to_fc32(src, src_stride, dst, dst_stride, n_arrays, n, scale,
                           (hipStream_t)s))
    return fail(MIMO_ERR_ARG, "mimo_ingest_sc16: too many rows or samples for one launch");
  HIPCHK(hipGetLastError());
  return MIMO_OK;
}
int mimo_cfo_estimate(const void *x, uint64_t stride, uint32_t n_ant, uint64_t start,
                      uint32_t M, double *eps, void *s) {
  if (!x || !eps || n_ant == 0) return fail(MIMO_ERR_ARG, "mimo_cfo_estimate: null argument");
  if (M < 2 || (M & 1)) return fail(MIMO_ERR_ARG, "mimo_cfo_estimate: M must be even");
  if (n_ant > 1 && stride < start + M)
    return fail(MIMO_ERR_ARG, "mimo_cfo_estimate: window runs past the row stride");
  double *d = nullptr;
  HIPCHK(hipMalloc(&d, sizeof(double) * 2 * n_ant));
  std::vector<double> h(2 * n_ant);
  const hipStream_t st = (hipStream_t)s;
  bool ok = launch_cfo_corr(x, stride, n_ant, start, M / 2, d, st);
  hipError_t e = ok ? hipGetLastError() : hipSuccess;
  if (ok && e == hipSuccess) e = hipMemcpyAsync(h.data(), d, sizeof(double) * 2 * n_ant,
                                                hipMemcpyDeviceToHost, st);
  if (ok && e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(d);
  if (!ok) return fail(MIMO_ERR_ARG, "mimo_cfo_estimate: too many antenna rows");
  if (e != hipSuccess) return fail(MIMO_ERR_HIP, std::string("mimo_cfo_estimate: ") +
                                                     hipGetErrorString(e));
  double re = 0.0, im = 0.0;
  for (uint32_t r = 0; r < n_ant; ++r) {
    eps[r] = std::atan2(h[2 * r + 1], h[2 * r]) / M_PI;
    re += h[2 * r];
    im += h[2 * r + 1];
  }
  eps[n_ant] = std::atan2(im, re) / M_PI;
  return MIMO_OK;
}
int mimo_cfo_derotate(void *x, uint64_t stride, uint32_t n_ant, uint64_t n, int64_t n0,
                      double eps, uint32_t M, void *s) {
  if (n == 0 || n_ant == 0) return MIMO_OK;
  if (!x || M == 0) return fail(MIMO_ERR_ARG, "mimo_cfo_derotate: null buffer or M");
  if (n_ant > 1 && stride < n) return fail(MIMO_ERR_ARG, "mimo_cfo_derotate: stride < n");
  if (!launch_cfo_derotate(x, stride, n_ant, n, n0, eps / M, (hipStream_t)s))
    return fail(MIMO_ERR_ARG, "mimo_cfo_derotate: too many rows or samples for one launch");
  HIPCHK(hipGetLastError());
  return MIMO_OK;
}
int mimo_stream_sync(void *s) {
  HIPCHK(hipStreamSynchronize((hipStream_t)s));
  return MIMO_OK;
}
int mimo_device_count(int *n) {
  if (!n) return fail(MIMO_ERR_ARG, "null argument");
  HIPCHK(hipGetDeviceCount(n));
  return MIMO_OK;
}

}  // extern "C"
