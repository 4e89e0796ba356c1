// rub_mimo_amd/csrc/engine_sic.cpp -- ordered MMSE-SIC detection over the last batch
// (sic_kernels.hip): mimo_rx_sic_detect, mimo_rx_sic_soft (the same pass with per-bit LLRs),
// mimo_rx_sic_soft_fb (that pass cancelling expected symbols) and the getters of the detection
// order and post-SIC MSE. Opt-in passes like the soft output: the
// batch itself launches nothing for them.
#include "engine_internal.hpp"

// MIMO_OK when the handle's detector delivers y = (Q + lambda I)^-1 G^H X
int mimo::sic_supported(const mimo_rx *h) {
  if (h->det == MIMO_DET_SISO)
    return fail(MIMO_ERR_UNSUPPORTED, "SIC detection with the SISO detector");
  if (h->det == MIMO_DET_ZF2 && h->N != 2)
    return fail(MIMO_ERR_UNSUPPORTED, "SIC detection with MIMO_DET_ZF2 at N != 2 (identity weights)");
  return MIMO_OK;
}

// the order, tables and post-SIC MSE of the last batch's F frame slots, on stream s
static int launch_batch_sic_tables(mimo_rx *h, uint32_t F, hipStream_t s) {
  const size_t fm = (size_t)F * h->M_occ;
  if (h->sic_T.ensure(fm * h->N * h->N) != hipSuccess ||
      h->sic_C.ensure(fm * sic_c_rows(h->N)) != hipSuccess ||
      h->sic_order.ensure(fm * h->N) != hipSuccess || h->sic_nu.ensure(fm * h->N) != hipSuccess ||
      h->sic_ok.ensure(fm) != hipSuccess)
    return fail(MIMO_ERR_NOMEM, "SIC tables");
  SicTableArgs t{};
  t.N = h->N; t.M = h->M; t.M_occ = h->M_occ; t.detector = h->det;
  t.occ_index = h->occ.p; t.G = h->ws.G.p; t.info = h->ws.info.p;
  t.T = h->sic_T.p; t.C = h->sic_C.p; t.order = h->sic_order.p; t.nu = h->sic_nu.p;
  t.ok = h->sic_ok.p;
  if (!launch_sic_tables(t, F, s))
    return fail(MIMO_ERR_UNSUPPORTED, "no SIC table kernel for this stream or frame count");
  HIPCHK(hipGetLastError());
  return MIMO_OK;
}

// what mimo_rx_sic_detect, mimo_rx_sic_soft and mimo_rx_pic_soft ask of the handle and of the
// arguments they share (the callers have checked their pointers for null and alignment): a batch has run, its
// detector is supported, the shape is that batch's and z does not land on d_sym
int mimo::sic_pass_check(const mimo_rx *h, const void *d_sym, const void *d_out_sym,
                          uint32_t n_frames, uint32_t max_out_syms, uint32_t out_layout) {
  if (out_layout != MIMO_LAYOUT_STREAM_MAJOR && out_layout != MIMO_LAYOUT_SYMBOL_MAJOR)
    return fail(MIMO_ERR_ARG, "out_layout must be MIMO_LAYOUT_STREAM_MAJOR or _SYMBOL_MAJOR");
  if (h->last_frames == 0) return fail(MIMO_ERR_STATE, "no batch has run on this handle");
  int rc = sic_supported(h);
  if (rc) return rc;
  if (n_frames != h->last_frames || max_out_syms != h->last_max_out ||
      out_layout != h->last_layout)
    return fail(MIMO_ERR_ARG, "n_frames, max_out_syms and out_layout must be the last batch's");
  const uint64_t total = (uint64_t)n_frames * h->N * max_out_syms * h->M_occ;
  if (d_out_sym) {
    const uintptr_t x = (uintptr_t)d_sym, y = (uintptr_t)d_out_sym;
    if (x < y + total * sizeof(float2) && y < x + total * sizeof(float2))
      return fail(MIMO_ERR_ARG, "d_out_sym overlaps d_sym");
  }
  return MIMO_OK;
}

// every pass after its own argument checks: the shared checks, the tables, the symbol pass.
// A null a->d_llr is the hard output (format and llr_scale are not looked at then); feedback
// is the soft output with expected-symbol cancellation.
static int sic_pass(mimo_rx *h, const mimo_sic_soft *a, bool feedback, void *hip_stream) {
  int rc = sic_pass_check(h, a->d_sym, a->d_out_sym, a->n_frames, a->max_out_syms, a->out_layout);
  if (rc) return rc;
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
  rc = launch_batch_sic_tables(h, a->n_frames, s);
  if (rc) return rc;
  SicPassArgs k{};
  k.sym = reinterpret_cast<const float2 *>(a->d_sym);
  k.out_sym = reinterpret_cast<float2 *>(a->d_out_sym);
  k.out_idx = reinterpret_cast<uint8_t *>(a->d_out_idx);
  k.N = h->N; k.M_occ = h->M_occ; k.max_out = a->max_out_syms;
  k.symbol_major = a->out_layout == MIMO_LAYOUT_SYMBOL_MAJOR;
  k.qam = h->qam;
  k.info = h->ws.info.p;
  k.T = h->sic_T.p; k.C = h->sic_C.p; k.order = h->sic_order.p;
  if (a->d_llr) {
    k.llr = a->d_llr;
    k.nu = h->sic_nu.p;
    k.ok = h->sic_ok.p;
    k.llr_scale = a->llr_scale;
    k.f32 = a->format == MIMO_LLR_F32;
    k.bits = h->qam.b;
    k.feedback = feedback ? 1 : 0;
  }
  if (!launch_sic_pass(k, a->n_frames, s))
    return fail(MIMO_ERR_UNSUPPORTED,
                a->d_llr ? "no soft SIC kernel for this stream count, QAM order or batch shape"
                         : "no SIC kernel for this stream count or batch shape");
  HIPCHK(hipGetLastError());
  return MIMO_OK;
}

extern "C" {

int mimo_rx_sic_detect(mimo_rx *h, const mimo_sic_detect *a, void *hip_stream) {
  if (!h || !a || !a->d_sym) return fail(MIMO_ERR_ARG, "null argument");
  if (!a->d_out_sym && !a->d_out_idx)
    return fail(MIMO_ERR_ARG, "d_out_sym and d_out_idx are both null");
  if (((uintptr_t)a->d_sym & 15u) || ((uintptr_t)a->d_out_sym & 15u) ||
      ((uintptr_t)a->d_out_idx & 15u))
    return fail(MIMO_ERR_ARG, "d_sym, d_out_sym and d_out_idx must be 16-byte aligned");
  mimo_sic_soft q{};     // d_llr null: hard output
  q.d_sym = a->d_sym; q.d_out_sym = a->d_out_sym; q.d_out_idx = a->d_out_idx;
  q.n_frames = a->n_frames; q.max_out_syms = a->max_out_syms; q.out_layout = a->out_layout;
  return sic_pass(h, &q, false, hip_stream);
}

// the argument checks mimo_rx_sic_soft and mimo_rx_sic_soft_fb share
static int sic_soft_args(const mimo_rx *h, const mimo_sic_soft *a) {
  if (!h || !a || !a->d_sym || !a->d_llr) return fail(MIMO_ERR_ARG, "null argument");
  if (((uintptr_t)a->d_sym & 15u) || ((uintptr_t)a->d_llr & 15u) ||
      ((uintptr_t)a->d_out_sym & 15u) || ((uintptr_t)a->d_out_idx & 15u))
    return fail(MIMO_ERR_ARG, "d_sym, d_llr, d_out_sym and d_out_idx must be 16-byte aligned");
  if (!std::isfinite(a->llr_scale) || !(a->llr_scale > 0.0f))
    return fail(MIMO_ERR_ARG, "llr_scale must be finite and positive");
  if (a->format != MIMO_LLR_I8 && a->format != MIMO_LLR_F32)
    return fail(MIMO_ERR_ARG, "mimo_sic_soft.format must be MIMO_LLR_I8 or _F32");
  return MIMO_OK;
}

int mimo_rx_sic_soft(mimo_rx *h, const mimo_sic_soft *a, void *hip_stream) {
  const int rc = sic_soft_args(h, a);
  return rc ? rc : sic_pass(h, a, false, hip_stream);
}

int mimo_rx_sic_soft_fb(mimo_rx *h, const mimo_sic_soft *a, void *hip_stream) {
  const int rc = sic_soft_args(h, a);
  return rc ? rc : sic_pass(h, a, true, hip_stream);
}

// the getters' common part: the tables of every slot of the last batch, finished
static int sic_tables_now(mimo_rx *h, const void *out, uint32_t F) {
  if (!h || !out) return fail(MIMO_ERR_ARG, "null argument");
  if (h->last_frames == 0) return fail(MIMO_ERR_STATE, "no batch has run on this handle");
  int rc = sic_supported(h);
  if (rc) return rc;
  if (F > h->last_frames) return fail(MIMO_ERR_ARG, "more frames than the last batch");
  HIPCHK(hipDeviceSynchronize());
  rc = launch_batch_sic_tables(h, h->last_frames, h->stream);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  return MIMO_OK;
}

int mimo_rx_sic_order(mimo_rx *h, uint8_t *order, uint32_t F) {
  int rc = sic_tables_now(h, order, F);
  if (rc || F == 0) return rc;
  HIPCHK(hipMemcpy(order, h->sic_order.p, (size_t)F * h->M_occ * h->N, hipMemcpyDeviceToHost));
  return MIMO_OK;
}

int mimo_rx_sic_mse(mimo_rx *h, float *mse, uint32_t F) {
  int rc = sic_tables_now(h, mse, F);
  if (rc || F == 0) return rc;
  HIPCHK(hipMemcpy(mse, h->sic_nu.p, sizeof(float) * (size_t)F * h->N * h->M_occ,
                   hipMemcpyDeviceToHost));
  return MIMO_OK;
}

}  // extern "C"
