// rub_mimo_amd/csrc/engine_pic.cpp -- soft-input MMSE-PIC detection over the last batch
// (pic_kernels.hip): mimo_rx_pic_soft. An opt-in pass like the SIC passes, whose handle and
// shape checks it shares (engine_sic.cpp): the batch itself launches nothing for it.
#include "engine_internal.hpp"

// Q and the carrier flags of the last batch's F frame slots, on stream s
static int launch_batch_pic_tables(mimo_rx *h, uint32_t F, hipStream_t s) {
  const size_t fm = (size_t)F * h->M_occ;
  if (h->pic_Q.ensure(fm * pic_q_rows(h->N)) != hipSuccess || h->pic_ok.ensure(fm) != hipSuccess)
    return fail(MIMO_ERR_NOMEM, "PIC tables");
  PicTableArgs t{};
  t.N = h->N; t.M = h->M; t.M_occ = h->M_occ;
  t.occ_index = h->occ.p; t.G = h->ws.G.p; t.info = h->ws.info.p;
  t.Q = h->pic_Q.p; t.ok = h->pic_ok.p;
  if (!launch_pic_tables(t, F, s))
    return fail(MIMO_ERR_UNSUPPORTED, "no PIC table kernel for this stream or frame count");
  HIPCHK(hipGetLastError());
  return MIMO_OK;
}

extern "C" int mimo_rx_pic_soft(mimo_rx *h, const mimo_pic_soft *a, void *hip_stream) {
  if (!h || !a || !a->d_sym || !a->d_llr) return fail(MIMO_ERR_ARG, "null argument");
  if (((uintptr_t)a->d_sym & 15u) || ((uintptr_t)a->d_llr & 15u) ||
      ((uintptr_t)a->d_prior & 15u) || ((uintptr_t)a->d_out_sym & 15u) ||
      ((uintptr_t)a->d_out_idx & 15u))
    return fail(MIMO_ERR_ARG,
                "d_sym, d_prior, d_llr, d_out_sym and d_out_idx must be 16-byte aligned");
  if (!std::isfinite(a->llr_scale) || !(a->llr_scale > 0.0f))
    return fail(MIMO_ERR_ARG, "llr_scale must be finite and positive");
  if (!std::isfinite(a->prior_scale) || !(a->prior_scale > 0.0f))
    return fail(MIMO_ERR_ARG, "prior_scale must be finite and positive");
  if (a->format != MIMO_LLR_I8 && a->format != MIMO_LLR_F32)
    return fail(MIMO_ERR_ARG, "mimo_pic_soft.format must be MIMO_LLR_I8 or _F32");
  int rc = sic_pass_check(h, a->d_sym, a->d_out_sym, a->n_frames, a->max_out_syms, a->out_layout);
  if (rc) return rc;
  if (h->N != 1 && h->N != 2 && h->N != 4)
    return fail(MIMO_ERR_UNSUPPORTED, "MMSE-PIC detection has instances for 1, 2 and 4 streams");
  if (a->d_prior) {
    const uint64_t vals = (uint64_t)a->n_frames * h->N * a->max_out_syms * h->M_occ * 2 * h->qam.b;
    const uintptr_t x = (uintptr_t)a->d_prior, y = (uintptr_t)a->d_llr;
    if (x < y + vals * (a->format == MIMO_LLR_F32 ? sizeof(float) : 1) && y < x + vals)
      return fail(MIMO_ERR_ARG, "d_prior overlaps d_llr");
  }
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
  rc = launch_batch_pic_tables(h, a->n_frames, s);
  if (rc) return rc;
  PicPassArgs k{};
  k.sym = reinterpret_cast<const float2 *>(a->d_sym);
  k.prior = reinterpret_cast<const int8_t *>(a->d_prior);
  k.out_sym = reinterpret_cast<float2 *>(a->d_out_sym);
  k.out_idx = reinterpret_cast<uint8_t *>(a->d_out_idx);
  k.llr = a->d_llr;
  k.N = h->N; k.M_occ = h->M_occ; k.max_out = a->max_out_syms;
  k.symbol_major = a->out_layout == MIMO_LAYOUT_SYMBOL_MAJOR;
  k.mmse = h->det == MIMO_DET_MMSE;
  k.qam = h->qam;
  k.info = h->ws.info.p;
  k.Q = h->pic_Q.p; k.ok = h->pic_ok.p;
  k.llr_scale = a->llr_scale; k.prior_scale = a->prior_scale;
  k.f32 = a->format == MIMO_LLR_F32;
  k.bits = h->qam.b;
  if (!launch_pic_pass(k, a->n_frames, s))
    return fail(MIMO_ERR_UNSUPPORTED,
                "no MMSE-PIC kernel for this stream count, QAM order or batch shape");
  HIPCHK(hipGetLastError());
  return MIMO_OK;
}
