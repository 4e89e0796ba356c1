// rub_mimo_amd/csrc/engine_lord.cpp -- layered tree-search soft detection over the last batch
// (lord_kernels.hip): mimo_rx_lord_soft. An opt-in pass like the SIC and PIC passes, whose
// handle and shape checks it shares (engine_sic.cpp): the batch itself launches nothing for it.
#include "engine_internal.hpp"

// Q, the factors, the permutations and the carrier flags of the last batch's F frame slots, on
// stream s
static int launch_batch_lord_tables(mimo_rx *h, uint32_t F, hipStream_t s) {
  const size_t fm = (size_t)F * h->M_occ;
  if (h->lord_Q.ensure(fm * pic_q_rows(h->N)) != hipSuccess ||
      h->lord_U.ensure(fm * h->N * lord_u_rows(h->N)) != hipSuccess ||
      h->lord_perm.ensure(fm * h->N) != hipSuccess || h->lord_ok.ensure(fm) != hipSuccess)
    return fail(MIMO_ERR_NOMEM, "LORD tables");
  LordTableArgs t{};
  t.N = h->N; t.M = h->M; t.M_occ = h->M_occ;
  t.occ_index = h->occ.p; t.G = h->ws.G.p; t.info = h->ws.info.p;
  t.Q = h->lord_Q.p; t.U = h->lord_U.p; t.perm = h->lord_perm.p; t.ok = h->lord_ok.p;
  if (!launch_lord_tables(t, F, s))
    return fail(MIMO_ERR_UNSUPPORTED,
                "mimo_rx_lord_soft: no LORD table kernel for this stream or frame count");
  HIPCHK(hipGetLastError());
  return MIMO_OK;
}

extern "C" int mimo_rx_lord_soft(mimo_rx *h, const mimo_lord_soft *a, void *hip_stream) {
  if (!h || !a || !a->d_sym || !a->d_llr) return fail(MIMO_ERR_ARG, "null argument");
  if (((uintptr_t)a->d_sym & 15u) || ((uintptr_t)a->d_llr & 15u) ||
      ((uintptr_t)a->d_out_idx & 15u))
    return fail(MIMO_ERR_ARG, "d_sym, d_llr and d_out_idx must be 16-byte aligned");
  if (!std::isfinite(a->llr_scale) || !(a->llr_scale > 0.0f))
    return fail(MIMO_ERR_ARG, "llr_scale must be finite and positive");
  if (a->format != MIMO_LLR_I8 && a->format != MIMO_LLR_F32)
    return fail(MIMO_ERR_ARG, "mimo_lord_soft.format must be MIMO_LLR_I8 or _F32");
  int rc = sic_pass_check(h, a->d_sym, nullptr, a->n_frames, a->max_out_syms, a->out_layout);
  if (rc == MIMO_ERR_UNSUPPORTED)
    return fail(MIMO_ERR_UNSUPPORTED,
                "mimo_rx_lord_soft (LORD) with MIMO_DET_SISO, or MIMO_DET_ZF2 at N != 2");
  if (rc) return rc;
  if (h->N != 1 && h->N != 2 && h->N != 4)
    return fail(MIMO_ERR_UNSUPPORTED,
                "mimo_rx_lord_soft (LORD) has instances for 1, 2 and 4 streams");
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
  rc = launch_batch_lord_tables(h, a->n_frames, s);
  if (rc) return rc;
  LordPassArgs k{};
  k.sym = reinterpret_cast<const float2 *>(a->d_sym);
  k.out_idx = reinterpret_cast<uint8_t *>(a->d_out_idx);
  k.llr = a->d_llr;
  k.N = h->N; k.M_occ = h->M_occ; k.max_out = a->max_out_syms;
  k.symbol_major = a->out_layout == MIMO_LAYOUT_SYMBOL_MAJOR;
  k.mmse = h->det == MIMO_DET_MMSE;
  k.qam = h->qam;
  k.info = h->ws.info.p;
  k.Q = h->lord_Q.p; k.U = h->lord_U.p; k.perm = h->lord_perm.p; k.ok = h->lord_ok.p;
  k.llr_scale = a->llr_scale;
  k.f32 = a->format == MIMO_LLR_F32;
  k.bits = h->qam.b;
  if (!launch_lord_pass(k, a->n_frames, s))
    return fail(MIMO_ERR_UNSUPPORTED,
                "mimo_rx_lord_soft: no LORD kernel for this stream count, QAM order or batch shape");
  HIPCHK(hipGetLastError());
  return MIMO_OK;
}
