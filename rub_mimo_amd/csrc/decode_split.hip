// rub_mimo_amd/csrc/decode_split.hip -- split decode for 8x8 on gfx950 (C4: one symbol is
// 8 x 4096 x 8 B = 256 KB, more than LDS, and its weights are 2 MB per frame, so neither a
// symbol nor a frame's W fits a workgroup and the streaming form of decode_stream.hip does not
// apply):
//   1. spectra_kernel: one workgroup per (frame, symbol, antenna) transforms the body in LDS
//      and writes X to a scratch laid out [frame][chunk of 64 subcarriers][symbol][antenna][64]
//      -- the apply of one chunk then reads 4 KB contiguous per symbol;
//   2. apply_split_kernel: one workgroup per (frame, chunk, symbol range) keeps W*gain*dn of
//      its 64 subcarriers in registers (wave h: outputs 2h and 2h+1, 32 VGPRs) and streams
//      the range's symbols through the 8x8 apply, demap, EVM and stores.
// Weights are read once per (chunk, range) instead of once per symbol (the per-symbol kernel
// reads 2 MB of W from L2 for every 256 KB symbol). The two kernels can alternate over groups
// of symbols (a.sym0 .. + a.sym_cap) through one scratch of that many symbols per frame, so
// that a group's spectra are read back while still in the 256 MB Infinity Cache
// (-DDS_SPLIT_GROUP, off by default: see split_group_symbols). EVM records: symbol group x
// chunk x range per frame (nrec), NA/2 per record.
#include <algorithm>

#include "fft.hpp"
#include "fft_reg.hpp"
#include "kernels.hpp"

namespace mimo {

constexpr uint32_t kSplitSets = 16;   // EVM partial sets per record (<= kMaxEvmParts)
// the split decode's spectra scratch: [F][sym_cap][N][M] complex64, each (symbol, antenna)
// spectrum one contiguous row: the spectra pass writes one sequential 8 M-byte run per item
// (chunked forms [F][M / CH][sym_cap][N][CH] measured slower the smaller CH: C4 decode 1.335 /
// 1.317 / 1.290 / 1.254 ms at CH = 64 / 512 / 1024 / M, profiles/r05/ab/r05_specch.txt)
// float2 offset of subcarrier k of antenna r, scratch slot sl, frame f
MIMO_DEV uint64_t spec_off(const DecodeArgs &a, uint32_t f, uint32_t sl, uint32_t r, uint32_t k) {
  return (((uint64_t)f * a.sym_cap + sl) * a.N + r) * a.M + k;
}

// hard decision as qam_slice (decode_kernels.hip) / qam_demap (common.hpp): the level is
// floor((y * inv_scale + L) * 0.5) clamped to [0, L-1] (NaN -> 0); truncation of the
// non-negative value by v_cvt_u32_f32 with its saturation gives exactly that clamp
MIMO_DEV uint32_t qam_slice_pk(v2f y, v2f inv_scale, v2f Lf, uint32_t Lm1, uint32_t b) {
#pragma clang fp contract(off)
  const v2f t = (y * inv_scale + Lf) * 0.5f;
  const uint32_t mI = min(cvt_u32_sat(t.x), Lm1), mQ = min(cvt_u32_sat(t.y), Lm1);
  return (gray_enc(mI) << b) | gray_enc(mQ);
}

template <int LOG2M, int T, bool SC16>
__global__ __launch_bounds__(T) void spectra_kernel(DecodeArgs a) {
  constexpr int M = 1 << LOG2M;
  extern __shared__ __attribute__((aligned(16))) float2 lds_sp[];
  const uint32_t f = blockIdx.y, sl = blockIdx.x, r = blockIdx.z;
  const uint32_t s = a.sym0 + sl;                     // symbol; sl its scratch slot
  const FrameInfo &I = a.info[f];
  const uint32_t n_out = (I.status == 0) ? min(I.n_sym, a.max_out) : 0u;
  if (s >= n_out) return;                             // uniform
  const int64_t abs0 = I.base + (int64_t)I.i0 + (int64_t)s * a.SL + a.cp;
  const int64_t L = (int64_t)a.frame_len;
  const auto xs = iq_row<SC16>(a.iq, a.iq_scale, ((uint64_t)I.cap * a.N + r) * a.stride);
  const int tid = threadIdx.x;
  if (abs0 >= 0 && abs0 + M <= L && xs.pair_ok() && (abs0 & 1) == 0) {
#pragma unroll
    for (int i = tid; i < M / 2; i += T) {
      const float4 v = xs.pair(abs0 + 2 * i);
      lds_sp[lds_pad(2 * i)] = make_float2(v.x, v.y);
      lds_sp[lds_pad(2 * i + 1)] = make_float2(v.z, v.w);
    }
  } else {
    for (int i = tid; i < M; i += T) {
      const int64_t n = abs0 + i;
      lds_sp[lds_pad(i)] = (n >= 0 && n < L) ? xs.at(n) : make_float2(0.0f, 0.0f);
    }
  }
  __syncthreads();
  fft_lds<LOG2M, T, 1, false>(lds_sp, a.tw);
  float2 *o = a.spec + spec_off(a, f, sl, r, 0);
#pragma unroll
  for (int k = tid; k < M; k += T) o[k] = lds_sp[lds_pad(k)];
}

// Persistent form of spectra_kernel for M = 2^LOG2M >= 2048 (C4: M = 4096): each workgroup
// walks (frame, symbol, antenna) items with a stride of the grid, the next item's body loaded
// straight into registers (PTS = 16 per thread, in the order the first radix-16 pass reads)
// while the current one is transformed (register-resident radix-16 Stockham FFT, two LDS
// exchanges, base twiddles held per thread) and stored from registers (each wave store
// instruction writes 512 contiguous bytes of one 64-subcarrier chunk). The one-item-per-
// workgroup kernel waited on its load, four global twiddle reads and its stores in turn.
template <int LOG2M, bool SC16>
__global__ __launch_bounds__((1 << LOG2M) / 16) void spectra_persist_kernel(DecodeArgs a) {
  using PL = RegPlan<LOG2M, 16>;
  constexpr int M = 1 << LOG2M, T = PL::T;
  static_assert(T % 64 == 0, "whole waves");
  extern __shared__ __attribute__((aligned(16))) float2 lds_sp[];
  v2f *buf = reinterpret_cast<v2f *>(lds_sp);
  const int tid = threadIdx.x;
  v2f w1[PL::NTW > 0 ? PL::NTW : 1];
  reg_twiddles<LOG2M, 16>(w1, a.tw, tid);
  const uint32_t NI = a.N;
  const uint64_t per_frame = (uint64_t)a.sym_cap * NI;
  const uint64_t total = per_frame * a.n_frames;
  const int64_t L = (int64_t)a.frame_len;
  // item -> (frame, scratch slot, antenna); false when its symbol is not decoded
  auto item = [&](uint64_t it, uint32_t &f, uint32_t &sl, uint32_t &r, int64_t &abs0,
                  uint32_t &cap) -> bool {
    f = (uint32_t)(it / per_frame);
    const uint32_t rem = (uint32_t)(it % per_frame);
    sl = rem / NI;
    r = rem % NI;
    const FrameInfo &I = a.info[f];
    const uint32_t n_out = (I.status == 0) ? min(I.n_sym, a.max_out) : 0u;
    abs0 = I.base + (int64_t)I.i0 + (int64_t)(a.sym0 + sl) * a.SL + a.cp;
    cap = I.cap;
    return a.sym0 + sl < n_out;
  };
  auto load = [&](v2f (&x)[16], uint32_t cap, uint32_t r, int64_t abs0) {
    const auto xs = iq_row<SC16>(a.iq, a.iq_scale, ((uint64_t)cap * a.N + r) * a.stride);
    if (abs0 >= 0 && abs0 + M <= L) {
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const float2 t = xs.at(abs0 + reg_index<LOG2M, 16>(tid, e));
        x[e] = v2f{t.x, t.y};
      }
    } else {   // the capture's edge: zero outside it
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int64_t n = abs0 + reg_index<LOG2M, 16>(tid, e);
        const float2 t = xs.at(n < 0 ? 0 : (n >= L ? L - 1 : n));
        x[e] = (n >= 0 && n < L) ? v2f{t.x, t.y} : v2f{0.0f, 0.0f};
      }
    }
  };
  uint64_t it = blockIdx.x;
  uint32_t f = 0, sl = 0, r = 0, cap = 0;
  int64_t abs0 = 0;
  // the first live item of this workgroup
  while (it < total && !item(it, f, sl, r, abs0, cap)) it += gridDim.x;
  if (it >= total) return;                            // uniform
  v2f v[16], nx[16];
  load(v, cap, r, abs0);
  for (;;) {
    // the next live item's body, in flight during this transform
    uint64_t nit = it + gridDim.x;
    uint32_t nf = 0, nsl = 0, nr = 0, ncap = 0;
    int64_t nabs0 = 0;
    while (nit < total && !item(nit, nf, nsl, nr, nabs0, ncap)) nit += gridDim.x;
    if (nit < total) load(nx, ncap, nr, nabs0);
    reg_compute<LOG2M, 16, 0, false>(v, w1);
    reg_rest<LOG2M, 16, 1, false>(buf, v, w1, tid);
    // X[k], k = tid + T e, into the whole row [F][sym_cap][N][M] (spec_off)
    float2 *o = a.spec + spec_off(a, f, sl, r, 0);
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const uint32_t k = (uint32_t)reg_index<LOG2M, 16>(tid, e);
      o[k] = make_float2(v[e].x, v[e].y);
    }
    if (nit >= total) break;                          // uniform
    it = nit; f = nf; sl = nsl; r = nr;
#pragma unroll
    for (int e = 0; e < 16; e++) v[e] = nx[e];
    // (reg_rest opens with a barrier: this transform's LDS readers finish before the next store)
  }
}

template <int NA, int REF>
__global__ __launch_bounds__(32 * NA) void apply_split_kernel(DecodeArgs a) {
  constexpr int T = 32 * NA;                          // NA/2 waves
  constexpr int PF = 4;                               // symbols in flight per workgroup
  static_assert(NA == 8, "one 16-byte load per thread covers a symbol's 8 x 64 spectra");
  const uint32_t c = blockIdx.x, f = blockIdx.y, part = blockIdx.z;
  const uint32_t NCH = gridDim.x, P = gridDim.z;
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t h = __builtin_amdgcn_readfirstlane((uint32_t)tid >> 6);
  __shared__ v2f ptab[kStreamMaxQam];
  __shared__ __attribute__((aligned(16))) v2f xs[2][NA * 64];    // spectra of one symbol
  __shared__ __attribute__((aligned(16))) uint8_t rs[2][NA * 64];  // its reference indices
  for (uint32_t e = tid; e < a.qam.L * a.qam.L; e += T) {
    const float2 p = qam_point(e, a.qam);
    ptab[e] = v2f{p.x, p.y};
  }
  const FrameInfo &I = a.info[f];
  const uint32_t n_out = (I.status == 0) ? min(I.n_sym, a.max_out) : 0u;
  const uint32_t grp = a.sym0 / a.sym_cap;            // this launch's symbol group
  if (grp == 0 && c == 0 && part == 0 && tid == 0)
    a.nrec[f] = a.sym_groups * NCH * P * (T / 64) / kSplitSets;
  // the group's symbols of this frame, split in P ranges
  const uint32_t ng = n_out > a.sym0 ? min(n_out - a.sym0, a.sym_cap) : 0u;
  const uint32_t s0 = a.sym0 + (uint32_t)((uint64_t)ng * part / P);
  const uint32_t s1 = a.sym0 + (uint32_t)((uint64_t)ng * (part + 1) / P);
  const uint32_t M = a.M, k = c * 64 + lane;
  v2f Wr[2][NA];
  {
    const float gk = a.gain[(uint64_t)f * M + k] * a.dn;
#pragma unroll
    for (int tt = 0; tt < 2; tt++)
#pragma unroll
      for (int r = 0; r < NA; r++) {
        const float2 w = a.W[(((uint64_t)f * NA + 2 * h + tt) * NA + r) * M + k];
        Wr[tt][r] = v2f{w.x * gk, w.y * gk};
      }
  }
  const v2f inv_sc = v2f{a.qam.inv_scale, a.qam.inv_scale};
  const v2f Lf = v2f{(float)a.qam.L, (float)a.qam.L};
  const uint32_t Lm1 = a.qam.L - 1;
  const uint64_t frame_id = a.frame_id0 + I.ref;
  // symbol s of this chunk: 4 KB at spec4 + (s - sym0) * 256 (16 B per thread), reference
  // indices of stream t at ref + t o_ts + s o_ss (16 B per thread for tid < 32)
  // (thread tid: antenna tid / 32, subcarriers c 64 + 2 (tid % 32) + 0, 1; symbols N M apart)
  const float4 *spec4 = reinterpret_cast<const float4 *>(
      a.spec + spec_off(a, f, 0, (uint32_t)tid >> 5, c * 64 + 2 * ((uint32_t)tid & 31u)));
  const uint8_t *refb = (REF == 1) ? a.ref_idx + (uint64_t)I.ref * NA * a.max_out * a.M_occ +
                                         (uint64_t)(tid >> 2) * a.o_ts + c * 64 + (tid & 3) * 16
                                   : nullptr;
  // symbols in flight: slot u holds symbol sb + u; loads are unconditional (past the range
  // they re-read the last symbol) so the slots stay in registers with counted waits
  const uint32_t slast = s1 > s0 ? s1 - 1 : s0;
  float4 pf0, pf1, pf2, pf3;                           // symbol slots (named: no scratch)
  uint4 pr0, pr1, pr2, pr3;
  auto load_sym = [&](float4 &x, uint4 &r, uint32_t s) {
    const uint32_t sc = min(s, slast);
    x = spec4[(uint64_t)(sc - a.sym0) * (NA * a.M / 2)];
    if constexpr (REF == 1)
      if (tid < 32) r = *reinterpret_cast<const uint4 *>(refb + (uint64_t)sc * a.o_ss);
  };
  if (s0 < s1) {
    load_sym(pf0, pr0, s0);
    load_sym(pf1, pr1, s0 + 1);
    load_sym(pf2, pr2, s0 + 2);
    load_sym(pf3, pr3, s0 + 3);
  }
  float e_num[2] = {0.0f, 0.0f}, e_den[2] = {0.0f, 0.0f};
  uint32_t n_err[2] = {0u, 0u};
  // one symbol: slot -> LDS, refill the slot PF symbols ahead, barrier, apply + demap + EVM
  auto one = [&](float4 &x, uint4 &r, uint32_t s, int b) {
    reinterpret_cast<float4 *>(xs[b])[tid] = x;
    if constexpr (REF == 1)
      if (tid < 32) reinterpret_cast<uint4 *>(rs[b])[tid] = r;
    load_sym(x, r, s + PF);
    __syncthreads();                                  // xs[b] complete; xs[b^1] readers done
    if (s >= s1) return;                              // uniform: the range's last block
    v2f X[NA];
#pragma unroll
    for (int q = 0; q < NA; q++) X[q] = xs[b][q * 64 + lane];
#pragma unroll
    for (int tt = 0; tt < 2; tt++) {
      const uint32_t t = 2 * h + tt;
      v2f acc = v2f{0.0f, 0.0f};
#pragma unroll
      for (int q = 0; q < NA; q++) acc = cmac_pk(acc, Wr[tt][q], X[q]);
      const uint32_t d = qam_slice_pk(acc, inv_sc, Lf, Lm1, a.qam.b);
      const uint64_t o = (uint64_t)f * NA * a.max_out * a.M_occ + t * a.o_ts + s * a.o_ss + k;
      uint32_t refi;
      if constexpr (REF == 1) refi = rs[b][t * 64 + lane];
      else if constexpr (REF == 2)
        refi = (uint32_t)(hash5(a.ref_seed, DOM_DATA, frame_id, t, (uint64_t)s * a.M_occ + k) &
                          (uint64_t)(a.qam.L * a.qam.L - 1));
      else refi = d;
      n_err[tt] += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(refi != d));
      const v2f pt = ptab[refi];
      const v2f er = acc - pt;
      e_num[tt] = __builtin_fmaf(er.x, er.x, __builtin_fmaf(er.y, er.y, e_num[tt]));
      e_den[tt] = __builtin_fmaf(pt.x, pt.x, __builtin_fmaf(pt.y, pt.y, e_den[tt]));
      if (a.out_sym) reinterpret_cast<v2f *>(a.out_sym)[o] = acc;
      if (a.out_idx) a.out_idx[o] = (uint8_t)d;
    }
  };
  for (uint32_t sb = s0; sb < s1; sb += PF) {
    one(pf0, pr0, sb, 0);
    one(pf1, pr1, sb + 1, 1);
    one(pf2, pr2, sb + 2, 0);
    one(pf3, pr3, sb + 3, 1);
  }
#pragma unroll
  for (int tt = 0; tt < 2; tt++)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      e_num[tt] += __shfl_xor(e_num[tt], off);
      e_den[tt] += __shfl_xor(e_den[tt], off);
    }
  // partial set ((grp * NCH + c) * P + part) * waves + h: this wave's two streams, zeros elsewhere
  const uint64_t set = (((uint64_t)grp * NCH + c) * P + part) * (T / 64) + h;
  double *ep = a.evm_part + ((uint64_t)f * a.rec_stride * kSplitSets + set) * NA * 3;
  if (lane < NA * 3) {
    const uint32_t t = lane / 3, comp = lane % 3;
    float v = 0.0f;
#pragma unroll
    for (int tt = 0; tt < 2; tt++)
      if (t == 2 * h + tt) v = comp == 0 ? e_num[tt] : (comp == 1 ? e_den[tt] : (float)n_err[tt]);
    ep[lane] = (double)v;
  }
}

// The same 8x8 apply over 128-subcarrier chunks: wave w owns output stream w and lane l the
// adjacent subcarriers 2l, 2l+1 of the chunk, so each lane stores 16 bytes of symbols and 2 of
// indices per symbol (a wave writes 1 KB of symbols and one whole 128-byte line of indices).
// The 64-subcarrier form (apply_split_kernel, RMIMO_APPLY_V1=1) wrote 64-byte index segments:
// 98 of its 767 us at C4 x 8 went to the index stores (a store-ablation build), for 11% of
// the bytes. EVM sets: (group, chunk, range, wave), NA per record as before.
template <int NA, int REF>
__global__ __launch_bounds__(64 * NA) void apply_split2_kernel(DecodeArgs a) {
  constexpr int T = 64 * NA;                          // NA waves: one output stream each
  constexpr int PF = 4;                               // symbols in flight per workgroup
  constexpr int CW = 128;                             // subcarriers per chunk
  static_assert(NA == 8, "one 16-byte load per thread covers a symbol's 8 x 128 spectra");
  const uint32_t c2 = blockIdx.x, f = blockIdx.y, part = blockIdx.z;
  const uint32_t NCH2 = gridDim.x, P = gridDim.z;
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t w = __builtin_amdgcn_readfirstlane((uint32_t)tid >> 6);
  __shared__ v2f ptab[kStreamMaxQam];
  __shared__ __attribute__((aligned(16))) v2f xs[2][NA * CW];     // [antenna][subcarrier]
  __shared__ __attribute__((aligned(16))) uint8_t rs[2][NA * CW];   // [stream][subcarrier]
  for (uint32_t e = tid; e < a.qam.L * a.qam.L; e += T) {
    const float2 p = qam_point(e, a.qam);
    ptab[e] = v2f{p.x, p.y};
  }
  const FrameInfo &I = a.info[f];
  const uint32_t n_out = (I.status == 0) ? min(I.n_sym, a.max_out) : 0u;
  const uint32_t grp = a.sym0 / a.sym_cap;            // this launch's symbol group
  if (grp == 0 && c2 == 0 && part == 0 && tid == 0)
    a.nrec[f] = a.sym_groups * NCH2 * P * (T / 64) / kSplitSets;
  const uint32_t ng = n_out > a.sym0 ? min(n_out - a.sym0, a.sym_cap) : 0u;
  const uint32_t s0 = a.sym0 + (uint32_t)((uint64_t)ng * part / P);
  const uint32_t s1 = a.sym0 + (uint32_t)((uint64_t)ng * (part + 1) / P);
  const uint32_t M = a.M, kb = c2 * CW + 2 * lane;    // this lane's subcarriers kb, kb + 1
  v2f Wr[2][NA];
  {
    const float2 g2 = *reinterpret_cast<const float2 *>(a.gain + (uint64_t)f * M + kb);
    const float gk0 = g2.x * a.dn, gk1 = g2.y * a.dn;
#pragma unroll
    for (int r = 0; r < NA; r++) {
      const float4 wv = *reinterpret_cast<const float4 *>(a.W + (((uint64_t)f * NA + w) * NA + r) * M + kb);
      Wr[0][r] = v2f{wv.x * gk0, wv.y * gk0};
      Wr[1][r] = v2f{wv.z * gk1, wv.w * gk1};
    }
  }
  const v2f inv_sc = v2f{a.qam.inv_scale, a.qam.inv_scale};
  const v2f Lf = v2f{(float)a.qam.L, (float)a.qam.L};
  const uint32_t Lm1 = a.qam.L - 1;
  const uint64_t frame_id = a.frame_id0 + I.ref;
  // thread t loads the float4 of antenna t / 64, subcarriers c2 CW + 2 (t % 64) + 0, 1 (symbols
  // N M apart in the scratch); threads < 64 load 16 bytes of reference indices (stream t / 8,
  // bytes 16 (t % 8) ..)
  const uint32_t ant = (uint32_t)tid >> 6, pr = (uint32_t)tid & 63u;
  const float4 *spec4 = reinterpret_cast<const float4 *>(a.spec + spec_off(a, f, 0, ant, c2 * CW + 2 * pr));
  v4f *xdst0 = reinterpret_cast<v4f *>(&xs[0][ant * CW + 2 * pr]);
  v4f *xdst1 = reinterpret_cast<v4f *>(&xs[1][ant * CW + 2 * pr]);
  const uint8_t *refb = (REF == 1) ? a.ref_idx + (uint64_t)I.ref * NA * a.max_out * a.M_occ +
                                         (uint64_t)(tid >> 3) * a.o_ts + c2 * CW + (tid & 7) * 16
                                   : nullptr;
  const uint32_t slast = s1 > s0 ? s1 - 1 : s0;
  float4 pf0, pf1, pf2, pf3;                          // symbol slots (named: no scratch)
  uint4 pr0, pr1, pr2, pr3;
  auto load_sym = [&](float4 &x, uint4 &r, uint32_t s) {
    const uint32_t sc = min(s, slast);
    x = spec4[(uint64_t)(sc - a.sym0) * (NA * a.M / 2)];
    if constexpr (REF == 1)
      if (tid < 64) r = *reinterpret_cast<const uint4 *>(refb + (uint64_t)sc * a.o_ss);
  };
  if (s0 < s1) {
    load_sym(pf0, pr0, s0);
    load_sym(pf1, pr1, s0 + 1);
    load_sym(pf2, pr2, s0 + 2);
    load_sym(pf3, pr3, s0 + 3);
  }
  float e_num = 0.0f, e_den = 0.0f;
  uint32_t n_err = 0u;
  auto one = [&](float4 &x, uint4 &r, uint32_t s, int b) {
    *(b ? xdst1 : xdst0) = v4f{x.x, x.y, x.z, x.w};
    if constexpr (REF == 1)
      if (tid < 64) reinterpret_cast<uint4 *>(rs[b])[tid] = r;
    load_sym(x, r, s + PF);
    __syncthreads();                                  // xs[b] complete; xs[b^1] readers done
    if (s >= s1) return;                              // uniform: the range's last block
    v2f acc[2] = {v2f{0.0f, 0.0f}, v2f{0.0f, 0.0f}};
#pragma unroll
    for (int q = 0; q < NA; q++) {
      const v4f xv = *reinterpret_cast<const v4f *>(&xs[b][q * CW + 2 * lane]);
      acc[0] = cmac_pk(acc[0], Wr[0][q], v2f{xv.x, xv.y});
      acc[1] = cmac_pk(acc[1], Wr[1][q], v2f{xv.z, xv.w});
    }
    uint32_t d[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
      d[j] = qam_slice_pk(acc[j], inv_sc, Lf, Lm1, a.qam.b);
      uint32_t refi;
      if constexpr (REF == 1) refi = rs[b][w * CW + 2 * lane + j];
      else if constexpr (REF == 2)
        refi = (uint32_t)(hash5(a.ref_seed, DOM_DATA, frame_id, w, (uint64_t)s * a.M_occ + kb + j) &
                          (uint64_t)(a.qam.L * a.qam.L - 1));
      else refi = d[j];
      n_err += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(refi != d[j]));
      const v2f pt = ptab[refi];
      const v2f er = acc[j] - pt;
      e_num = __builtin_fmaf(er.x, er.x, __builtin_fmaf(er.y, er.y, e_num));
      e_den = __builtin_fmaf(pt.x, pt.x, __builtin_fmaf(pt.y, pt.y, e_den));
    }
    const uint64_t o = (uint64_t)f * NA * a.max_out * a.M_occ + w * a.o_ts + s * a.o_ss + kb;
    // (plain stores: non-temporal ones measured +3.7% on this kernel at C4)
    if (a.out_sym)
      *reinterpret_cast<v4f *>(reinterpret_cast<v2f *>(a.out_sym) + o) =
          v4f{acc[0].x, acc[0].y, acc[1].x, acc[1].y};
    if (a.out_idx) *reinterpret_cast<uint16_t *>(a.out_idx + o) = (uint16_t)(d[0] | (d[1] << 8));
  };
  for (uint32_t sb = s0; sb < s1; sb += PF) {
    one(pf0, pr0, sb, 0);
    one(pf1, pr1, sb + 1, 1);
    one(pf2, pr2, sb + 2, 0);
    one(pf3, pr3, sb + 3, 1);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    e_num += __shfl_xor(e_num, off);
    e_den += __shfl_xor(e_den, off);
  }
  // partial set ((grp * NCH2 + c2) * P + part) * waves + w: this wave's stream, zeros elsewhere
  const uint64_t set = (((uint64_t)grp * NCH2 + c2) * P + part) * (T / 64) + w;
  double *ep = a.evm_part + ((uint64_t)f * a.rec_stride * kSplitSets + set) * NA * 3;
  if (lane < NA * 3) {
    const uint32_t t = lane / 3, comp = lane % 3;
    const float v = t != w ? 0.0f : (comp == 0 ? e_num : (comp == 1 ? e_den : (float)n_err));
    ep[lane] = (double)v;
  }
}

bool decode_split_accepts(const DecodeArgs &a, int log2M) {
  // (the apply reads 16 bytes of reference indices per lane)
  return a.N == 8 && a.detector != 3 && a.all_occ && log2M >= 9 && log2M <= 12 &&
         a.max_out >= (1u << log2M) / 64 && a.qam.L * a.qam.L <= kStreamMaxQam &&
         (a.ref_mode != 1 || ((uintptr_t)a.ref_idx & 15u) == 0);
}

// symbols per group: every symbol in one group (the spectra of the whole batch in the
// scratch). Infinity-Cache-sized groups (e.g. 32, compile with -DDS_SPLIT_GROUP=32) measured
// slower at C4 x 8 -- 2.10 vs 1.58 ms per decode -- because each group's apply re-reads its
// chunk's weights, 16x the weight traffic, and each launch is a quarter of the chip
uint32_t split_group_symbols(uint32_t max_out) {
#ifdef DS_SPLIT_GROUP
  const uint32_t g = DS_SPLIT_GROUP;
#else
  const uint32_t g = max_out;
#endif
  return std::max(1u, std::min(g, max_out));
}

// symbol groups, ranges per (group, chunk) and the EVM records per frame of the split decode:
// ranges of ~8 symbols (four in flight per workgroup) so that each apply launch has enough
// workgroups; records = groups * chunks * ranges * 4 waves / kSplitSets
uint32_t split_plan(uint32_t max_out, int log2M, uint32_t *groups_out, uint32_t *P_out) {
  const uint32_t NCH = (1u << log2M) / 64, cap = split_group_symbols(max_out);
  const uint32_t groups = (max_out + cap - 1) / cap;
  uint32_t P = std::max(1u, std::min(16u, cap / 8));
  while ((groups * NCH * P * 4) % kSplitSets) P++;    // whole records (NCH * 4 >= 32: P as is)
  if (groups_out) *groups_out = groups;
  if (P_out) *P_out = P;
  return groups * NCH * P * 4 / kSplitSets;
}

// workgroups of a kernel resident per CU at this block size and dynamic LDS (a persistent
// grid is that many times the CU count: no workgroup waits for another to finish)
static uint32_t resident_blocks(const void *k, int threads, size_t shm) {
  int n = 1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, threads, shm) != hipSuccess || n < 1) n = 1;
  return (uint32_t)n;
}

// 8x8 split decode; returns the partial sets per record (0: not handled)
uint32_t launch_decode_split(const DecodeArgs &a, int log2M, uint32_t n_frames, hipStream_t s) {
  if (!a.spec || !a.nrec || !decode_split_accepts(a, log2M)) return 0;
  const uint32_t NCH = a.M / 64;
  const uint32_t cap = split_group_symbols(a.max_out);
  uint32_t groups = 0, P = 0;
  if (split_plan(a.max_out, log2M, &groups, &P) > a.rec_stride) return 0;   // EVM space
  constexpr int T1 = 512;
  const size_t shm = sizeof(float2) * lds_padded_len(1 << log2M);
  DecodeArgs g = a;
  g.sym_cap = cap;
  g.sym_groups = groups;
  const dim3 g2(NCH, n_frames, P);
  for (uint32_t k = 0; k < groups; k++) {
    g.sym0 = k * cap;
    const dim3 g1(std::min(cap, a.max_out - g.sym0), n_frames, a.N);
#define SPECTRA(L2)                                                                      \
  do {                                                                                   \
    if (a.sc16) hipLaunchKernelGGL((spectra_kernel<L2, T1, true>), g1, dim3(T1), shm, s, g); \
    else hipLaunchKernelGGL((spectra_kernel<L2, T1, false>), g1, dim3(T1), shm, s, g);       \
  } while (0)
#define SPECTRA_P(L2)                                                                    \
  do {                                                                                   \
    constexpr int TP = (1 << L2) / 16;                                                   \
    auto kp = a.sc16 ? spectra_persist_kernel<L2, true> : spectra_persist_kernel<L2, false>; \
    hipLaunchKernelGGL(kp, dim3(a.n_cu * resident_blocks((const void *)kp, TP, shm)), dim3(TP), \
                       shm, s, g);                                                       \
  } while (0)
    switch (log2M) {
      case 9: SPECTRA(9); break;
      case 10: SPECTRA(10); break;
      case 11: SPECTRA_P(11); break;
      default: SPECTRA_P(12); break;
    }
#undef SPECTRA
#undef SPECTRA_P
    // (the 128-subcarrier form stores 16 bytes of symbols and 2 of indices per lane: the
    // 64-subcarrier form takes outputs without that alignment)
    const bool v1 = ((uintptr_t)a.out_sym & 15u) || ((uintptr_t)a.out_idx & 1u);
    if (v1) {
      if (a.ref_mode == 1) hipLaunchKernelGGL((apply_split_kernel<8, 1>), g2, dim3(256), 0, s, g);
      else if (a.ref_mode == 2) hipLaunchKernelGGL((apply_split_kernel<8, 2>), g2, dim3(256), 0, s, g);
      else hipLaunchKernelGGL((apply_split_kernel<8, 0>), g2, dim3(256), 0, s, g);
    } else {
      const dim3 g3(NCH / 2, n_frames, P);
      if (a.ref_mode == 1) hipLaunchKernelGGL((apply_split2_kernel<8, 1>), g3, dim3(512), 0, s, g);
      else if (a.ref_mode == 2) hipLaunchKernelGGL((apply_split2_kernel<8, 2>), g3, dim3(512), 0, s, g);
      else hipLaunchKernelGGL((apply_split2_kernel<8, 0>), g3, dim3(512), 0, s, g);
    }
  }
  return kSplitSets;
}

}  // namespace mimo
