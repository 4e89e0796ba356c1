// rub_mimo_amd/csrc/sic_pass.hpp -- what the symbol passes after the batch share
// (sic_pass_kernel in sic_kernels.hip, pic_pass_kernel in pic_kernels.hip): the workgroup's
// frame of (frame, kSicT adjacent carriers, kSicSB symbols), the packed complex multiply-add,
// the slicer and the LDS image that the LLRs leave through. Both files are compiled with
// -ffp-contract=off (llr.hpp says why).
#pragma once

#include <type_traits>

#include "fft.hpp"
#include "kernels.hpp"
#include "llr.hpp"

namespace mimo {

constexpr int kSicT = 128;
constexpr int kSicSB = 32;      // symbols per workgroup
template <int N>
constexpr int sic_sc() { return N <= 2 ? 8 : (N <= 4 ? 4 : 2); }   // symbols per iteration

// acc += a b as two packed fused multiply-adds: (a.x, a.x) b + (a.y, a.y) (-b.y, b.x); br is
// (-b.y, b.x)
MIMO_DEV v2f sic_mac(v2f acc, float2 a, v2f b, v2f br) {
  v2f ax, ay;
  ax.x = ax.y = a.x;
  ay.x = ay.y = a.y;
  acc = __builtin_elementwise_fma(ax, b, acc);
  return __builtin_elementwise_fma(ay, br, acc);
}
MIMO_DEV v2f sic_rot(v2f b) {
  v2f r;
  r.x = -b.y;
  r.y = b.x;
  return r;
}

// qam_demap and qam_point of its index in one go: the levels m of both dimensions give the
// index (gray(mI) << b) | gray(mQ) and the point ((2 m - (L - 1)) scale), as qam_point finds
// it from gray_dec of the index
MIMO_DEV uint32_t sic_slice(v2f z, const Qam &q, v2f *point) {
  const uint32_t mI = qam_level(z.x * q.inv_scale, q.L), mQ = qam_level(z.y * q.inv_scale, q.L);
  point->x = (float)(int32_t)(2 * mI - (q.L - 1)) * q.scale;
  point->y = (float)(int32_t)(2 * mQ - (q.L - 1)) * q.scale;
  return (gray_enc(mI) << q.b) | gray_enc(mQ);
}

// the LLR image of the soft output
constexpr int kSicLlrImg = 40 * 1024;   // 3 workgroups per CU beside the index image
template <int B, bool F32>
constexpr int sic_llr_bps() { return F32 ? 8 * B : 2 * B; }   // LLR bytes per symbol
template <int B, bool F32>
constexpr int sic_llr_rs() { return kSicT * sic_llr_bps<B, F32>() + 16; }   // image row bytes
template <int N, int B, bool F32>
constexpr int sic_soft_sc() {
  int sc = sic_sc<N>();
  while (sc > 1 && sc * N * sic_llr_rs<B, F32>() > kSicLlrImg) sc /= 2;
  return sc;
}

// a symbol's 2 B LLRs into the image: p is aligned as the row's misalignment and the lane
// stride allow (8 bytes for fp32 and 256-QAM int8, 4 for 16-QAM int8, else 2)
template <int B, bool F32>
MIMO_DEV void sic_llr_put(uint8_t *p, const float *v) {
  if constexpr (F32) {
#pragma unroll
    for (int i = 0; i < B; i++)
      reinterpret_cast<float2 *>(p)[i] = make_float2(v[2 * i], v[2 * i + 1]);
  } else if constexpr (B == 4) {
    *reinterpret_cast<uint2 *>(p) = make_uint2(llr_pack4(v), llr_pack4(v + 4));
  } else if constexpr (B == 2) {
    *reinterpret_cast<uint32_t *>(p) = llr_pack4(v);
  } else {
#pragma unroll
    for (int i = 0; i < B; i++)
      reinterpret_cast<uint16_t *>(p)[i] = (uint16_t)(llr_q8(v[2 * i]) | (llr_q8(v[2 * i + 1]) << 8));
  }
}

// The two drains of a pass's LDS images as functions, for passes written after the SIC and PIC
// kernels (those keep theirs inline: sic_kernels.hip says what splitting them changed). Called
// by the whole workgroup after a barrier; `row(q, t)` is the output row of symbol q, stream t of
// the iteration, `rows` = symbols * N of them hold data, nj carriers from carrier j0.
//
// The LLR image (row r at limg + r RS, a row's bytes behind its own misalignment) to d_llr:
// 16-byte chunks, narrower pieces at a row's ends.
template <int N, int B, bool F32, class Row>
MIMO_DEV void sic_llr_drain(const uint8_t *limg, void *llr, uint32_t rows, uint32_t nj,
                            uint64_t mo, uint32_t j0, uint32_t tid, Row row) {
  constexpr int BPS = sic_llr_bps<B, F32>();
  constexpr int RS = sic_llr_rs<B, F32>();
  constexpr int CH = RS / 16;
  typedef uint32_t v4u __attribute__((ext_vector_type(4)));
  typedef typename std::conditional<F32, uint32_t, uint16_t>::type edge_t;   // a row end's pieces
  const uint32_t nb = nj * BPS;
  for (uint32_t w = tid; w < rows * CH; w += kSicT) {
    const uint32_t r = w / CH, c = w - r * CH;
    const uint32_t q = r / N, t = r - q * N;
    uint8_t *dst = reinterpret_cast<uint8_t *>(llr) + (row(q, t) * mo + j0) * BPS;
    const uint32_t mis = (uint32_t)((uintptr_t)dst & 15u);
    const uint8_t *src = limg + r * RS;           // image byte mis is dst[0]
    uint8_t *al = dst - mis;                      // the aligned span: image byte b is al[b]
    const uint32_t b0 = 16 * c;
    if (b0 >= mis && b0 + 16 <= mis + nb) {
      const v4u v = *reinterpret_cast<const v4u *>(src + b0);
      __builtin_nontemporal_store(v, reinterpret_cast<v4u *>(al + b0));
    } else {
      for (uint32_t bb = b0; bb < b0 + 16; bb += sizeof(edge_t))
        if (bb >= mis && bb < mis + nb)
          *reinterpret_cast<edge_t *>(al + bb) = *reinterpret_cast<const edge_t *>(src + bb);
    }
  }
}

// The index image (row r at img + r kSicT) to out_idx: dwords, single bytes at a row's ends.
template <int N, class Row>
MIMO_DEV void sic_idx_drain(const uint8_t *img, uint8_t *out_idx, uint32_t rows, uint32_t nj,
                            uint64_t mo, uint32_t j0, uint32_t tid, Row row) {
  constexpr int SLOTS = kSicT / 4 + 1;   // dwords a row's kSicT index bytes can touch
  for (uint32_t w = tid; w < rows * SLOTS; w += kSicT) {
    const uint32_t r = w / SLOTS, c = w - r * SLOTS;
    const uint32_t q = r / N, t = r - q * N;
    uint8_t *dst = out_idx + row(q, t) * mo + j0;   // the row's nj bytes
    const uint8_t *src = img + r * kSicT;
    const uint32_t mis = (uint32_t)((uintptr_t)dst & 3u);
    const int b0 = (int)(4 * c) - (int)mis;    // dword c of the aligned span: bytes b0..b0+3
    if (b0 >= 0 && b0 + 4 <= (int)nj) {
      uint32_t v;
      if (mis == 0) v = *reinterpret_cast<const uint32_t *>(src + b0);
      else v = (uint32_t)src[b0] | ((uint32_t)src[b0 + 1] << 8) |
               ((uint32_t)src[b0 + 2] << 16) | ((uint32_t)src[b0 + 3] << 24);
      __builtin_nontemporal_store(v, reinterpret_cast<uint32_t *>(dst + b0));
    } else {
      for (int b = 0; b < 4; b++) {
        const int bb = b0 + b;
        if (bb >= 0 && bb < (int)nj) dst[bb] = src[bb];
      }
    }
  }
}

}  // namespace mimo
