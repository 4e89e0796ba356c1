// rub_mimo_amd/csrc/fec_enc_kernels.hip -- the K = 7 encoder on gfx950 (mimo_fec_encode_rows):
// packed info bits in, coded rows out, as 0/1 bytes at row positions (G = 1) or as QAM indices
// of G = 2b row positions each (the bit mapper).
//
// One workgroup per row, striding over the rows. Per row, two phases:
//   1. bit-parallel parities: thread w forms the 32 steps t = 32 w .. 32 w + 31 of A and of B
//      from the info words w - 1 and w (MSB first, so u_(t-d) is the stream shifted right by d)
//      and parks them in LDS, step t at bit t & 31 of word t >> 5: A in words [0, nw), B in
//      [nw, 2 nw), and one zero word at 2 nw. Info bits past n_info are masked to 0 here: they
//      are the six tail steps, and whatever else the caller's buffer holds.
//   2. by output position: the inverse position map (row position -> LDS bit address of its A_t
//      or B_t, or of the zero word where no coded bit refers to the position) turns perm and
//      puncturing into a table read. A lane gathers 16 G bits into 16 output bytes and stores
//      them with one 16-byte store; rows whose start is not 16-byte aligned (n_out not a multiple
//      of 16) and the last n_out % 16 bytes of a row go a byte per lane.
// Integer arithmetic throughout: the output is mimo_fec_encode's, bit for bit.
#include "kernels.hpp"

namespace mimo {

namespace {

// info word w of a row, MSB first (bit k of the stream at bit 31 - (k & 31) of word k >> 5),
// zero from bit n_info on
__device__ __forceinline__ uint32_t enc_info_word(const uint32_t *iw, uint32_t w,
                                                  uint32_t n_info) {
  if (32u * w >= n_info) return 0u;
  uint32_t x = __builtin_bswap32(iw[w]);
  const uint32_t rem = n_info - 32u * w;
  if (rem < 32u) x &= ~0u << (32u - rem);
  return x;
}

__device__ __forceinline__ uint32_t enc_bit(const uint32_t *ab, uint32_t e) {
  return (ab[e >> 5] >> (e & 31u)) & 1u;
}

// one output byte: its G map entries, the first one the most significant bit
template <int G>
__device__ __forceinline__ uint32_t enc_byte(const uint32_t *ab, const uint16_t *e) {
  uint32_t v = 0;
#pragma unroll
  for (int i = 0; i < G; i++) v |= enc_bit(ab, e[i]) << (G - 1 - i);
  return v;
}

// the map entries of four output bytes, loaded as one vector
template <int G>
struct alignas(G % 2 ? 8 : 16) EncQuad {
  uint16_t e[4 * G];
};

template <int G>
__global__ __launch_bounds__(kFecEncBlock) void fec_encode_kernel(FecEncArgs a) {
  __shared__ uint32_t ab[2 * kFecEncMaxWords + 1];
  const uint32_t tid = threadIdx.x, nw = a.nw;
  for (uint32_t row = blockIdx.x; row < a.n_rows; row += gridDim.x) {
    const uint32_t *iw = reinterpret_cast<const uint32_t *>(a.info + (size_t)row * a.pitch);
    for (uint32_t w = tid; w < nw; w += kFecEncBlock) {
      const uint32_t cur = enc_info_word(iw, w, a.n_info);
      const uint32_t prev = w ? enc_info_word(iw, w - 1, a.n_info) : 0u;
      const uint64_t v = ((uint64_t)prev << 32) | cur;
      const uint32_t x1 = (uint32_t)(v >> 1), x2 = (uint32_t)(v >> 2), x3 = (uint32_t)(v >> 3),
                     x5 = (uint32_t)(v >> 5), x6 = (uint32_t)(v >> 6);
      const uint32_t c = cur ^ x2 ^ x3 ^ x6;           // the taps 133 and 171 share
      ab[w] = __brev(c ^ x5);
      ab[nw + w] = __brev(c ^ x1);
    }
    if (tid == 0) ab[2 * nw] = 0u;
    __syncthreads();
    const uint64_t base = (uint64_t)row * a.n_out;
    uint8_t *o = a.out + base;
    uint32_t done = 0;
    if ((base & 15u) == 0) {
      const uint32_t units = a.n_out >> 4;
      for (uint32_t s = tid; s < units; s += kFecEncBlock) {
        const EncQuad<G> *q = reinterpret_cast<const EncQuad<G> *>(a.inv) + 4 * (size_t)s;
        uint32_t d[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const EncQuad<G> e = q[j];
          uint32_t v = 0;
#pragma unroll
          for (int k = 0; k < 4; k++) v |= enc_byte<G>(ab, e.e + k * G) << (8 * k);
          d[j] = v;
        }
        *reinterpret_cast<uint4 *>(o + 16 * (size_t)s) = make_uint4(d[0], d[1], d[2], d[3]);
      }
      done = units << 4;
    }
    for (uint32_t b = done + tid; b < a.n_out; b += kFecEncBlock)
      o[b] = (uint8_t)enc_byte<G>(ab, a.inv + (size_t)b * G);
    __syncthreads();                                   // ab is the next row's
  }
}

}  // namespace

bool launch_fec_encode(const FecEncArgs &a, uint32_t group, uint32_t blocks, hipStream_t s) {
  if (a.nw > kFecEncMaxWords) return false;
  switch (group) {
#define ENC_CASE(G)                                                                          \
  case G:                                                                                    \
    hipLaunchKernelGGL(fec_encode_kernel<G>, dim3(blocks), dim3(kFecEncBlock), 0, s, a);     \
    return true;
    ENC_CASE(1) ENC_CASE(2) ENC_CASE(4) ENC_CASE(6) ENC_CASE(8)
#undef ENC_CASE
  }
  return false;
}

}  // namespace mimo
