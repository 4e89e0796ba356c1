// rub_mimo_amd/csrc/fec_kernels.hip -- K = 7 (133 / 171) Viterbi decoder over rows of int8 LLRs
// on gfx950 (mimo_fec_decode, DESIGN.md "Viterbi decoder"; the definition is in
// include/mimo_rx.h and, as numpy, in rub_mimo_amd/fec.py).
//
// No reference counterpart: the reference stops at the hard demodulated index. A separate,
// opt-in pass over a buffer of LLRs; nothing here is launched by the batch.
//
// One wave decodes one row and lane = trellis state (64 states, wave64). Waves are persistent
// and stride over the rows. All arithmetic is int32, so the output is defined exactly.
//
// Per row, in chunks of 64 trellis steps:
//   LLRs       lane j of chunk c owns step t = 64 c + j: it reads the row positions of A_t and
//              B_t from the position table (perm and the puncturing pattern resolved by the
//              host) and then the two int8 values, one chunk ahead of their use. The ACS loop
//              takes step j's pair from lane j with v_readlane: both are wave-uniform scalars.
//   ACS        state s is entered from p0 = s >> 1 and p1 = p0 | 32 (two ds_bpermute reads of
//              the metric). Both generators contain u_t and u_(t-6), so the outputs of the p1
//              branch are the complements of the p0 branch's: its metric is -bm, with
//              bm = sa L_A + sb L_B and sa, sb = +-1 lane constants. p1 survives where
//              m1 > m0: a tie keeps p0.
//   decisions  kept transposed: lane s shifts its own decision bit into its own word (the sign
//              of m0 - m1 through v_alignbit, one instruction), so no ballot has to be moved
//              into a lane. After 64 steps each lane holds one 8-byte word, the decisions of
//              its state over the chunk, and the chunk leaves as one coalesced 512-byte store
//              into the wave's slice of the workspace.
//   traceback  chunk by chunk from the end: one coalesced 512-byte load, then 64 steps on
//              wave-uniform scalars (v_readlane of the current state's word, one bit of it).
//              The 64 decoded bits of a chunk are two dwords of the packed output.
// The workspace slice is written and read back by the same lanes of the same wave, so program
// order alone makes the loads see the stores.

#include "kernels.hpp"

namespace mimo {

static_assert(kFecChunk == 64, "one decision word per lane of a wave64");

__device__ __forceinline__ int fec_llr(const int8_t *row, uint32_t pos) {
  return pos == kFecPunctured ? 0 : (int)row[pos];
}

// one add-compare-select step: step j's pair from lane j; the lane's own decision (1: p1
// survives, i.e. m1 > m0) is shifted into its word from below, m0 - m1 < 0 being its sign bit
// (|m0 - m1| < 2^31: metrics stay within -2^30 - 6.3 M .. 6.3 M)
__device__ __forceinline__ void fec_acs(int &m, int la_v, int lb_v, int j, int sa, int sb,
                                        int a0, int a1, uint32_t &w) {
  const int la = __builtin_amdgcn_readlane(la_v, j);
  const int lb = __builtin_amdgcn_readlane(lb_v, j);
  const int bm = __mul24(sa, la) + __mul24(sb, lb);
  const int m0 = __builtin_amdgcn_ds_bpermute(a0, m) + bm;
  const int m1 = __builtin_amdgcn_ds_bpermute(a1, m) - bm;
  w = __builtin_amdgcn_alignbit(w, (uint32_t)(m0 - m1), 31);      // (w << 1) | (m1 > m0)
  m = m1 > m0 ? m1 : m0;
}

// one traceback step on wave-uniform values: s the state after step j, w_v the half of the
// decision words that holds step j (at bit 31 - (j & 31) of state s's word). Bit u_j = s & 1
// goes to the packed output (bit k of a row in byte k >> 3 under mask 0x80 >> (k & 7); the
// chunk's 8 bytes are the little-endian dwords olo, ohi); the decision moves s to the state
// before the step
__device__ __forceinline__ void fec_back(uint32_t &s, int w_v, int j, uint32_t &o) {
  const uint32_t w = (uint32_t)__builtin_amdgcn_readlane(w_v, (int)s);
  const uint32_t d = (w >> (31 - (j & 31))) & 1u;
  o |= (s & 1u) << (((j >> 3) & 3) * 8 + 7 - (j & 7));
  s = (s >> 1) | (d << 5);
}

__global__ __launch_bounds__(kFecBlock) void fec_viterbi_kernel(FecArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t wpb = kFecBlock / 64;
  const uint32_t wave = blockIdx.x * wpb + (threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * wpb;
  // lane constants: the predecessors' bpermute addresses and the output signs of the p0 branch
  const int p0 = lane >> 1, u = lane & 1;
  const int a0 = p0 << 2, a1 = (p0 | 32) << 2;
  const int oa = u ^ (p0 >> 1) ^ (p0 >> 2) ^ (p0 >> 4);            // bit k of p0 is u_(t-1-k)
  const int ob = u ^ p0 ^ (p0 >> 1) ^ (p0 >> 2);                    // (u_(t-6) = 0 on this branch)
  const int sa = 1 - 2 * (oa & 1), sb = 1 - 2 * (ob & 1);
  unsigned long long *dw = a.ws + (size_t)wave * a.chunks * kFecChunk;
  const uint32_t chunks = a.chunks;

  for (uint32_t row = wave; row < a.n_rows; row += nwaves) {
    const int8_t *r = a.llr + (size_t)row * a.n_c;
    int m = lane ? -(1 << 30) : 0;
    uint32_t pp = a.pos[lane];
    int la = fec_llr(r, pp & 0xFFFFu), lb = fec_llr(r, pp >> 16);
    uint32_t ppn = chunks > 1 ? a.pos[kFecChunk + lane] : ~0u;
    for (uint32_t c = 0; c < chunks; c++) {
      // the next chunk's LLRs and the positions of the one after it, under this chunk's steps
      const int lan = fec_llr(r, ppn & 0xFFFFu), lbn = fec_llr(r, ppn >> 16);
      const uint32_t ppn2 = c + 2 < chunks ? a.pos[(size_t)(c + 2) * kFecChunk + lane] : ~0u;
      const int n = (int)min(kFecChunk, a.T - c * kFecChunk);
      uint32_t wlo = 0, whi = 0;
      if (n == (int)kFecChunk) {
#pragma unroll
        for (int j = 0; j < 32; j++) fec_acs(m, la, lb, j, sa, sb, a0, a1, wlo);
#pragma unroll
        for (int j = 32; j < 64; j++) fec_acs(m, la, lb, j, sa, sb, a0, a1, whi);
      } else {
        const int n0 = min(n, 32);
        for (int j = 0; j < n0; j++) fec_acs(m, la, lb, j, sa, sb, a0, a1, wlo);
        for (int j = 32; j < n; j++) fec_acs(m, la, lb, j, sa, sb, a0, a1, whi);
        // left-align the part-filled half: step j at bit 31 - (j & 31) as in a full chunk
        if (n < 32) wlo <<= 32 - n;
        else if (n > 32) whi <<= 64 - n;
      }
      dw[(size_t)c * kFecChunk + lane] = ((unsigned long long)whi << 32) | wlo;
      la = lan; lb = lbn; ppn = ppn2;
    }
    if (a.metric && lane == 0) a.metric[row] = m;

    uint32_t *out = reinterpret_cast<uint32_t *>(a.bits) + (size_t)row * a.pitch_dw;
    uint32_t s = 0;
    for (uint32_t c = chunks; c-- > 0;) {
      const unsigned long long w = dw[(size_t)c * kFecChunk + lane];
      const int wlo = (int)(uint32_t)w, whi = (int)(uint32_t)(w >> 32);
      const int n = (int)min(kFecChunk, a.T - c * kFecChunk);
      uint32_t olo = 0, ohi = 0;
      if (n == (int)kFecChunk) {
#pragma unroll
        for (int j = 63; j >= 32; j--) fec_back(s, whi, j, ohi);
#pragma unroll
        for (int j = 31; j >= 0; j--) fec_back(s, wlo, j, olo);
      } else {
        for (int j = n - 1; j >= 32; j--) fec_back(s, whi, j, ohi);
        for (int j = min(n, 32) - 1; j >= 0; j--) fec_back(s, wlo, j, olo);
      }
      // the six tail bits are the low bits of a state that started at 0: they are 0, so every
      // bit >= n_info of these dwords is; dwords past the pitch would hold only such bits
      if (lane == 0) {
        if (2 * c < a.pitch_dw) out[2 * c] = olo;
        if (2 * c + 1 < a.pitch_dw) out[2 * c + 1] = ohi;
      }
    }
    for (uint32_t i = 2 * chunks + lane; i < a.pitch_dw; i += 64) out[i] = 0;
  }
}

void launch_fec_viterbi(const FecArgs &a, uint32_t blocks, hipStream_t s) {
  hipLaunchKernelGGL(fec_viterbi_kernel, dim3(blocks), dim3(kFecBlock), 0, s, a);
}

}  // namespace mimo
