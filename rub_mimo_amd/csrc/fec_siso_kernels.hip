// rub_mimo_amd/csrc/fec_siso_kernels.hip -- max-log-MAP (soft-in soft-out) decoder of the K = 7
// (133 / 171) code over rows of int8 LLRs on gfx950 (mimo_fec_siso, DESIGN.md "Soft-output
// decoder"; the definition is in include/mimo_rx.h and, as numpy, in rub_mimo_amd/fec.py).
//
// No reference counterpart. A separate, opt-in pass; nothing here is launched by the batch.
//
// The Viterbi kernel's frame (fec_kernels.hip): one wave per row, one lane per trellis state,
// persistent waves striding over the rows, the same position table, chunks of 64 trellis steps
// with lane j of a chunk owning step j's two LLRs. All arithmetic is int32 max and plus without
// overflow, so the output is defined exactly whatever the order of evaluation.
//
// Lane <-> state. Both output bits are GF(2)-linear in the state, so the states are relabelled:
// lane l holds the state p with
//   l = A0(p) << 5 | B0(p) << 4 | (p & 15),   A0 = p1 ^ p2 ^ p4 ^ p5,   B0 = p0 ^ p1 ^ p2 ^ p5
// (A0, B0): the outputs of the transition that leaves p with u_t = 0; the one with u_t = 1 has
// the complements, both generators containing u_t). The map is invertible (p5 = B0 ^ p0 ^ p1 ^
// p2, p4 = A0 ^ p1 ^ p2 ^ p5) and sends state 0 to lane 0. The four 16-lane DPP rows of the wave
// are then the four classes (A0, B0), and only the ds_bpermute addresses know about it.
//
// Per row:
//   forward    alpha by the Viterbi add-compare-select without decisions. At every chunk start
//              the wave stores its 64 alpha values (one coalesced 256-byte store) into its slice
//              of the workspace.
//   backward   chunk by chunk from the end: load the chunk's checkpoint, recompute the chunk's
//              alpha vectors into 64 registers (fully unrolled, static indices), then the beta
//              recursion for j = 63..0. Lane p as predecessor has the branches to s0 = 2p & 63
//              (metric g) and s0 | 1 (metric -g):
//                b0 = g + beta(s0), b1 = -g + beta(s1), beta_t(p) = max(b0, b1),
//                e0 = alpha_t(p) + b0, e1 = alpha_t(p) + b1.
//   reductions e0 and e1 are reduced over each 16-lane row (4 DPP stages each) and the eight row
//              maxima X[ab] (of e0) and Y[ab] (of e1) leave through v_readlane. On scalars:
//                M^u(0) = max X, M^u(1) = max Y,
//                M^A(0) = max(X[0.], Y[1.]), M^A(1) = max(X[1.], Y[0.]),
//                M^B(0) = max(X[.0], Y[.1]), M^B(1) = max(X[.1], Y[.0]).
//   stores     step j's three clamped int8 values are parked in lane j; per chunk
//              lane j stores its two coded values at its two row positions (punctured entries
//              skipped) and its info LLR; the 64 info-bit decisions leave as two dwords.
// A part-filled last chunk runs exactly T mod 64 steps (a zero-LLR step is not neutral: it would
// spread beta_T's 0 from state 0 into state 32). It is one chunk of a row, so it takes rolled
// loops: the forward sweep leaves its alpha vectors in the workspace (64 more vectors per wave)
// and the backward loop reads them back; the unrolled code of the full chunks has no tests.
// The workspace slice is written and read back by the same lanes of the same wave, so program
// order alone makes the loads see the stores.

#include "kernels.hpp"

namespace mimo {

static_assert(kFecChunk == 64, "one step per lane of a wave64");

constexpr int kSisoNeg = -(1 << 29);

__device__ __forceinline__ int siso_llr(const int8_t *row, uint32_t pos) {
  return pos == kFecPunctured ? 0 : (int)row[pos];
}

// the state held by lane l, and the lane that holds state p
__device__ __forceinline__ int siso_state(int l) {
  const int p5 = ((l >> 4) ^ l ^ (l >> 1) ^ (l >> 2)) & 1;
  const int p4 = ((l >> 5) ^ (l >> 1) ^ (l >> 2) ^ p5) & 1;
  return (l & 15) | (p4 << 4) | (p5 << 5);
}
__device__ __forceinline__ int siso_lane(int p) {
  const int a0 = ((p >> 1) ^ (p >> 2) ^ (p >> 4) ^ (p >> 5)) & 1;
  const int b0 = (p ^ (p >> 1) ^ (p >> 2) ^ (p >> 5)) & 1;
  return (a0 << 5) | (b0 << 4) | (p & 15);
}

// one forward step: alpha_(t+1) of the lane's state from its two predecessors (lanes a0 / 4,
// a1 / 4), step j's LLR pair from lane j
__device__ __forceinline__ int siso_fwd(int m, int la_v, int lb_v, int j, int sa, int sb, int a0,
                                        int a1) {
  const int la = __builtin_amdgcn_readlane(la_v, j);
  const int lb = __builtin_amdgcn_readlane(lb_v, j);
  const int bm = __mul24(sa, la) + __mul24(sb, lb);
  const int m0 = __builtin_amdgcn_ds_bpermute(a0, m) + bm;
  const int m1 = __builtin_amdgcn_ds_bpermute(a1, m) - bm;
  return max(m0, m1);
}

// the maximum over each 16-lane row, in every lane of the row: quad_perm [1,0,3,2] and
// [2,3,0,1], row_half_mirror, row_mirror (every source lane exists; bound_ctrl with old = 0 only
// lets the move fold into v_max_i32_dpp)
__device__ __forceinline__ int siso_row_max(int v) {
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true));
  return v;
}

__device__ __forceinline__ int siso_clamp(int v) { return min(max(v, -127), 127); }

// one backward step j of a chunk: beta_(t+1) -> beta_t in `beta`, the three Lambdas of the step
// on scalars; clamp(Lambda^A) | clamp(Lambda^B) << 8 | clamp(Lambda^u) << 16 goes into lane j of
// `park`, the decision Lambda^u < 0 into `o` at the packed output's bit of step j (as fec_back).
// kStatic: j is a constant after unrolling and the parked value leaves the scalar unit through
// v_writelane (a select on lane == j makes the compiler keep 64 lane masks alive and spill them)
template <bool kStatic>
__device__ __forceinline__ void siso_bwd(int &beta, int alpha, int la_v, int lb_v, int j, int ga,
                                         int gb, int a0, int a1, int ext, int lane, int &park,
                                         uint32_t &o) {
  const int la = __builtin_amdgcn_readlane(la_v, j);
  const int lb = __builtin_amdgcn_readlane(lb_v, j);
  const int g = __mul24(ga, la) + __mul24(gb, lb);
  const int b0 = __builtin_amdgcn_ds_bpermute(a0, beta) + g;
  const int b1 = __builtin_amdgcn_ds_bpermute(a1, beta) - g;
  beta = max(b0, b1);
  const int r0 = siso_row_max(alpha + b0), r1 = siso_row_max(alpha + b1);
  const int x00 = __builtin_amdgcn_readlane(r0, 0), x01 = __builtin_amdgcn_readlane(r0, 16);
  const int x10 = __builtin_amdgcn_readlane(r0, 32), x11 = __builtin_amdgcn_readlane(r0, 48);
  const int y00 = __builtin_amdgcn_readlane(r1, 0), y01 = __builtin_amdgcn_readlane(r1, 16);
  const int y10 = __builtin_amdgcn_readlane(r1, 32), y11 = __builtin_amdgcn_readlane(r1, 48);
  const int x0_ = max(x00, x01), x1_ = max(x10, x11), y0_ = max(y00, y01), y1_ = max(y10, y11);
  const int lu = max(x0_, x1_) - max(y0_, y1_);
  const int lA = max(x0_, y1_) - max(x1_, y0_) - ext * la;
  const int lB = max(max(x00, x10), max(y01, y11)) - max(max(x01, x11), max(y00, y10)) - ext * lb;
  const int v = (siso_clamp(lA) & 0xFF) | ((siso_clamp(lB) & 0xFF) << 8) |
                ((siso_clamp(lu) & 0xFF) << 16);
  if constexpr (kStatic)
    asm("v_writelane_b32 %0, %1, %2"
        : "+v"(park)
        : "s"(__builtin_amdgcn_readfirstlane(v)), "i"(j));
  else park = lane == j ? v : park;
  o |= ((uint32_t)lu >> 31) << (((j >> 3) & 3) * 8 + 7 - (j & 7));
}

__global__ __launch_bounds__(kFecBlock) void fec_siso_kernel(FecSisoArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t wpb = kFecBlock / 64;
  // (wave-uniform, and said so: the row loop and the row's pointers then stay on the scalar unit)
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * wpb + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * wpb;
  // lane constants. Forward, the lane's state s as successor: the predecessors' lanes and the
  // output signs of the p0 branch (as in fec_viterbi_kernel). Backward, s as predecessor: the
  // successors' lanes and the output signs of the u = 0 branch, which are lane bits 5 and 4
  const int s = siso_state(lane);
  const int q0 = s >> 1, u = s & 1;
  const int fa0 = siso_lane(q0) << 2, fa1 = siso_lane(q0 | 32) << 2;
  const int oa = u ^ (q0 >> 1) ^ (q0 >> 2) ^ (q0 >> 4);
  const int ob = u ^ q0 ^ (q0 >> 1) ^ (q0 >> 2);
  const int sa = 1 - 2 * (oa & 1), sb = 1 - 2 * (ob & 1);
  const int ba0 = siso_lane((2 * s) & 63) << 2, ba1 = siso_lane(((2 * s) & 63) | 1) << 2;
  const int ga = 1 - 2 * ((lane >> 5) & 1), gb = 1 - 2 * ((lane >> 4) & 1);
  // the wave's slice: a checkpoint per chunk, then the alpha vectors of a part-filled last chunk
  int *ck = a.ws + (size_t)wave * (a.chunks + kFecChunk) * kFecChunk;
  int *pk = ck + (size_t)a.chunks * kFecChunk;
  const uint32_t chunks = a.chunks, n_info = a.T - 6;
  const int ext = (int)a.ext;

  for (uint32_t row = wave; row < a.n_rows; row += nwaves) {
    const int8_t *r = a.llr + (size_t)row * a.n_c;
    // ---- forward: alpha, a checkpoint at every chunk start ----
    int m = lane ? kSisoNeg : 0;
    uint32_t pp = a.pos[lane];
    int la = siso_llr(r, pp & 0xFFFFu), lb = siso_llr(r, pp >> 16);
    uint32_t ppn = chunks > 1 ? a.pos[kFecChunk + lane] : ~0u;
    for (uint32_t c = 0; c < chunks; c++) {
      const int lan = siso_llr(r, ppn & 0xFFFFu), lbn = siso_llr(r, ppn >> 16);
      const uint32_t ppn2 = c + 2 < chunks ? a.pos[(size_t)(c + 2) * kFecChunk + lane] : ~0u;
      const int n = (int)min(kFecChunk, a.T - c * kFecChunk);
      ck[(size_t)c * kFecChunk + lane] = m;
      if (n == (int)kFecChunk) {
#pragma unroll
        for (int j = 0; j < 64; j++) m = siso_fwd(m, la, lb, j, sa, sb, fa0, fa1);
      } else {
        // the part-filled last chunk: its alpha vectors stay in the workspace for the way back
        for (int j = 0; j < n; j++) {
          pk[(size_t)j * kFecChunk + lane] = m;
          m = siso_fwd(m, la, lb, j, sa, sb, fa0, fa1);
        }
      }
      if (c + 1 < chunks) { pp = ppn; la = lan; lb = lbn; }
      ppn = ppn2;
    }
    if (a.metric && lane == 0) a.metric[row] = m;

    // ---- backward: per chunk the alpha vectors again, then beta and the reductions ----
    // pp, la, lb are the last chunk's; the chunk below it is fetched under this chunk's steps
    int beta = lane ? kSisoNeg : 0;
    int8_t *orow = a.out ? a.out + (size_t)row * a.n_c : nullptr;
    int8_t *irow = a.info_llr ? a.info_llr + (size_t)row * a.info_pitch : nullptr;
    uint32_t *brow = a.bits ? reinterpret_cast<uint32_t *>(a.bits) + (size_t)row * a.pitch_dw
                            : nullptr;
    ppn = chunks > 1 ? a.pos[(size_t)(chunks - 2) * kFecChunk + lane] : ~0u;
    for (uint32_t c = chunks; c-- > 0;) {
      const int lan = siso_llr(r, ppn & 0xFFFFu), lbn = siso_llr(r, ppn >> 16);
      const uint32_t ppn2 = c >= 2 ? a.pos[(size_t)(c - 2) * kFecChunk + lane] : ~0u;
      const int n = (int)min(kFecChunk, a.T - c * kFecChunk);
      int park = 0;
      uint32_t olo = 0, ohi = 0;
      if (n == (int)kFecChunk) {
        int al[kFecChunk];
        al[0] = ck[(size_t)c * kFecChunk + lane];
#pragma unroll
        for (int j = 0; j < 63; j++) al[j + 1] = siso_fwd(al[j], la, lb, j, sa, sb, fa0, fa1);
#pragma unroll
        for (int j = 63; j >= 32; j--)
          siso_bwd<true>(beta, al[j], la, lb, j, ga, gb, ba0, ba1, ext, lane, park, ohi);
#pragma unroll
        for (int j = 31; j >= 0; j--)
          siso_bwd<true>(beta, al[j], la, lb, j, ga, gb, ba0, ba1, ext, lane, park, olo);
      } else {
        for (int j = n - 1; j >= 32; j--)
          siso_bwd<false>(beta, pk[(size_t)j * kFecChunk + lane], la, lb, j, ga, gb, ba0, ba1, ext,
                          lane, park, ohi);
        for (int j = min(n, 32) - 1; j >= 0; j--)
          siso_bwd<false>(beta, pk[(size_t)j * kFecChunk + lane], la, lb, j, ga, gb, ba0, ba1, ext,
                          lane, park, olo);
      }
      // lanes >= n hold punctured entries (the table is padded with them) and park 0
      const uint32_t pa = pp & 0xFFFFu, pb = pp >> 16;
      if (orow) {
        if (pa != kFecPunctured) orow[pa] = (int8_t)(park & 0xFF);
        if (pb != kFecPunctured) orow[pb] = (int8_t)((park >> 8) & 0xFF);
      }
      const uint32_t k = c * kFecChunk + lane;
      if (irow && k < n_info) irow[k] = (int8_t)((park >> 16) & 0xFF);
      // the six tail steps have no path with u_t = 1 that avoids a NEG start, so their Lambda^u
      // is positive and every bit >= n_info of these dwords is 0; dwords past the pitch would
      // hold only such bits
      if (brow && lane == 0) {
        if (2 * c < a.pitch_dw) brow[2 * c] = olo;
        if (2 * c + 1 < a.pitch_dw) brow[2 * c + 1] = ohi;
      }
      pp = ppn; la = lan; lb = lbn; ppn = ppn2;
    }
    if (brow)
      for (uint32_t i = 2 * chunks + lane; i < a.pitch_dw; i += 64) brow[i] = 0;
    if (irow)
      for (uint32_t i = n_info + lane; i < a.info_pitch; i += 64) irow[i] = 0;
  }
}

void launch_fec_siso(const FecSisoArgs &a, uint32_t blocks, hipStream_t s) {
  hipLaunchKernelGGL(fec_siso_kernel, dim3(blocks), dim3(kFecBlock), 0, s, a);
}

}  // namespace mimo
