// rub_mimo_amd/csrc/sync_kernels.hip -- the screened Schmidl-Cox path on gfx950, the default
// (sc_screen_kernel, sc_exact_kernel; the algorithm is described below, above the kernels).
// The unscreened item path is in sc_item_kernels.hip, the plateau rule's completion and the
// stream walk in plateau_kernels.hip; sc_common.hpp holds what the three files share.
// (This file keeps the name of the monolith it was cut from: it holds the largest part.)
#include <algorithm>
#include <cstdio>

#include "kernels.hpp"

#pragma clang fp contract(off)

#include "sc_common.hpp"

namespace mimo {

// item_conditions for cp + 2 > kScS without block scans: only a thread whose 16 positions are
// ones on every antenna can hold a candidate, and for it the last zero before its segment is
// found by walking the antenna's words backwards -- at most ~(cp + 2) / 16 words: a longer run
// of ones qualifies whatever lies further back. The walk stops at the item start, which counts
// as a zero (item_conditions' carry = w0 - 1), so the result equals run_cond's leading-run
// branch bit for bit.
MIMO_DEV int item_conditions_walk(const uint16_t *wbits, uint16_t (*acond)[kScT], uint32_t n_done,
                                  int64_t w0, int64_t c0, int64_t cend, int64_t cp) {
  const int tid = threadIdx.x;
  int surv = 0;
#pragma unroll 1
  for (int it = 0; it < kScIters; it++) {
    const int64_t sb = w0 + (int64_t)it * kScIt + kScS * tid;
    const int64_t lo = c0 - sb, hi = cend - sb;
    uint32_t mask = 0;
    if (hi > 0 && lo < kScS) {
      const int l = lo < 0 ? 0 : (int)lo, u = hi > kScS ? kScS : (int)hi;
      mask = ((1u << u) - 1u) & ~((1u << l) - 1u);
    }
    uint32_t all = mask;
    for (uint32_t s = 0; s < n_done; s++) all &= wbits[((int)s * kScIters + it) * kScT + tid];
    uint32_t cond = 0;
    if (all) {
      cond = all;
      for (uint32_t s = 0; s < n_done && cond; s++) {
        const uint32_t bits = wbits[((int)s * kScIters + it) * kScT + tid];
        const uint32_t lead = bits & ~(bits + 1u) & 0xFFFFu;
        int64_t before = w0 - 1;
        int wt = tid, wi = it;
        for (;;) {
          if (--wt < 0) {
            wt = kScT - 1;
            if (--wi < 0) break;
          }
          const int64_t wsb = w0 + (int64_t)wi * kScIt + kScS * wt;
          const uint32_t z = ~(uint32_t)wbits[((int)s * kScIters + wi) * kScT + wt] & 0xFFFFu;
          if (z) { before = wsb + 31 - __clz(z); break; }
          if (sb - wsb > cp + 2) { before = wsb - 1; break; }
        }
        const int64_t i0 = before + cp + 2 - sb;
        cond &= i0 <= 0 ? lead : (i0 >= kScS ? 0u : lead & ~((1u << i0) - 1u));
      }
    }
    acond[it][tid] = (uint16_t)cond;
    surv |= (cond != 0);
  }
  return __syncthreads_or(surv);
}

// ======================================================================================
// Screened S&C (default path). The per-chunk item kernel (sc_item_kernels.hip) scans every chunk of every
// frame and walks the antennas of a plateau chunk one after another in one workgroup; here
//  1. sc_screen_kernel streams antenna 0 once and proves, per block of B positions, that
//     y[n] < thr for every n of the block, from block sums alone: with Sp, Sz, Ap the block
//     sums of p = conj(x[k-M/2]) x[k], |x[k]|^2 and |Re p| + |Im p| (M/2 = D*B),
//       |P[n]| <= |sum_{j=1..D} Sp[b-j]| + Ap[b] + Ap[b-D]
//       2R[n]  >= sum_{j=1..2D-1} Sz[b-j]
//     (fp32 block sums: the bounds are widened by 1e-4 of the absolute sums and the test
//     uses thr - 0.01, far outside the fp32 error of both the sums and the oracle's y).
//     Chunks whose candidate range meets an unproven block are appended to a work list
//     with the first/last unproven position;
//  2. sc_exact_kernel evaluates every (listed chunk, antenna) in parallel, exactly as the item
//     kernel does for one antenna (fp64 running sums, band, deferred near-threshold samples),
//     over the iterations that cover the unproven range and its cp+2 run history;
//  3. sc_resolve_kernel / sc_finalize_kernel (there) resolve the deferred samples and apply
//     the plateau rule per chunk; plateau_kernel completes run starts and the sync index.
// Positions outside the evaluated iterations carry zero bits: for antenna 0 that is exact
// (proven), for the others it only affects run starts, which item_record / plateau_kernel
// then take from an exact backward scan, as for a run that began before a chunk's halo.
// ======================================================================================

// one step of the transposing butterfly: of v[0 .. N) a lane keeps the half selected by its
// lane bit OFF and adds the partner's copy of that half (compile-time indices throughout), with
// no LDS traffic. Offsets 32 and 16 pair lanes l and l ^ OFF through v_permlane32/16_swap: one
// swap of (v[i], v[i + N/2]) leaves a lane its own kept value and the partner's copy of it, so
// the kept sum is the two results added. Offsets 8 and 4 pair lanes through DPP row_mirror
// (l <-> 15 - l in a row) and row_half_mirror (l <-> 7 - l in 8), which flip the same lane bit:
// a lane then holds the sum over lanes l ^ {0, 7, 8, 15} of every row, and the quad sums that
// follow (l ^ {0, 1, 2, 3}) cover each of the 64 lanes once.
template <int CTRL>
MIMO_DEV float dpp_mov(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}
template <int OFF, int N>
MIMO_DEV void tr_reduce_step(float *v, int lane) {
  static_assert(OFF == 32 || OFF == 16 || OFF == 8 || OFF == 4, "lane bits 5..2");
  if constexpr (OFF >= 16) {
#pragma unroll
    for (int i = 0; i < N / 2; i++) {
      const uint32_t a = __float_as_uint(v[i]), b = __float_as_uint(v[i + N / 2]);
      const auto r = OFF == 32 ? __builtin_amdgcn_permlane32_swap(a, b, false, false)
                               : __builtin_amdgcn_permlane16_swap(a, b, false, false);
      v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
  } else {
    const bool up = (lane & OFF) != 0;
#pragma unroll
    for (int i = 0; i < N / 2; i++) {
      const float send = up ? v[i] : v[i + N / 2];
      const float keep = up ? v[i + N / 2] : v[i];
      v[i] = keep + dpp_mov<OFF == 8 ? 0x140 : 0x141>(send);   // row_mirror / row_half_mirror
    }
  }
}

// block sums of antenna 0 over a span, the screen test, and the chunk list
template <bool S, int SPAN>
__global__ __launch_bounds__(kScrT) __attribute__((amdgpu_waves_per_eu(6))) void sc_screen_kernel(ScreenArgs a) {
  constexpr int B = kScrB;
  static_assert(SPAN <= kScrSpan && SPAN % (kScrB * kScrBPI * (kScrT / 64)) == 0, "screen span");
  __shared__ float4 recs[SPAN / B + 2 * (kScrMaxD)];
  // per chunk the test can touch (chunk_len >= kScrSpan / 2: at most three), the first and last
  // unproven position, gathered before the global list update
  constexpr int kScrChunks = 4;
  __shared__ unsigned long long s_cmin[kScrChunks], s_cmax[kScrChunks];
  const uint32_t f = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int D = (int)(a.M / 2) / B, RL = (int)a.M / 2;
  if (a.trig && a.trig[f] != ~0ull) return;           // triggered in an earlier phase
  if (tid < kScrChunks) {
    s_cmin[tid] = ~0ull;
    s_cmax[tid] = 0ull;
  }
  const int64_t L = a.chunk_hi ? std::min<int64_t>((int64_t)a.frame_len,
                                                   (int64_t)(a.chunk_hi * a.chunk_len))
                               : (int64_t)a.frame_len;   // end of this phase's positions
  const int64_t LF = (int64_t)a.frame_len;
  const int64_t q0 = (int64_t)a.chunk_lo * (int64_t)a.chunk_len + (int64_t)blockIdx.x * SPAN;
  if (q0 >= L) return;
  const int NB = SPAN / B + 2 * D;
  const int64_t h0 = q0 - (int64_t)2 * D * B;     // first block of the history
  const auto x = iq_row<S>(a.iq, a.iq_scale, (uint64_t)f * a.N * a.stride);   // antenna 0
  const bool vec = x.pair_ok();
  // block sums: a wave per block, two positions per lane (B = 128); kScrBPI blocks per wave
  // iteration with all their loads issued before the first use (one memory latency per
  // iteration instead of per block)
  for (int j0 = wv * kScrBPI; j0 < NB; j0 += (kScrT / 64) * kScrBPI) {
    float4 cur[kScrBPI], del[kScrBPI];
    const int64_t nb = h0 + (int64_t)j0 * B;
    if (vec && nb - RL >= 0 && nb + (int64_t)kScrBPI * B <= LF && j0 + kScrBPI <= NB) {
#pragma unroll
      for (int b = 0; b < kScrBPI; b++) {
        cur[b] = x.pair(nb + 2 * lane + (int64_t)b * B);
        del[b] = x.pair(nb - RL + 2 * lane + (int64_t)b * B);
      }
    } else {
#pragma unroll
      for (int b = 0; b < kScrBPI; b++) {
        const int64_t n = nb + (int64_t)b * B + 2 * lane;
        cur[b] = ld_pair(x, n, LF, vec);
        del[b] = ld_pair(x, n - RL, LF, vec);
      }
    }
    // per-lane partials v[4 b + c] (c: Re P, Im P, |x|^2, |Re p| + |Im p|), then a transposing
    // butterfly: at offsets 32, 16, 8, 4 a lane keeps half of its values and adds the
    // partner's copy of them (8 + 4 + 2 + 1 exchanges for 16 sums instead of 16 x 6); lanes
    // then hold value (lane >> 2) summed over 16 lanes, and the quad sums finish it
    float v[4 * kScrBPI];
#pragma unroll
    for (int b = 0; b < kScrBPI; b++) {
      const float2 c0 = make_float2(cur[b].x, cur[b].y), c1 = make_float2(cur[b].z, cur[b].w);
      const float2 d0 = make_float2(del[b].x, del[b].y), d1 = make_float2(del[b].z, del[b].w);
      const float2 p0 = cj_mul(d0, c0), p1 = cj_mul(d1, c1);
      v[4 * b + 0] = p0.x + p1.x;
      v[4 * b + 1] = p0.y + p1.y;
      v[4 * b + 2] = (c0.x * c0.x + c0.y * c0.y) + (c1.x * c1.x + c1.y * c1.y);
      v[4 * b + 3] = (fabsf(p0.x) + fabsf(p0.y)) + (fabsf(p1.x) + fabsf(p1.y));
    }
    static_assert(4 * kScrBPI == 16, "transposing reduction of 16 values over 64 lanes");
    tr_reduce_step<32, 16>(v, lane);
    tr_reduce_step<16, 8>(v, lane);
    tr_reduce_step<8, 4>(v, lane);
    tr_reduce_step<4, 2>(v, lane);
    float tot = v[0];
    tot += dpp_mov<0x4E>(tot);   // quad_perm [2, 3, 0, 1]: lane ^ 2
    tot += dpp_mov<0xB1>(tot);   // quad_perm [1, 0, 3, 2]: lane ^ 1
    {
      const int q = lane >> 2, b = q >> 2, c = q & 3;   // value q = 4 b + c
      if ((lane & 3) == 0 && j0 + b < NB) reinterpret_cast<float *>(&recs[j0 + b])[c] = tot;
    }
  }
  __syncthreads();
  const int64_t K = (int64_t)a.chunk_len;
  const int64_t lo_all = (int64_t)a.chunk_lo * K;
  const int64_t c_base = q0 / K;                       // the first chunk the test can touch
  for (int j = 2 * D + tid; j < NB; j += kScrT) {
    const int64_t n0 = h0 + (int64_t)j * B;
    if (n0 >= L) break;
    // positions n < M/2 of a capture that starts at the framesync's origin: every lagged
    // sample x[k - M/2] of P[n] is the empty delay line's zero, so P[n] = 0 and y[n] is 0 (or
    // the oracle's 0/0, compared false) -- never above the threshold. (Block sums cannot show
    // it for the first block, whose energy lower bound is zero, and every capture's chunk 0
    // used to become an exact-pass item for that block alone.)
    if (a.empty_history && n0 + B <= (int64_t)RL) continue;
    // (one pass over the 2D records: each read once; the same sums in the same order)
    double pr = 0.0, pi = 0.0, apw = 0.0, rz = 0.0, azw = 0.0;
    for (int u = 1; u <= 2 * D; u++) {
      const float4 r = recs[j - u];
      if (u <= D) {
        pr += (double)r.x;
        pi += (double)r.y;
        apw += (double)r.w;
      }
      if (u < 2 * D) rz += (double)r.z;
      azw += (double)r.z;
    }
    const double ab = (double)recs[j].w, ad = (double)recs[j - D].w;
    const double pup = sqrt(pr * pr + pi * pi) + ab + ad + 1e-4 * (apw + ab + ad);
    const double rlow = 0.5 * (rz - 1e-4 * (azw + (double)recs[j].z));
    const bool proven = rlow > 0.0 && pup * pup < a.thr_screen * (rlow * rlow);
    if (proven) continue;
    // unproven block: its positions in [lo_all, L) may be candidates -- gathered per chunk in
    // LDS first, so each chunk the workgroup touches costs one set of global atomics (a chain
    // of returning atomics per unproven block kept a workgroup alive ~20 us)
    const int64_t s0 = n0 < lo_all ? lo_all : n0;
    const int64_t s1 = (n0 + B < L ? n0 + B : L) - 1;
    if (s1 < s0) continue;
    for (int64_t c = s0 / K; c <= s1 / K; c++) {
      const int64_t u0 = s0 > c * K ? s0 : c * K, u1 = s1 < (c + 1) * K - 1 ? s1 : (c + 1) * K - 1;
      atomicMin(&s_cmin[c - c_base], (unsigned long long)u0);
      atomicMax(&s_cmax[c - c_base], (unsigned long long)u1);
    }
  }
  __syncthreads();
  if (tid < kScrChunks && s_cmin[tid] != ~0ull) {
    const int64_t c = c_base + tid;
    const uint64_t ci = (uint64_t)f * a.nchunks + (uint64_t)c;
    atomicMin(&a.fmin[ci], s_cmin[tid]);
    atomicMax(&a.fmax[ci], s_cmax[tid]);
    if (atomicOr(&a.flag[ci], 1u) == 0u) {
      const uint32_t slot = atomicAdd(a.count, 1u);
      if (slot < a.cap) {
        ScHot *hp = a.hot + slot;
        hp->f = f;
        hp->n_done = a.N;
        hp->namb = 0;
        hp->arrived = 0;
        hp->chunk = (uint64_t)c;
        hp->c0 = c * K;
        hp->w0 = c * K - ((int64_t)kScSpan - K);
        hp->cend = (c + 1) * K < L ? (c + 1) * K : L;
      }
    }
  }
}

// Ring slot of position p in the exact kernel's LDS ring, which holds positions
// [ib - M, ib + kScIt) of the current iteration at slots (M + p - w0) mod RING.
MIMO_DEV int ring_slot(int64_t p, int64_t w0, int M, int RING) {
  return (int)(((int64_t)M + (p - w0)) % RING);
}

constexpr int kLocAmb = kScT / 2;   // near-threshold samples resolved per iteration pass
// positions spanned by one exact-recompute window: the tables hold M + kResSpread positions,
// sized so that two workgroups fit a CU at M = 2048 (a plateau's two near-threshold edges,
// ~cp + 115 positions apart, still share one window)
constexpr int kResSpread = 512;

// one (listed chunk, antenna): the item kernel's antenna pass over the iterations covering the
// chunk's unproven range (and its cp+2 run history). Near-threshold samples are resolved in
// place with the oracle's exact fp32 chains from the ring (two lanes per sample); the last
// antenna workgroup of an item to finish then applies the plateau rule to the item's words
// (item_conditions / item_record, as sc_finalize_kernel) -- no separate resolve/finalize pass.
template <bool S>
__global__ __launch_bounds__(kScT) __attribute__((amdgpu_waves_per_eu(2)))
void sc_exact_kernel(ScArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sc_dyn[];
  const int M = (int)a.M, RL = M / 2, RING = M + kScIt;
  float2 *ring = reinterpret_cast<float2 *>(sc_dyn);
  __shared__ double scan_ws[2][5][kScT / 64];
  __shared__ long long s_amb[kLocAmb], s_sorted[kLocAmb];
  __shared__ float s_rv[kLocAmb][3];
  // exact-recompute tables after the ring: rtz[i] = 0.5|x|^2 at table position i < W and
  // rtp[i - M/2] = -conj(x[k-M/2]) x[k] for M/2 <= i < W (only those are summed)
  float *rtz = reinterpret_cast<float *>(sc_dyn + sizeof(float2) * ring_pad(RING));
  float2 *rtp = reinterpret_cast<float2 *>(rtz + ((M + kResSpread + 3) & ~3));
  __shared__ int s_namb, s_last;
  // the plateau step's word copy and conditions alias the ring (dead after the iterations)
  uint16_t *fwb = reinterpret_cast<uint16_t *>(sc_dyn);
  uint16_t(*acond)[kScT] = reinterpret_cast<uint16_t(*)[kScT]>(fwb + kMaxStreams * kScIters * kScT);
  __shared__ long long run_ws[2][kScT / 64];
  __shared__ long long flo[kMaxStreams];
  __shared__ unsigned long long s_min;
  const uint32_t count_raw = *a.hot_count;
  const uint32_t count = min(count_raw, a.hot_cap);
  const uint32_t item0 = a.item_lo ? *a.item_lo : 0u;   // items of earlier screen phases: done
  // the next screen phase appends after this phase's items: their count, for its exact launch
  // (the kernel boundary orders this store before the next screen's appends)
  if (a.snap && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *a.snap = count_raw;
  // one (item, antenna) pass per workgroup (blockIdx.x the antenna), walking the item's unproven
  // iterations in turn (splitting them over 2 or 4 workgroups, each with its own M-sample
  // history setup, measured 1.5-2.2x slower: DESIGN.md)
  const uint32_t s = blockIdx.x;
  uint32_t slot = item0 + blockIdx.y;
  // the first slot's record is read before the count is known (it is inside the allocation
  // whatever the count, and used only if the slot is live): in phase 1 (item0 = 0) its loads
  // go out with the count's instead of one memory latency after it
  const ScHot *hs = a.hot + min(slot, a.hot_cap - 1u);
  uint32_t f_n = hs->f;
  int64_t w0_n = hs->w0;
  uint64_t chunk_n = hs->chunk;
  for (; slot < count; slot += gridDim.y) {
  ScHot *hp = a.hot + slot;
  const int tid = threadIdx.x;
  if (tid == 0) s_namb = 0;
  const unsigned long long t_item = a.prof ? (unsigned long long)wall_clock64() : 0ull;
  if (a.prof && tid == 0) atomicMin(&a.prof[0], t_item);
  unsigned long long t_res = 0;
  uint32_t n_win = 0, n_smp = 0;   // diagnostics: resolve windows and samples of this pass
  bool multi_win = false;          // diagnostics: an iteration of this pass had >= 2 windows
  const uint32_t f = f_n;
  const int64_t L = (int64_t)a.frame_len;
  const int64_t w0 = w0_n;
  const uint64_t ci = (uint64_t)f * a.nchunks + chunk_n;
  const int64_t fmin = (int64_t)a.fmin[ci], fmax = (int64_t)a.fmax[ci];
  const unsigned long long t_rec = a.prof ? (unsigned long long)wall_clock64() + (fmin & 0) : 0ull;
  int it_lo = (int)std::max<int64_t>(0, (fmin - (int64_t)a.cp - 2 - w0) / kScIt);
  int it_hi = (int)std::min<int64_t>(kScIters - 1, (fmax - w0) / kScIt);
  const auto x = iq_row<S>(a.iq, a.iq_scale, ((uint64_t)f * a.N + s) * a.stride);
  const bool vec = x.pair_ok();
  if (tid == 0) hp->lo[s] = w0 + (int64_t)it_lo * kScIt;   // first evaluated position
  for (int it = 0; it < kScIters; it++)
    if (it < it_lo || it > it_hi) hp->wbits[((int)s * kScIters + it) * kScT + tid] = 0;
  const int64_t ib_lo = w0 + (int64_t)it_lo * kScIt;
  {
  // the first two blocks' loads, then the history [ib_lo - M, ib_lo) -> its ring slots: all in
  // flight together (the window sums below wait for the history only). Block it_lo + j goes
  // through register set j & 1 (pre, pre2): each iteration refills the set it consumed two
  // blocks ahead, so an iteration's ring fill no longer waits one memory latency on the load
  // the previous iteration issued (the second iteration of a pass did, ~5 us)
  float4 pre[kScIt / (2 * kScT)], pre2[kScIt / (2 * kScT)];
  bool pf = fetch_block(pre, x, ib_lo, L, vec);
  bool pf2 = it_hi > it_lo ? fetch_block(pre2, x, ib_lo + kScIt, L, vec) : false;
  const int wb = (kScIt * it_lo) % RING;
  if (vec && ib_lo - M >= 0 && ib_lo <= L) {
    // all history pairs in flight together, then the ring writes
    constexpr int HU = 4;
    for (int j0 = 0; 2 * j0 < M; j0 += kScT * HU) {
      float4 hv[HU];
#pragma unroll
      for (int u = 0; u < HU; u++) {
        const int j = j0 + u * kScT + tid;
        hv[u] = x.pair(ib_lo - M + 2 * (2 * j < M ? j : 0));
      }
#pragma unroll
      for (int u = 0; u < HU; u++) {
        const int j = j0 + u * kScT + tid;
        if (2 * j < M) {
          int sl = wb + 2 * j;
          if (sl >= RING) sl -= RING;
          *reinterpret_cast<float4 *>(ring + ring_pad(sl)) = hv[u];
        }
      }
    }
  } else {
    for (int j = tid; 2 * j < M; j += kScT) {
      int sl = wb + 2 * j;
      if (sl >= RING) sl -= RING;
      *reinterpret_cast<float4 *>(ring + ring_pad(sl)) = ld_pair(x, ib_lo - M + 2 * j, L, vec);
    }
  }
  __syncthreads();
  // window sums ending at ib_lo - 1: P over the last M/2, 2R and the nonzero count over M
  double c[4] = {0.0, 0.0, 0.0, 0.0}, t4[4], tot[5];
  for (int k = tid; k < M; k += kScT) {
    int sl = wb + k;
    if (sl >= RING) sl -= RING;
    const float2 v = ring[ring_pad(sl)];
    const float z = v.x * v.x + v.y * v.y;
    c[2] += (double)z;
    c[3] += (z != 0.0f) ? 1.0 : 0.0;
    if (k >= RL) {
      int sd = sl - RL;
      if (sd < 0) sd += RING;
      const float2 pp = cj_mul(ring[ring_pad(sd)], v);
      c[0] += (double)pp.x;
      c[1] += (double)pp.y;
    }
  }
  int par = 0;
  block_scan<4>(c, t4, scan_ws[par]);
  par ^= 1;
  double Pc_re = t4[0], Pc_im = t4[1], Zc = t4[2], Cc = t4[3], Ac = t4[2];
  const unsigned long long t_setup = a.prof ? (unsigned long long)wall_clock64() : 0ull;
  if (a.prof && tid == 0) {
    atomicAdd(&a.prof[20], t_rec - t_item);
    atomicAdd(&a.prof[21], t_setup - t_rec);
    atomicAdd(&a.prof[23], (unsigned long long)(it_hi - it_lo + 1));
    atomicMax(&a.prof[25], t_item);
    atomicAdd(&a.prof[26], t_item);
  }
  unsigned long long pq_ring = 0, pq_scan = 0, pq_walk = 0, pq_first = 0;
#pragma unroll 1
  for (int it = it_lo; it <= it_hi; it++) {
    const int64_t ib = w0 + (int64_t)it * kScIt;
    const unsigned long long tq0 = a.prof ? (unsigned long long)wall_clock64() : 0ull;
    const bool odd = ((it - it_lo) & 1) != 0;                  // uniform: register set
    const bool pf_used = odd ? pf2 : pf;
    {
      const int sl0 = (M + it * kScIt) % RING + 2 * tid;
      if (pf_used) {
        if (odd) {
#pragma unroll
          for (int j = 0; j < kScIt / (2 * kScT); j++) {
            int sl = sl0 + 2 * kScT * j;
            if (sl >= RING) sl -= RING;
            *reinterpret_cast<float4 *>(ring + ring_pad(sl)) = pre2[j];
          }
        } else {
#pragma unroll
          for (int j = 0; j < kScIt / (2 * kScT); j++) {
            int sl = sl0 + 2 * kScT * j;
            if (sl >= RING) sl -= RING;
            *reinterpret_cast<float4 *>(ring + ring_pad(sl)) = pre[j];
          }
        }
      } else {   // frame edges: guarded loads straight into the ring
#pragma unroll 1
        for (int j = 0; j < kScIt / (2 * kScT); j++) {
          int sl = sl0 + 2 * kScT * j;
          if (sl >= RING) sl -= RING;
          *reinterpret_cast<float4 *>(ring + ring_pad(sl)) =
              ld_pair(x, ib + 2 * (tid + kScT * j), L, vec);
        }
      }
    }
    __syncthreads();
    const unsigned long long tq1 = a.prof ? (unsigned long long)wall_clock64() : 0ull;
    if (it + 2 <= it_hi) {                        // two blocks ahead, into the set just used
      if (odd) pf2 = fetch_block(pre2, x, ib + 2 * kScIt, L, vec);
      else pf = fetch_block(pre, x, ib + 2 * kScIt, L, vec);
    }
    const float2 *xn = ring + ring_pad((M + it * kScIt + kScS * tid) % RING);
    const float2 *xr = ring + ring_pad((RL + it * kScIt + kScS * tid) % RING);
    const float2 *xm = ring + ring_pad((it * kScIt + kScS * tid) % RING);
    double d[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    float bp = 0.0f, bz = 0.0f;
    int dc = 0;
#pragma unroll 2
    for (int i = 0; i < kScS; i += 2) {
      const float4 vn = *reinterpret_cast<const float4 *>(xn + i);
      const float4 vr = *reinterpret_cast<const float4 *>(xr + i);
      const float4 vm = *reinterpret_cast<const float4 *>(xm + i);
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const float2 n_ = h ? make_float2(vn.z, vn.w) : make_float2(vn.x, vn.y);
        const float2 r_ = h ? make_float2(vr.z, vr.w) : make_float2(vr.x, vr.y);
        const float2 m_ = h ? make_float2(vm.z, vm.w) : make_float2(vm.x, vm.y);
        const float2 pn = cj_mul(r_, n_), pl = cj_mul(m_, r_);
        const float zn = n_.x * n_.x + n_.y * n_.y, zl = m_.x * m_.x + m_.y * m_.y;
        const double zn64 = (double)zn;
        d[0] += (double)pn.x - (double)pl.x;
        d[1] += (double)pn.y - (double)pl.y;
        d[2] += zn64 - (double)zl;
        d[4] += zn64;
        dc += (zn != 0.0f ? 1 : 0) - (zl != 0.0f ? 1 : 0);
        bp += (fabsf(pn.x) + fabsf(pn.y)) + (fabsf(pl.x) + fabsf(pl.y));
        bz += zl;
      }
    }
    d[3] = (double)dc;
    block_scan<5>(d, tot, scan_ws[par]);
    par ^= 1;
    const unsigned long long tq2 = a.prof ? (unsigned long long)wall_clock64() : 0ull;
    double Pre = Pc_re + d[0], Pim = Pc_im + d[1], Z = Zc + d[2], C = Cc + d[3];
    const double Aend = Ac + tot[4];
    const double zfloor = 1e-6 * Aend;
    const int64_t sb = ib + kScS * tid;
    uint32_t bits = 0, ovf = 0;
    bool walk = true;
    {
      const double pmax = sqrt(Pre * Pre + Pim * Pim) + 1.001 * (double)bp;
      const double rmin = 0.5 * (Z - 1.001 * (double)bz);
      if (rmin > 0.0 && Z > 16.0 * zfloor && pmax * pmax < (a.thr - 2.0 * a.band) * (rmin * rmin))
        walk = false;
    }
#pragma unroll 1
    for (int i = 0; walk && i < kScS; i += 2) {
      const float4 vn = *reinterpret_cast<const float4 *>(xn + i);
      const float4 vr = *reinterpret_cast<const float4 *>(xr + i);
      const float4 vm = *reinterpret_cast<const float4 *>(xm + i);
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const float2 n_ = h ? make_float2(vn.z, vn.w) : make_float2(vn.x, vn.y);
        const float2 r_ = h ? make_float2(vr.z, vr.w) : make_float2(vr.x, vr.y);
        const float2 m_ = h ? make_float2(vm.z, vm.w) : make_float2(vm.x, vm.y);
        const float2 pn = cj_mul(r_, n_), pl = cj_mul(m_, r_);
        const float zn = n_.x * n_.x + n_.y * n_.y, zl = m_.x * m_.x + m_.y * m_.y;
        Pre += (double)pn.x - (double)pl.x;
        Pim += (double)pn.y - (double)pl.y;
        Z += (double)zn - (double)zl;
        C += ((zn != 0.0f) ? 1.0 : 0.0) - ((zl != 0.0f) ? 1.0 : 0.0);
        const int64_t n = sb + i + h;
        bool b = false;
        if (n >= 0 && n < L && C > 0.5) {
          const double R = 0.5 * Z, R2 = R * R;
          const double q = Pre * Pre + Pim * Pim - a.thr * R2;
          if (fabs(q) <= a.band * R2 || Z <= zfloor) {
            const int k = atomicAdd(&s_namb, 1);
            b = true;                  // provisional: the recompute below clears it
            if (k < kLocAmb) {
              s_amb[k] = n;            // resolved from the ring
            } else {
              ovf |= 1u << (i + h);   // list full: this lane recomputes it below
            }
          } else {
            b = q > 0.0;
          }
        }
        bits |= (b ? 1u : 0u) << (i + h);
      }
    }
    while (ovf) {   // overflow of the deferred list (pathological input): exact here
      const int i = __ffs((int)ovf) - 1;
      ovf &= ovf - 1u;
      if (!((double)sc_exact(x, sb + i, a.M) > a.thr)) bits &= ~(1u << i);
      if (a.n_exact) atomicAdd(a.n_exact, 1ull);
    }
    __syncthreads();
    const unsigned long long tq3 = a.prof ? (unsigned long long)wall_clock64() : 0ull;
    if (a.prof) {   // per-pass sums, added once per pass (atomics here would time themselves)
      pq_ring += tq1 - tq0;
      pq_scan += tq2 - tq1;
      pq_walk += tq3 - tq2;
      if (it == it_lo) pq_first += tq1 - tq0;
      if (tid == 0 && !pf_used) atomicAdd(&a.prof[24], 1ull);   // diagnostics: guarded ring fills
    }
    const int namb = (a.diag & 8) ? 0 : min(s_namb, kLocAmb);          // uniform
    const unsigned long long t_r0 = a.prof ? (unsigned long long)wall_clock64() : 0ull;
    const uint32_t n_win0 = n_win;
    if (namb > 0) {
      // exact fp32 recompute of this iteration's near-threshold samples (the oracle's chains,
      // as resolve_window): ascending order, then windows of <= kResSpread positions; per
      // window the per-sample terms are tabled from the ring by every thread, then each
      // sample's R chain runs on a lane of waves 0-1 and its P chains on a lane of waves 2-3
      for (int i = tid; i < namb; i += kScT) {
        int rank = 0;
        for (int j = 0; j < namb; j++) rank += (s_amb[j] < s_amb[i]) ? 1 : 0;
        s_sorted[rank] = s_amb[i];
      }
      __syncthreads();
      for (int k = 0; k < namb;) {                    // uniform
        const int64_t nmin = s_sorted[k];
        int e = k + 1;
        while (e < namb && s_sorted[e] - nmin < kResSpread) e++;
        const int64_t q0 = nmin - M + 1;              // table index i <-> position q0 + i
        const int W = (int)(s_sorted[e - 1] - nmin) + M;
        // ring slots of positions q0 + i and q0 + i - RL: one 64-bit remainder per window, then
        // a conditional wrap per entry (i < W < RING) -- a remainder per entry was ~2 us
        const int sq = ring_slot(q0, w0, M, RING);
        const int sqd = sq >= RL ? sq - RL : sq - RL + RING;
        for (int i = tid; i < W; i += kScT) {
          const int sl = sq + i < RING ? sq + i : sq + i - RING;
          const float2 vv = ring[ring_pad(sl)];
          const float z = vv.x * vv.x + vv.y * vv.y;
          rtz[i] = 0.5f * z;
          if (i >= RL) {
            const int sd = sqd + i < RING ? sqd + i : sqd + i - RING;
            const float2 dv = ring[ring_pad(sd)];
            const float2 pp = cj_mul(dv, vv);
            rtp[i - RL] = make_float2((-1.0f) * pp.x, (-1.0f) * pp.y);
          }
        }
        __syncthreads();
        {
          const int g = k + (tid & (kLocAmb - 1));
          if (g < e) {
            const int r = (int)(s_sorted[g] - nmin);
            if (tid < kLocAmb) {
              s_rv[g][0] = seq_sum(rtz + r, M);
            } else {
              const float2 P = seq_sum2(rtp + r, RL);
              s_rv[g][1] = P.x;
              s_rv[g][2] = P.y;
            }
          }
        }
        __syncthreads();
        k = e;
        n_win++;
      }
      n_smp += namb;
      for (int g = 0; g < namb; g++) {
        const int64_t o = s_sorted[g] - sb;
        if (o >= 0 && o < kScS) {
          const float Pr = s_rv[g][1], Pi = s_rv[g][2], R = s_rv[g][0];
          const float y32 = (Pr * Pr + Pi * Pi) / (R * R);
          if (!((double)y32 > a.thr)) bits &= ~(1u << (int)o);
        }
      }
      if (tid == 0 && a.n_exact) atomicAdd(a.n_exact, (unsigned long long)namb);
      __syncthreads();
      if (tid == 0) s_namb = 0;
      if (a.prof) t_res += (unsigned long long)wall_clock64() - t_r0;
    }
    if (a.prof && tid == 0 && n_win > n_win0) {   // diagnostics: windows of this iteration
      atomicMax(&a.prof[27], (unsigned long long)(n_win - n_win0));
      if (n_win - n_win0 >= 2) {
        atomicAdd(&a.prof[28], 1ull);
        multi_win = true;
      }
    }
    Pc_re += tot[0]; Pc_im += tot[1]; Zc += tot[2]; Cc += tot[3]; Ac = Aend;
    hp->wbits[((int)s * kScIters + it) * kScT + tid] = (uint16_t)bits;
    __syncthreads();   // every lane's phase B reads of the ring precede the next block's writes
  }
  if (a.prof && tid == 0) {
    atomicAdd(&a.prof[22], (unsigned long long)wall_clock64() - t_setup - t_res);
    atomicAdd(&a.prof[16], pq_ring);
    atomicAdd(&a.prof[17], pq_scan);
    atomicAdd(&a.prof[18], pq_walk);
    atomicAdd(&a.prof[19], pq_first);
  }
  }
  // the item's last antenna pass: plateau rule over every antenna's words
  if (a.prof && tid == 0) {
    const unsigned long long t = (unsigned long long)wall_clock64();
    atomicMax(&a.prof[1], t);
    atomicAdd(&a.prof[3], t - t_item);
    atomicAdd(&a.prof[4], 1ull);
    atomicAdd(&a.prof[7], t_res);
    // slowest pass: duration (10 ns), iterations, resolve time (10 ns), packed
    const unsigned long long dur = t - t_item;
    atomicMax(&a.prof[13], (dur << 32) | ((unsigned long long)(it_hi - it_lo + 1) << 24) |
                               (t_res & 0xFFFFFFull));
    atomicMax(&a.prof[14], ((unsigned long long)n_win << 32) | n_smp);
    if (multi_win) atomicMax(&a.prof[29], dur);
    atomicAdd(&a.prof[15], (unsigned long long)n_smp);
  }
  __threadfence();
  __syncthreads();
  if (tid == 0)
    s_last = (__hip_atomic_fetch_add(&hp->arrived, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) ==
              hp->n_done - 1u) ? 1 : 0;
  __syncthreads();
  if (s_last && !(a.diag & 16)) {
    // the acquire of the arrival counter (agent scope) invalidated this CU's L1: plain 16-byte
    // loads see every antenna pass's words
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    const uint32_t n_done = hp->n_done;
    const uint4 *src = reinterpret_cast<const uint4 *>(hp->wbits);
    uint4 *dst = reinterpret_cast<uint4 *>(fwb);
    for (int i = tid; i < (int)n_done * kScIters * kScT / 8; i += kScT) dst[i] = src[i];
    if (tid < (int)n_done) flo[tid] = hp->lo[tid];
    if (tid == 0) s_min = ~0ull;
    __syncthreads();
    const unsigned long long tf0 = a.prof ? (unsigned long long)wall_clock64() : 0ull;
    int par = 0;
    const int any = (int64_t)a.cp + 2 > kScS
                        ? item_conditions_walk(fwb, acond, n_done, hp->w0, hp->c0, hp->cend,
                                               (int64_t)a.cp)
                        : item_conditions(fwb, acond, n_done, hp->w0, hp->c0, hp->cend,
                                          (int64_t)a.cp, run_ws, par);
    const unsigned long long tf1 = a.prof ? (unsigned long long)wall_clock64() : 0ull;
    if (any) item_record(a, hp->f, hp->chunk, hp->w0, fwb, acond, flo, s_min);
    if (a.prof && tid == 0) {
      atomicAdd(&a.prof[10], tf1 - tf0);
      atomicAdd(&a.prof[11], (unsigned long long)wall_clock64() - tf1);
      atomicAdd(&a.prof[12], any ? 1ull : 0ull);
      const unsigned long long t = (unsigned long long)wall_clock64();
      atomicMax(&a.prof[2], t);
      atomicAdd(&a.prof[6], 1ull);
    }
  }
  __syncthreads();
  if (slot + gridDim.y < count) {   // the next slot's record (uniform)
    const ScHot *hn = a.hot + slot + gridDim.y;
    f_n = hn->f;
    w0_n = hn->w0;
    chunk_n = hn->chunk;
  }
  }
}

void launch_sc_screen(const ScreenArgs &a, uint32_t n_frames, hipStream_t s) {
  const uint64_t end = a.chunk_hi ? std::min<uint64_t>(a.frame_len, a.chunk_hi * a.chunk_len)
                                  : (uint64_t)a.frame_len;
  const uint64_t span = end - std::min<uint64_t>(end, a.chunk_lo * a.chunk_len);
  // positions per workgroup: 8192 up to M = 2048 (twice the workgroups; a phase-1 screen of
  // 64 C3 captures is ~830 workgroups at 16384, under one per SIMD), 16384 above (the 2D-block
  // history, M positions, would be half of an 8192 span)
  const int sp = a.M <= 2048 ? 8192 : kScrSpan;
  const uint32_t gx = (uint32_t)((span + sp - 1) / sp);
  if (!gx) return;
  if (sp == 8192) {
    if (a.sc16)
      hipLaunchKernelGGL((sc_screen_kernel<true, 8192>), dim3(gx, n_frames), dim3(kScrT), 0, s, a);
    else
      hipLaunchKernelGGL((sc_screen_kernel<false, 8192>), dim3(gx, n_frames), dim3(kScrT), 0, s, a);
  } else if (a.sc16) {
    hipLaunchKernelGGL((sc_screen_kernel<true, kScrSpan>), dim3(gx, n_frames), dim3(kScrT), 0, s, a);
  } else {
    hipLaunchKernelGGL((sc_screen_kernel<false, kScrSpan>), dim3(gx, n_frames), dim3(kScrT), 0, s, a);
  }
}

void launch_sc_exact(const ScArgs &a, hipStream_t s) {
  const size_t shm = sc_table_bytes(a.M) +
                     sizeof(float) * (size_t)((a.M + kResSpread + 3) & ~3u) +
                     sizeof(float2) * (size_t)(a.M / 2 + kResSpread);
  static size_t set_shm[2] = {0, 0};
  const int v = a.sc16 ? 1 : 0;
  auto kern = a.sc16 ? sc_exact_kernel<true> : sc_exact_kernel<false>;
  if (shm != set_shm[v]) {
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)shm);
    set_shm[v] = shm;
  }
  hipLaunchKernelGGL(kern, dim3(a.N, std::min<uint32_t>(a.hot_cap, 256)), dim3(kScT), shm, s, a);
}

}  // namespace mimo
