// rub_mimo_amd/csrc/sc_common.hpp -- constants and device helpers that more than one of the
// Schmidl-Cox kernel files use (sc_item_kernels.hip, sync_kernels.hip,
// plateau_kernels.hip). A helper with one user lives in that file. Each of the three files sets
// `#pragma clang fp contract(off)` before it includes this header.
//
// Reference: framesync::execute_sc_sync (framing.cc:591-637), a per-sample state machine:
//   p[n] = conj(x[n-M/2]) x[n]  (wdelaycf read-before-push, lag M/2)
//   P[n] = -sum_{M/2} p          (firfilt_crcf, taps -1)
//   R[n] = 0.5 sum_M |x|^2       (firfilt_rrrf, taps 0.5)
//   y[n] = |P|^2 / R^2 ;  plateau: y > 0.95 run with end - start > cp on every antenna;
//   sync_index = floor(sum of run starts / N).
#pragma once

#include "kernels.hpp"

namespace mimo {

constexpr int kScT = kScThreads;        // threads per workgroup
constexpr int kScS = 16;                // consecutive positions per thread per iteration
constexpr int kScIt = kScT * kScS;      // 4096 positions per iteration
constexpr int kScIters = kScSpan / kScIt;
static_assert(kScIt == kScIterLen, "iteration length");
static_assert(kScSpan % kScIt == 0, "item span");

// LDS ring slot -> padded float2 index: 2 float2 of padding per 32 keeps the 16-byte reads
// of 16 consecutive threads (16 positions apart) on distinct banks
MIMO_DEV int ring_pad(int i) { return i + ((i >> 5) << 1); }

// Exactness. Samples whose fp64 metric lies within the band of the threshold -- or whose
// window energy is tiny next to the energy streamed so far, where fp64 cancellation could
// matter -- are provisionally 1 and recomputed exactly as the CPU oracle does (sequential fp32
// sums oldest->newest, no FMA: the S&C files are compiled with -ffp-contract=off) once the item
// still has a candidate. A sequential fp32 sum of M terms is within (M-1)u of the exact
// value, so |y32 - y_exact| <= ~4.2e-4 for M <= 2048; the band sc_band(M), 1.25 x
// that bound (about 5.2e-4 at M = 2048, 6.6e-5 at M = 256), keeps every plateau decision --
// hence plateau start/end and sync_index -- bit-identical to the oracle. A sample that finds
// the deferred list full is provisionally 1 as well and recomputed by its own lane (sc_exact).
// An all-zero window (R = 0, the oracle's 0/0) is tracked exactly with a nonzero count.

// exact restatement of framing.cc:626-637 under the pinned liquid semantics, on the M
// samples s[i] = x[n - M + 1 + i] (LDS). The three accumulation chains are interleaved for
// latency; each keeps its own oldest -> newest order.
MIMO_DEV float sc_exact_lds(const float2 *s, int M) {
  constexpr int U = 8;                 // M/2 is a multiple of 32 for every supported M
  const int M2 = M / 2;
  float Pr = 0.0f, Pi = 0.0f, R = 0.0f;
  float2 d[U], v[U], u[2 * U];         // the next block's operands load while this one sums
#pragma unroll
  for (int k = 0; k < U; k++) { d[k] = s[k]; v[k] = s[M2 + k]; }
#pragma unroll
  for (int k = 0; k < 2 * U; k++) u[k] = s[k];
  for (int j = 0; j < M2; j += U) {
    float2 dc[U], vc[U], uc[2 * U];
#pragma unroll
    for (int k = 0; k < U; k++) { dc[k] = d[k]; vc[k] = v[k]; }
#pragma unroll
    for (int k = 0; k < 2 * U; k++) uc[k] = u[k];
    if (j + U < M2) {
#pragma unroll
      for (int k = 0; k < U; k++) { d[k] = s[j + U + k]; v[k] = s[M2 + j + U + k]; }
#pragma unroll
      for (int k = 0; k < 2 * U; k++) u[k] = s[2 * (j + U) + k];
    }
#pragma unroll
    for (int k = 0; k < U; k++) {      // P: k' = n - M/2 + 1 + j + k
      float pr = dc[k].x * vc[k].x - (-dc[k].y) * vc[k].y;
      float pi = dc[k].x * vc[k].y + (-dc[k].y) * vc[k].x;
      Pr = Pr + (-1.0f) * pr;
      Pi = Pi + (-1.0f) * pi;
      float z0 = uc[2 * k].x * uc[2 * k].x + uc[2 * k].y * uc[2 * k].y;   // R: i = 2(j+k)
      R = R + 0.5f * z0;
      float z1 = uc[2 * k + 1].x * uc[2 * k + 1].x + uc[2 * k + 1].y * uc[2 * k + 1].y;
      R = R + 0.5f * z1;
    }
  }
  return (Pr * Pr + Pi * Pi) / (R * R);
}

// the same straight from global memory (one lane; list overflow and the rare backward scan)
template <bool S>
MIMO_DEV float sc_exact(const Iq<S> x, int64_t n, int64_t M) {
  const int64_t M2 = M / 2;
  float Pr = 0.0f, Pi = 0.0f, R = 0.0f;
  for (int64_t k = n - M2 + 1; k <= n; k++) {
    float2 d = (k - M2 >= 0) ? x.at(k - M2) : make_float2(0.0f, 0.0f);
    float2 v = (k >= 0) ? x.at(k) : make_float2(0.0f, 0.0f);
    float pr = d.x * v.x - (-d.y) * v.y;
    float pi = d.x * v.y + (-d.y) * v.x;
    Pr = Pr + (-1.0f) * pr;
    Pi = Pi + (-1.0f) * pi;
  }
  for (int64_t k = n - M + 1; k <= n; k++) {
    float2 v = (k >= 0) ? x.at(k) : make_float2(0.0f, 0.0f);
    float z = v.x * v.x + v.y * v.y;
    R = R + 0.5f * z;
  }
  return (Pr * Pr + Pi * Pi) / (R * R);
}
MIMO_DEV float sc_exact(const float2 *__restrict__ x, int64_t n, int64_t M) {
  return sc_exact(Iq<false>{x}, n, M);
}


// a double moved across lanes by one DPP control (both halves; lanes with no source, or in a
// row the row mask leaves out, read 0.0)
template <int CTRL, int ROWS = 0xF>
MIMO_DEV double dpp_f64(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, ROWS, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, ROWS, 0xF, true);
  return __hiloint2double(hi, lo);
}

// wave-inclusive scan of NV doubles on the DPP path (row_shr 1, 2, 4, 8 within rows of 16,
// then row_bcast 15 and 31 across rows): VALU moves, no LDS round trip per step as the
// ds_bpermute of __shfl_up
template <int NV>
MIMO_DEV void wave_scan_f64(double (&x)[NV]) {
#pragma unroll
  for (int k = 0; k < NV; k++) x[k] += dpp_f64<0x111>(x[k]);
#pragma unroll
  for (int k = 0; k < NV; k++) x[k] += dpp_f64<0x112>(x[k]);
#pragma unroll
  for (int k = 0; k < NV; k++) x[k] += dpp_f64<0x114>(x[k]);
#pragma unroll
  for (int k = 0; k < NV; k++) x[k] += dpp_f64<0x118>(x[k]);
#pragma unroll
  for (int k = 0; k < NV; k++) x[k] += dpp_f64<0x142, 0xA>(x[k]);
#pragma unroll
  for (int k = 0; k < NV; k++) x[k] += dpp_f64<0x143, 0xC>(x[k]);
}

// block-wide exclusive scan of NV doubles plus the block totals (one barrier; the caller
// alternates ws between consecutive scans)
template <int NV>
MIMO_DEV void block_scan(double (&v)[NV], double (&tot)[NV], double (*ws)[kScT / 64]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double inc[NV];
#pragma unroll
  for (int k = 0; k < NV; k++) inc[k] = v[k];
  wave_scan_f64<NV>(inc);
  if (lane == 63) {
#pragma unroll
    for (int k = 0; k < NV; k++) ws[k][wv] = inc[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; k++) {
    double o = 0.0, t = 0.0;
#pragma unroll
    for (int w = 0; w < kScT / 64; w++) {
      const double u = ws[k][w];
      if (w < wv) o += u;
      t += u;
    }
    v[k] = o + (inc[k] - v[k]);
    tot[k] = t;
  }
}

// "run of cp+2 ones ends at n" for the 16 positions sb..sb+15 of this thread. carry is the
// last zero before the iteration (block-uniform, updated to the last zero through it).
MIMO_DEV uint32_t run_cond(uint32_t bits, int64_t sb, long long &carry, int64_t cp,
                           long long *red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t inv = ~bits & 0xFFFFu;
  const long long lz = inv ? (long long)(sb + 31 - __clz(inv)) : -1;
  long long inc = lz;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const long long o = __shfl_up(inc, off);
    if (lane >= off && o > inc) inc = o;
  }
  long long ex = __shfl_up(inc, 1);
  if (lane == 0) ex = -1;
  if (lane == 63) red[wv] = inc;
  __syncthreads();
  long long before = carry, all = carry;
#pragma unroll
  for (int w = 0; w < kScT / 64; w++) {
    const long long u = red[w];
    if (w < wv && u > before) before = u;
    if (u > all) all = u;
  }
  if (ex > before) before = ex;
  uint32_t cond = 0;
  if (cp + 2 > kScS) {
    // a zero inside the segment is < cp+2 positions back, so only the leading run of ones
    // (bits 0..i all set) can qualify, and only where the last zero before it is old enough
    const uint32_t lead = bits & ~(bits + 1u) & 0xFFFFu;
    const long long i0 = before + cp + 2 - sb;
    cond = i0 <= 0 ? lead : (i0 >= kScS ? 0u : lead & ~((1u << i0) - 1u));
  } else {
#pragma unroll
    for (int i = 0; i < kScS; i++) {
      const uint32_t m = inv & ((2u << i) - 1u);
      const long long lzv = m ? (long long)(sb + 31 - __clz(m)) : before;
      if (lzv <= sb + i - cp - 2) cond |= 1u << i;
    }
  }
  carry = all;
  return cond;
}

// sequential fp32 sum q[0] + q[1] + ... + q[n-1], in that order. Scalar head up to 16-byte
// alignment, then 16-byte reads with the next 16 terms in flight while 16 are added (the
// dependent-add latency, ~7 cycles on gfx950, is the bound: ~9 cycles per term measured).
// Sequential fp32 sums in the oracle's order, oldest -> newest, from an LDS table. The chain
// of dependent adds is the critical path, so the table reads run three 16-term blocks ahead
// (the loop is unrolled by three so the blocks rotate through fixed registers; a read past the
// last block is clamped onto it and never consumed).
MIMO_DEV float seq_sum(const float *q, int n) {
  float acc = 0.0f;
  const int h = min(n, (int)((4u - (((uint32_t)(uintptr_t)q >> 2) & 3u)) & 3u));
  for (int k = 0; k < h; k++) acc = acc + q[k];
  const float4 *qa = reinterpret_cast<const float4 *>(q + h);
  const int m = n - h, nb = m >> 4;
  if (nb > 0) {
    auto ld = [&](float4 (&d)[4], int b) {
      const int bb = b < nb ? b : nb - 1;
#pragma unroll
      for (int i = 0; i < 4; i++) d[i] = qa[4 * bb + i];
    };
    auto add = [&](const float4 (&d)[4]) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        acc = acc + d[i].x; acc = acc + d[i].y; acc = acc + d[i].z; acc = acc + d[i].w;
      }
    };
    float4 A[4], B[4], C[4];
    ld(A, 0); ld(B, 1); ld(C, 2);
    int b = 0;
    for (; b + 3 <= nb; b += 3) {
      add(A); ld(A, b + 3);
      add(B); ld(B, b + 4);
      add(C); ld(C, b + 5);
    }
    if (b < nb) add(A);
    if (b + 1 < nb) add(B);
  }
  for (int k = h + 16 * nb; k < n; k++) acc = acc + q[k];
  return acc;
}

// two interleaved sequential sums over complex terms (the .x and .y chains), same scheme
MIMO_DEV float2 seq_sum2(const float2 *q, int n) {
  float ax = 0.0f, ay = 0.0f;
  const int h = min(n, (int)((((uint32_t)(uintptr_t)q) >> 3) & 1u));
  for (int k = 0; k < h; k++) { ax = ax + q[k].x; ay = ay + q[k].y; }
  const float4 *qa = reinterpret_cast<const float4 *>(q + h);
  const int m = n - h, nb = m >> 3;
  if (nb > 0) {
    auto ld = [&](float4 (&d)[4], int b) {
      const int bb = b < nb ? b : nb - 1;
#pragma unroll
      for (int i = 0; i < 4; i++) d[i] = qa[4 * bb + i];
    };
    auto add = [&](const float4 (&d)[4]) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        ax = ax + d[i].x; ay = ay + d[i].y; ax = ax + d[i].z; ay = ay + d[i].w;
      }
    };
    float4 A[4], B[4], C[4];
    ld(A, 0); ld(B, 1); ld(C, 2);
    int b = 0;
    for (; b + 3 <= nb; b += 3) {
      add(A); ld(A, b + 3);
      add(B); ld(B, b + 4);
      add(C); ld(C, b + 5);
    }
    if (b < nb) add(A);
    if (b + 1 < nb) add(B);
  }
  for (int k = h + 8 * nb; k < n; k++) { ax = ax + q[k].x; ay = ay + q[k].y; }
  return make_float2(ax, ay);
}

// two consecutive samples (q even), zero outside [0, L)
template <bool S>
MIMO_DEV float4 ld_pair(const Iq<S> x, int64_t q, int64_t L, bool vec) {
  if (vec && q >= 0 && q + 1 < L) return x.pair(q);
  const float2 v0 = (q >= 0 && q < L) ? x.at(q) : make_float2(0.0f, 0.0f);
  const float2 v1 = (q + 1 >= 0 && q + 1 < L) ? x.at(q + 1) : make_float2(0.0f, 0.0f);
  return make_float4(v0.x, v0.y, v1.x, v1.y);
}
MIMO_DEV float4 ld_pair(const float2 *__restrict__ x, int64_t q, int64_t L, bool vec) {
  return ld_pair(Iq<false>{x}, q, L, vec);
}

// one iteration's 4096 samples from q0 into registers, 16 bytes per lane, when the block is
// inside [0, L) (block-uniform); otherwise false and the ring is filled by guarded loads
template <bool S>
MIMO_DEV bool fetch_block(float4 (&pre)[kScIt / (2 * kScT)], const Iq<S> x,
                          int64_t q0, int64_t L, bool vec) {
  const bool ok = vec && q0 >= 0 && q0 + kScIt <= L;
  const int64_t p0 = (ok ? q0 : 0) + 2 * (int64_t)threadIdx.x;
  // one branch around all loads (a per-element select makes hipcc wait for each load in turn)
  if (ok) {
#pragma unroll
    for (int j = 0; j < kScIt / (2 * kScT); j++) pre[j] = x.pair(p0 + 2 * kScT * j);
  } else {
#pragma unroll
    for (int j = 0; j < kScIt / (2 * kScT); j++) pre[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  return ok;
}
MIMO_DEV bool fetch_block(float4 (&pre)[kScIt / (2 * kScT)], const float2 *__restrict__ x,
                          int64_t q0, int64_t L, bool vec) {
  return fetch_block(pre, Iq<false>{x}, q0, L, vec);
}

// conj(d) * v, the oracle's operation order
MIMO_DEV float2 cj_mul(float2 d, float2 v) {
  return make_float2(d.x * v.x - (-d.y) * v.y, d.x * v.y + (-d.y) * v.x);
}

// plateau rule for antennas [0, n_done) from their words into acond (candidates only in
// [c0, cend)); returns the block-wide OR of the surviving bits
MIMO_DEV int item_conditions(const uint16_t *wbits, uint16_t (*acond)[kScT], uint32_t n_done,
                             int64_t w0, int64_t c0, int64_t cend, int64_t cp,
                             long long (*run_ws)[kScT / 64], int &par) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int it = 0; it < kScIters; it++) acond[it][tid] = 0xFFFFu;
  for (uint32_t s = 0; s < n_done; s++) {
    long long carry = w0 - 1;
#pragma unroll 1
    for (int it = 0; it < kScIters; it++) {
      const int64_t sb = w0 + (int64_t)it * kScIt + kScS * tid;
      const uint32_t bits = wbits[((int)s * kScIters + it) * kScT + tid];
      par ^= 1;
      const uint32_t cond = run_cond(bits, sb, carry, cp, run_ws[par]);
      const int64_t lo = c0 - sb, hi = cend - sb;
      uint32_t mask = 0;
      if (hi > 0 && lo < kScS) {
        const int l = lo < 0 ? 0 : (int)lo, u = hi > kScS ? kScS : (int)hi;
        mask = ((1u << u) - 1u) & ~((1u << l) - 1u);
      }
      acond[it][tid] = (uint16_t)(acond[it][tid] & cond & mask);
    }
  }
  int surv = 0;
#pragma unroll
  for (int it = 0; it < kScIters; it++) surv |= (acond[it][tid] != 0);
  return __syncthreads_or(surv);
}

// first qualifying position -> the chunk's record (run starts from the words) and trig[f].
// s_min must be ~0 on entry.
MIMO_DEV void item_record(const ScArgs &a, uint32_t f, uint64_t chunk, int64_t w0,
                          const uint16_t *wbits, const uint16_t (*acond)[kScT],
                          const long long *lo_s, unsigned long long &s_min) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int it = 0; it < kScIters; it++) {
    const uint32_t v = acond[it][tid];
    if (v)
      atomicMin(&s_min, (unsigned long long)(w0 + (int64_t)it * kScIt + kScS * tid +
                                             __ffs((int)v) - 1));
  }
  __syncthreads();
  const unsigned long long cand = s_min;
  if (cand == ~0ull) return;
  ScRecord *rec = a.rec + (uint64_t)f * a.rec_stride + chunk;
  if (wv == 0) {   // run start: one past the last zero below the candidate
    bool found = false;
    if (lane < (int)a.N) {
      const int s = lane;
      const int64_t o = (int64_t)cand - w0;
      int it = (int)(o / kScIt), t = (int)((o % kScIt) / kScS);
      const int i = (int)(o % kScS);
      uint32_t m = ~(uint32_t)wbits[(s * kScIters + it) * kScT + t] & ((1u << i) - 1u);
      while (!m) {   // rare: only for a candidate item
        if (--t < 0) { t = kScT - 1; if (--it < 0) break; }
        m = ~(uint32_t)wbits[(s * kScIters + it) * kScT + t] & 0xFFFFu;
      }
      const long long lzv =
          m ? (long long)(w0 + (int64_t)it * kScIt + kScS * t + 31 - __clz(m)) : -1;
      found = lzv >= lo_s[s];    // a computed zero, not the evaluation boundary
      // found: the run start; otherwise where plateau_kernel's exact backward scan begins
      rec->start[s] = found ? (unsigned long long)(lzv + 1) : (unsigned long long)lo_s[s];
    }
    const unsigned long long fm = __ballot(found);
    if (lane == 0) {
      rec->found = (uint32_t)fm;
      rec->n_cand = cand;
      rec->pos0 = w0;
      atomicMin(&a.trig[f], cand);
      if (a.cand) a.cand[(uint64_t)f * a.nchunks + chunk] = cand;
    }
  }
}

}  // namespace mimo
