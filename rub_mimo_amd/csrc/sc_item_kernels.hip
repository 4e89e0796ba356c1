// rub_mimo_amd/csrc/sc_item_kernels.hip -- the unscreened Schmidl-Cox item path on gfx950:
//   sc_kernel          : persistent grid over (frame, chunk) items, every antenna of an item
//   sc_resolve_kernel  : hot items, exact recompute of the near-threshold samples
//   sc_finalize_kernel : hot items, plateau rule on the corrected words
// The default screened path is in sync_kernels.hip, the plateau rule's completion and the
// stream walk in plateau_kernels.hip; sc_common.hpp holds what they share.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "kernels.hpp"

#pragma clang fp contract(off)

#include "sc_common.hpp"

// cycle counters of the item kernel (build with -DMIMO_SC_PROFILE and run with RMIMO_SC_PROF=1)
#ifdef MIMO_SC_PROFILE
#define SC_PROF(...) __VA_ARGS__
#else
#define SC_PROF(...)
#endif

namespace mimo {

constexpr int kAmbMax = kScAmbMax;      // provisional samples per item
constexpr int kResGroup = kScT / 2;     // samples per resolve pass (two lanes each)
constexpr int kResWin = 4;              // resolve workgroups per (item, antenna): windows in parallel

// the recompute tables of one window: tz[i] = 0.5 |x[q0+i]|^2, tp[i] = -conj(x[q0+i-M/2]) x[q0+i]
// (the oracle's tap products, same fp32 operations). Loads are unconditional from clamped
// addresses and masked afterwards: a per-element "load or zero" select makes hipcc branch
// around each load and wait for it before the next (one memory latency per element);
// kTabU iterations' loads are in flight together
constexpr int kTabU = 8;
MIMO_DEV void table_fill(const float2 *__restrict__ x, int64_t q0, int64_t L, int RL, int WCAP,
                         float *tz, float2 *tp) {
  const int tid = threadIdx.x;
  for (int i0 = 0; i0 < WCAP; i0 += kScT * kTabU) {
    float2 v[kTabU], dd[kTabU];
#pragma unroll
    for (int u = 0; u < kTabU; u++) {
      const int64_t k = q0 + i0 + u * kScT + tid, kd = k - RL;
      v[u] = x[k < 0 ? 0 : (k >= L ? L - 1 : k)];
      dd[u] = x[kd < 0 ? 0 : (kd >= L ? L - 1 : kd)];
    }
#pragma unroll
    for (int u = 0; u < kTabU; u++) {
      const int i = i0 + u * kScT + tid;
      const int64_t k = q0 + i, kd = k - RL;
      const float2 vv = (k >= 0 && k < L) ? v[u] : make_float2(0.0f, 0.0f);
      const float2 dv = (kd >= 0 && kd < L) ? dd[u] : make_float2(0.0f, 0.0f);
      if (i < WCAP) {
        float z = vv.x * vv.x + vv.y * vv.y;
        tz[i] = 0.5f * z;
        const float2 pp = cj_mul(dv, vv);
        tp[i] = make_float2((-1.0f) * pp.x, (-1.0f) * pp.y);
      }
    }
  }
}

struct ResolveLds {            // LDS scratch of the exact recompute
  unsigned long long key;
  int ng;
  int res_i[kResGroup];
  float res_v[3][kResGroup];
};

// Exact fp32 recompute of the pending samples pos[i] (antenna ant[i]; pos0 keeps the
// positions, pos[i] becomes -1 once taken), a batch per (antenna, table window). The oracle's
// per-sample terms -pr, -pi (P taps -1) and 0.5|x|^2 (R taps 0.5) are tabled once per window
// with the same fp32 operations; each sample's three sequential sums then run on two lanes
// (R; Pr and Pi interleaved), oldest -> newest exactly as framing.cc:626-637 under the pinned
// liquid semantics. A sample whose exact metric fails the threshold clears its bit in wbits
// ([antenna][iteration][thread] x 16 bits, LDS or global).
MIMO_DEV void resolve_pending(const ScArgs &a, uint32_t f, int64_t w0, long long *pos,
                              const long long *pos0, const uint8_t *ant, int namb,
                              uint16_t *wbits, unsigned char *tables, int table_bytes,
                              ResolveLds &rl) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int M = (int)a.M, RL = M / 2;
  const int64_t L = (int64_t)a.frame_len;
  const int WCAP = (table_bytes / 12) & ~3;
  float *tz = reinterpret_cast<float *>(tables);
  float2 *tp = reinterpret_cast<float2 *>(tables + sizeof(float) * WCAP);
  for (;;) {
    if (tid == 0) { rl.key = ~0ull; rl.ng = 0; }
    __syncthreads();
    for (int i = tid; i < namb; i += kScT)
      if (pos[i] >= 0)
        atomicMin(&rl.key, ((unsigned long long)ant[i] << 48) | (unsigned long long)pos[i]);
    __syncthreads();
    const unsigned long long key = rl.key;
    if (key == ~0ull) break;   // block-uniform
    const int s = (int)(key >> 48);
    const int64_t nmin = (int64_t)(key & ((1ull << 48) - 1));
    const int64_t q0 = nmin - M + 1;       // table index i <-> sample q0 + i
    const float2 *__restrict__ x = a.iq + ((uint64_t)f * a.N + s) * a.stride;
    table_fill(x, q0, L, RL, WCAP, tz, tp);
    // this window's samples (at most kResGroup per pass; the rest wait for the next pass)
    for (int i = tid; i < namb; i += kScT) {
      const int64_t n = pos[i];
      if (n >= 0 && ant[i] == s && n - nmin <= WCAP - M) {
        const int g = atomicAdd(&rl.ng, 1);
        if (g < kResGroup) { rl.res_i[g] = i; pos[i] = -1; }
      }
    }
    __syncthreads();
    const int ng = rl.ng < kResGroup ? rl.ng : kResGroup;
    if (a.prof && tid == 0) {                     // diagnostics (RMIMO_SC_PROF=1)
      atomicAdd(&a.prof[17], 1ull);
      atomicAdd(&a.prof[19], (unsigned long long)ng);
    }
    {
      const int g = lane + 64 * (wv >> 1);
      if (g < ng) {
        const int r = (int)(pos0[rl.res_i[g]] - nmin);
        if ((wv & 1) == 0) {          // R over i = r .. r + M - 1
          rl.res_v[0][g] = seq_sum(tz + r, M);
        } else {                      // P over i = r + M/2 .. r + M - 1
          const float2 P = seq_sum2(tp + r + RL, RL);
          rl.res_v[1][g] = P.x;
          rl.res_v[2][g] = P.y;
        }
      }
    }
    __syncthreads();
    if (tid < ng) {
      const float Pr = rl.res_v[1][tid], Pi = rl.res_v[2][tid], R = rl.res_v[0][tid];
      const float y32 = (Pr * Pr + Pi * Pi) / (R * R);
      if (!((double)y32 > a.thr)) {
        const int64_t o = pos0[rl.res_i[tid]] - w0;
        const int it = (int)(o / kScIt), t = (int)((o % kScIt) / kScS);
        const int bit = (int)(o % kScS) + 16 * (t & 1);
        uint32_t *w32 = reinterpret_cast<uint32_t *>(wbits) + ((s * kScIters + it) * kScT + t) / 2;
        atomicAnd(w32, ~(1u << bit));
      }
    }
    __syncthreads();
  }
}

// Exact fp32 recompute of one window's samples sorted[0 .. cnt) of antenna s (ascending,
// sorted[cnt-1] - sorted[0] <= WCAP - M): the same table and chains as resolve_pending, for a
// window chosen by the caller, so that the windows of one antenna run in parallel workgroups
MIMO_DEV void resolve_window(const ScArgs &a, uint32_t f, int64_t w0, int s,
                             const long long *sorted, int cnt, uint16_t *wbits,
                             unsigned char *tables, int table_bytes, ResolveLds &rl) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int M = (int)a.M, RL = M / 2;
  const int64_t L = (int64_t)a.frame_len;
  const int WCAP = (table_bytes / 12) & ~3;
  float *tz = reinterpret_cast<float *>(tables);
  float2 *tp = reinterpret_cast<float2 *>(tables + sizeof(float) * WCAP);
  const int64_t nmin = sorted[0];
  const int64_t q0 = nmin - M + 1;         // table index i <-> sample q0 + i
  const float2 *__restrict__ x = a.iq + ((uint64_t)f * a.N + s) * a.stride;
  table_fill(x, q0, L, RL, WCAP, tz, tp);
  __syncthreads();
  {
    const int g = lane + 64 * (wv >> 1);
    if (g < cnt) {
      const int r = (int)(sorted[g] - nmin);
      if ((wv & 1) == 0) {          // R over i = r .. r + M - 1
        rl.res_v[0][g] = seq_sum(tz + r, M);
      } else {                      // P over i = r + M/2 .. r + M - 1
        const float2 P = seq_sum2(tp + r + RL, RL);
        rl.res_v[1][g] = P.x;
        rl.res_v[2][g] = P.y;
      }
    }
  }
  __syncthreads();
  if (tid < cnt) {
    const float Pr = rl.res_v[1][tid], Pi = rl.res_v[2][tid], R = rl.res_v[0][tid];
    const float y32 = (Pr * Pr + Pi * Pi) / (R * R);
    if (!((double)y32 > a.thr)) {
      const int64_t o = sorted[tid] - w0;
      const int it = (int)(o / kScIt), t = (int)((o % kScIt) / kScS);
      const int bit = (int)(o % kScS) + 16 * (t & 1);
      uint32_t *w32 = reinterpret_cast<uint32_t *>(wbits) + ((s * kScIters + it) * kScT + t) / 2;
      atomicAnd(w32, ~(1u << bit));
    }
  }
  __syncthreads();
}

// GPU form (throughput, not a per-sample scan). A persistent grid pulls (frame, chunk) items
// from a queue in chunk-major order. An item is kScSpan = 16384 positions: a halo of
// H >= cp+2 positions (run history) and K = kScSpan - H candidate positions. For each antenna
// the workgroup streams the item through an LDS ring of M + 4096 samples (coalesced 16-byte
// loads, the next 4096 samples in flight while the current ones are processed); thread t
// owns 16 consecutive positions per 4096-sample iteration. With the window sums written as
// running differences,
//   P[n] = P[n-1] + p[n] - p[n-M/2],   2R[n] = 2R[n-1] + |x[n]|^2 - |x[n-M]|^2,
// each thread sums its segment's differences, one block scan (fp64) gives every segment its
// starting sums, and the thread walks its 16 positions. The decision is division-free:
// |P|^2 - thr R^2 against band * R^2.
//
// "Run of cp+2 ones ending at n" is a last-zero prefix max (block scan per iteration).
// Antennas are processed in order and the item stops as soon as no position can still
// qualify on every antenna (provisional ones only enlarge that set, so the early-out is
// safe); noise and data regions cost one antenna, not N. The first qualifying n is
// atomicMin'ed into trig[frame] and the item records each antenna's run start from its LDS
// bits; plateau_kernel completes a run that began before the halo with an exact backward
// scan. Items beyond a frame's current trigger are skipped; results never depend on
// dispatch order (an item is skipped only when a smaller trigger already exists, and the
// kept candidate is the global minimum).
__global__ __launch_bounds__(kScT) __attribute__((amdgpu_waves_per_eu(2))) void sc_kernel(ScArgs a, uint32_t n_frames) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sc_dyn[];
  const int M = (int)a.M, RL = M / 2, RING = M + kScIt;
  float2 *ring = reinterpret_cast<float2 *>(sc_dyn);
  // provisional plateau bits, [antenna][iteration][thread] x 16
  uint16_t *wbits = reinterpret_cast<uint16_t *>(sc_dyn + sizeof(float2) * ring_pad(RING));
  __shared__ uint16_t acond[kScIters][kScT];
  __shared__ double scan_ws[2][5][kScT / 64];
  __shared__ long long run_ws[2][kScT / 64];
  __shared__ unsigned long long s_trig, s_min;
  __shared__ uint32_t s_item;
  __shared__ long long amb_n[kAmbMax];     // -1 once taken by a resolve pass
  __shared__ long long amb_pos[kAmbMax];
  __shared__ uint8_t amb_s[kAmbMax];
  __shared__ int s_namb;
  __shared__ uint32_t s_slot;
  __shared__ ResolveLds rl;
  __shared__ long long s_lo[kMaxStreams];
  __shared__ unsigned long long s_smin, s_smax;

  const int tid = threadIdx.x;
  const int64_t L = (int64_t)a.frame_len, cp = a.cp;
  const int64_t K = (int64_t)a.chunk_len, H = (int64_t)kScSpan - K;
  const uint64_t total = (a.chunk_hi - a.chunk_lo) * n_frames;
  int par = 0;
    SC_PROF(if (a.prof && tid == 0) atomicMin(&a.prof[8], (unsigned long long)wall_clock64());)

  for (;;) {
    if (tid == 0) s_item = atomicAdd(a.queue, 1u);
    __syncthreads();
    const uint64_t item = s_item;
    if (item >= total) {
    SC_PROF(if (a.prof && tid == 0) atomicMax(&a.prof[9], (unsigned long long)wall_clock64());)
      break;
    }
    const uint32_t f = (uint32_t)(item % n_frames);
    const uint64_t chunk = a.chunk_lo + item / n_frames;
    const int64_t c0 = (int64_t)chunk * K;
    if (tid == 0) {
      s_trig = __hip_atomic_load(&a.trig[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_min = ~0ull;
      s_namb = 0;
    }
#pragma unroll
    for (int it = 0; it < kScIters; it++) acond[it][tid] = 0xFFFFu;
    __syncthreads();
    if (c0 >= L || (!a.no_skip && s_trig < (unsigned long long)c0)) {  // an earlier trigger exists
    SC_PROF(if (a.prof && tid == 0) atomicAdd(&a.prof[6], 1ull);)
      continue;
    }
    SC_PROF(const long long t_item = clock64();)
    SC_PROF(const long long w_item = wall_clock64();)
    SC_PROF(long long t_rows = 0, t_words = 0, t_ph[5] = {0, 0, 0, 0, 0};)
    const int64_t w0 = c0 - H;                 // first evaluated position
    const int64_t cend = std::min<int64_t>(c0 + K, L);
    int any = 1;
    uint32_t n_done = 0;
    // antenna 0 evaluates the whole item; antenna s > 0 only the iterations covering the
    // survivors of antennas < s (and their cp+2 run history): a plateau region is short
    int it_lo = 0, it_hi = kScIters - 1;

    for (uint32_t s = 0; s < a.N && any; s++) {
    SC_PROF(const long long t_r0 = clock64();)
      const float2 *__restrict__ x = a.iq + ((uint64_t)f * a.N + s) * a.stride;
      const bool vec = ((uintptr_t)x & 15u) == 0;
      const int64_t ib_lo = w0 + (int64_t)it_lo * kScIt;   // first evaluated position
      if (tid == 0) s_lo[s] = ib_lo;
      for (int it = 0; it < kScIters; it++)
        if (it < it_lo || it > it_hi) {
          acond[it][tid] = 0;
          wbits[((int)s * kScIters + it) * kScT + tid] = 0;
        }
      // history [ib_lo - M, ib_lo) -> its ring slots; the first block in flight behind it
      const int wb = (kScIt * it_lo) % RING;
      for (int j = tid; 2 * j < M; j += kScT) {
        int sl = wb + 2 * j;
        if (sl >= RING) sl -= RING;
        *reinterpret_cast<float4 *>(ring + ring_pad(sl)) = ld_pair(x, ib_lo - M + 2 * j, L, vec);
      }
      float4 pre[kScIt / (2 * kScT)];
      bool pf = fetch_block(pre, x, ib_lo, L, vec);
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
      block_scan<4>(c, t4, scan_ws[par]);
    SC_PROF(long long t_m = clock64();)
    SC_PROF(t_ph[0] += t_m - t_r0;)
      par ^= 1;
      double Pc_re = t4[0], Pc_im = t4[1], Zc = t4[2], Cc = t4[3], Ac = t4[2];
      long long carry = ib_lo - 1;             // the evaluation boundary reads as a zero

#pragma unroll 1
      for (int it = it_lo; it <= it_hi; it++) {
        const int64_t ib = w0 + (int64_t)it * kScIt;
        {
          const int slot = (M + it * kScIt) % RING + 2 * tid;
          if (pf) {
#pragma unroll
            for (int j = 0; j < kScIt / (2 * kScT); j++) {
              int sl = slot + 2 * kScT * j;
              if (sl >= RING) sl -= RING;
              *reinterpret_cast<float4 *>(ring + ring_pad(sl)) = pre[j];
            }
          } else {   // frame edges: guarded loads straight into the ring
#pragma unroll 1
            for (int j = 0; j < kScIt / (2 * kScT); j++) {
              int sl = slot + 2 * kScT * j;
              if (sl >= RING) sl -= RING;
              *reinterpret_cast<float4 *>(ring + ring_pad(sl)) =
                  ld_pair(x, ib + 2 * (tid + kScT * j), L, vec);
            }
          }
        }
        __syncthreads();
        if (it + 1 <= it_hi) pf = fetch_block(pre, x, ib + kScIt, L, vec);
        const float2 *xn = ring + ring_pad((M + it * kScIt + kScS * tid) % RING);
        const float2 *xr = ring + ring_pad((RL + it * kScIt + kScS * tid) % RING);
        const float2 *xm = ring + ring_pad((it * kScIt + kScS * tid) % RING);
        // phase A: this segment's sum of window differences
        // (plus |dP| and lagged-energy sums that bound y over the segment)
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
        SC_PROF({ const long long t2 = clock64(); t_ph[1] += t2 - t_m; t_m = t2; })
        block_scan<5>(d, tot, scan_ws[par]);
        SC_PROF({ const long long t2 = clock64(); t_ph[2] += t2 - t_m; t_m = t2; })
        par ^= 1;
        // phase B: walk the segment
        double Pre = Pc_re + d[0], Pim = Pc_im + d[1], Z = Zc + d[2], C = Cc + d[3];
        const double Aend = Ac + tot[4];       // energy streamed through this iteration
        const double zfloor = 1e-6 * Aend;
        const int64_t sb = ib + kScS * tid;
        uint32_t bits = 0, ovf = 0;
        // Every n of the segment has |P[n]| <= |P_s| + bp and 2R[n] >= Z_s - bz. If that bound
        // keeps y below thr - 2*band everywhere (and the fp64 sums are far from cancellation),
        // all 16 decisions are 0 and the walk is skipped -- the common case away from a sync.
        bool walk = true;
        {
          const double pmax = sqrt(Pre * Pre + Pim * Pim) + 1.001 * (double)bp;
          const double rmin = 0.5 * (Z - 1.001 * (double)bz);
          if (rmin > 0.0 && Z > 16.0 * zfloor && pmax * pmax < (a.thr - 2.0 * a.band) * (rmin * rmin))
            walk = false;
        }
#pragma unroll 1
        for (int i = 0; walk && i < kScS; i += 2) {   // rare: near a plateau
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
                const int slot = atomicAdd(&s_namb, 1);
                b = true;                 // provisional: the recompute clears it
                if (slot < kAmbMax) {
                  amb_n[slot] = n;
                  amb_pos[slot] = n;
                  amb_s[slot] = (uint8_t)s;
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
        while (ovf) {   // overflow of the provisional list (pathological input): exact here
          const int i = __ffs((int)ovf) - 1;
          ovf &= ovf - 1u;
          if (!((double)sc_exact(x, sb + i, a.M) > a.thr)) bits &= ~(1u << i);
          if (a.n_exact) atomicAdd(a.n_exact, 1ull);
        }
        Pc_re += tot[0]; Pc_im += tot[1]; Zc += tot[2]; Cc += tot[3]; Ac = Aend;
        wbits[((int)s * kScIters + it) * kScT + tid] = (uint16_t)bits;
        SC_PROF({ const long long t2 = clock64(); t_ph[3] += t2 - t_m; t_m = t2; })
        const uint32_t cond = run_cond(bits, sb, carry, cp, run_ws[par]);
        // candidates only inside [c0, cend)
        const int64_t lo = c0 - sb, hi = cend - sb;
        uint32_t mask = 0;
        if (hi > 0 && lo < kScS) {
          const int l = lo < 0 ? 0 : (int)lo, u = hi > kScS ? kScS : (int)hi;
          mask = ((1u << u) - 1u) & ~((1u << l) - 1u);
        }
        acond[it][tid] = (uint16_t)(acond[it][tid] & cond & mask);
        SC_PROF({ const long long t2 = clock64(); t_ph[4] += t2 - t_m; t_m = t2; })
      }
    SC_PROF(const long long t_r1 = clock64();)
    SC_PROF(t_rows += t_r1 - t_r0;)
      if (tid == 0) { s_smin = ~0ull; s_smax = 0ull; }
      __syncthreads();
      {
        uint64_t lo = ~0ull, hi = 0ull;
#pragma unroll
        for (int it = 0; it < kScIters; it++) {
          const uint32_t v = acond[it][tid];
          if (v) {
            const uint64_t base = (uint64_t)(w0 + (int64_t)it * kScIt + kScS * tid);
            lo = std::min<uint64_t>(lo, base + __ffs((int)v) - 1);
            hi = std::max<uint64_t>(hi, base + 31 - __clz(v));
          }
        }
        if (lo != ~0ull) { atomicMin(&s_smin, (unsigned long long)lo); atomicMax(&s_smax, (unsigned long long)hi); }
      }
      __syncthreads();
      any = (s_smin != ~0ull) ? 1 : 0;
      if (any) {
        const int64_t ra = (int64_t)s_smin - cp - 2, rb = (int64_t)s_smax;
        it_lo = (int)std::max<int64_t>(0, (ra - w0) / kScIt);
        it_hi = (int)std::min<int64_t>(kScIters - 1, (rb - w0) / kScIt);
      }
      n_done = s + 1;
    SC_PROF(t_words += clock64() - t_r1;)
    }

    const int namb = s_namb < kAmbMax ? s_namb : kAmbMax;
    SC_PROF(const long long t_res0 = clock64();)
    if (any && namb > 0) {
      if (a.n_exact && tid == 0) atomicAdd(a.n_exact, (unsigned long long)namb);
      // hand the item to the hot-item kernels (every antenna's windows resolve in parallel);
      // resolve here only when the hot buffer is full
      if (tid == 0) s_slot = a.hot ? atomicAdd(a.hot_count, 1u) : ~0u;
      __syncthreads();
      if (s_slot < a.hot_cap) {
        ScHot *hp = a.hot + s_slot;
        if (tid == 0) {
          hp->f = f; hp->n_done = n_done; hp->namb = (uint32_t)namb;
          hp->chunk = chunk; hp->c0 = c0; hp->w0 = w0; hp->cend = cend;
        }
        if (tid < (int)n_done) hp->lo[tid] = s_lo[tid];
        for (int i = tid; i < namb; i += kScT) { hp->amb_n[i] = amb_pos[i]; hp->amb_s[i] = amb_s[i]; }
        uint32_t *dst = reinterpret_cast<uint32_t *>(hp->wbits);
        const uint32_t *src = reinterpret_cast<const uint32_t *>(wbits);
        for (int i = tid; i < (int)n_done * kScIters * kScT / 2; i += kScT) dst[i] = src[i];
        any = 0;
      } else {
        resolve_pending(a, f, w0, amb_n, amb_pos, amb_s, namb, wbits, sc_dyn,
                        (int)(sizeof(float2) * ring_pad(RING)), rl);
        any = item_conditions(wbits, acond, n_done, w0, c0, cend, cp, run_ws, par);
      }
    }
#ifdef MIMO_SC_PROFILE
    if (a.prof && tid == 0) {
      const long long t_end = clock64();
      atomicAdd(&a.prof[0], 1ull);
      atomicAdd(&a.prof[1], (unsigned long long)n_done);
      atomicAdd(&a.prof[2], (unsigned long long)t_rows);
      atomicAdd(&a.prof[3], (unsigned long long)t_words);
      for (int k = 0; k < 5; k++) atomicAdd(&a.prof[12 + k], (unsigned long long)t_ph[k]);
      atomicAdd(&a.prof[4], (unsigned long long)(t_end - t_res0));
      atomicAdd(&a.prof[5], (unsigned long long)(t_end - t_item));
      const long long w_end = wall_clock64();
      atomicAdd(&a.prof[7], (unsigned long long)(w_end - w_item));
      atomicMax(&a.prof[10], (unsigned long long)(w_end - w_item));
      atomicMax(&a.prof[11], (unsigned long long)w_item);
    }
#endif
    if (any) item_record(a, f, chunk, w0, wbits, acond, s_lo, s_min);
    __syncthreads();
  }
}

// hot items, stage 1: one workgroup per (item, antenna) resolves that antenna's pending samples
// against the capture and clears the failing bits of the item's saved plateau words
__global__ __launch_bounds__(kScT) void sc_resolve_kernel(ScArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tables[];
  __shared__ long long pos[kAmbMax], sorted[kAmbMax];
  __shared__ int wstart[kAmbMax + 1];
  __shared__ ResolveLds rl;
  __shared__ int s_n, s_nw;
  const uint32_t s = blockIdx.y;
  const int tid = threadIdx.x;
  const int table_bytes = (int)(sizeof(float2) * ring_pad((int)a.M + kScIt));
  const int WCAP = (table_bytes / 12) & ~3;
  const uint32_t count = min(*a.hot_count, a.hot_cap);
  for (uint32_t h = blockIdx.x; h < count; h += gridDim.x) {
    ScHot *hp = a.hot + h;
    if (s >= hp->n_done) continue;
    if (tid == 0) s_n = 0;
    __syncthreads();
    const int namb = (int)min(hp->namb, (uint32_t)kAmbMax);
    for (int i = tid; i < namb; i += kScT)
      if (hp->amb_s[i] == s) pos[atomicAdd(&s_n, 1)] = hp->amb_n[i];
    __syncthreads();
    const int n = s_n;
    if (n == 0) continue;                          // block-uniform
    if (tid == 0 && a.n_exact && blockIdx.z == 0) atomicAdd(a.n_exact, (unsigned long long)n);
    // ascending order (positions of one antenna are distinct), then greedy windows: a window
    // opens at its smallest sample and takes the next ones within WCAP - M, at most kResGroup;
    // every workgroup of this (item, antenna) derives the same windows and takes every
    // gridDim.z-th of them
    for (int i = tid; i < n; i += kScT) {
      int rank = 0;
      for (int j = 0; j < n; j++) rank += (pos[j] < pos[i]) ? 1 : 0;
      sorted[rank] = pos[i];
    }
    __syncthreads();
    if (tid == 0) {
      int nw = 0, k = 0;
      while (k < n) {
        wstart[nw++] = k;
        const long long lo = sorted[k];
        int e = k + 1;
        while (e < n && e - k < kResGroup && sorted[e] - lo <= (long long)(WCAP - (int)a.M)) e++;
        k = e;
      }
      wstart[nw] = n;
      s_nw = nw;
    }
    __syncthreads();
    const int nw = s_nw;
    for (int w = (int)blockIdx.z; w < nw; w += (int)gridDim.z)
      resolve_window(a, hp->f, hp->w0, (int)s, sorted + wstart[w], wstart[w + 1] - wstart[w],
                     hp->wbits, tables, table_bytes, rl);
    __syncthreads();
  }
}

// hot items, stage 2: plateau rule on the corrected words, candidate, record, trigger
__global__ __launch_bounds__(kScT) void sc_finalize_kernel(ScArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t wb[kMaxStreams * kScIters * kScT];
  __shared__ uint16_t acond[kScIters][kScT];
  __shared__ long long run_ws[2][kScT / 64];
  __shared__ long long lo[kMaxStreams];
  __shared__ unsigned long long s_min;
  const uint32_t count = min(*a.hot_count, a.hot_cap);
  for (uint32_t h = blockIdx.x; h < count; h += gridDim.x) {
    const ScHot *hp = a.hot + h;
    const uint32_t n_done = hp->n_done;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(hp->wbits);
    uint32_t *dst = reinterpret_cast<uint32_t *>(wb);
    for (int i = threadIdx.x; i < (int)n_done * kScIters * kScT / 2; i += kScT) dst[i] = src[i];
    if (threadIdx.x < n_done) lo[threadIdx.x] = hp->lo[threadIdx.x];
    if (threadIdx.x == 0) s_min = ~0ull;
    __syncthreads();
    int par = 0;
    const int any = item_conditions(wb, acond, n_done, hp->w0, hp->c0, hp->cend,
                                    (int64_t)a.cp, run_ws, par);
    if (any) item_record(a, hp->f, hp->chunk, hp->w0, wb, acond, lo, s_min);
    __syncthreads();
  }
}

size_t sc_lds_bytes(uint32_t M, uint32_t N) {
  const int ring = (int)M + kScIt;
  return sizeof(float2) * (size_t)(ring + ((ring >> 5) << 1)) +
         sizeof(uint16_t) * (size_t)N * kScIters * kScT;
}

void launch_sc(const ScArgs &a, uint32_t n_frames, uint32_t n_cu, hipStream_t s) {
  const size_t shm = sc_lds_bytes(a.M, a.N);
  static size_t set_shm = 0;
  static int per_cu = 0;
  if (shm != set_shm) {
    (void)hipFuncSetAttribute((const void *)sc_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)shm);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sc_kernel, kScT, shm) !=
            hipSuccess || per_cu < 1)
      per_cu = 1;
    set_shm = shm;
  }
  const uint64_t total = (a.chunk_hi - a.chunk_lo) * (uint64_t)n_frames;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(total, (uint64_t)n_cu * per_cu);
  if (grid) hipLaunchKernelGGL(sc_kernel, dim3(grid), dim3(kScT), shm, s, a, n_frames);
  if (a.prof) fprintf(stderr, "sc grid %u (per_cu %d, n_cu %u, lds %zu)\n", grid, per_cu, n_cu, shm);
}

size_t sc_table_bytes(uint32_t M) {
  const int ring = (int)M + kScIt;
  return sizeof(float2) * (size_t)(ring + ((ring >> 5) << 1));
}

void launch_sc_hot(const ScArgs &a, hipStream_t s) {
  if (!a.hot || !a.hot_cap) return;
  const size_t shm = sc_table_bytes(a.M);
  static size_t set_shm = 0;
  if (shm != set_shm) {
    (void)hipFuncSetAttribute((const void *)sc_resolve_kernel,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    set_shm = shm;
  }
  const uint32_t gx = std::min<uint32_t>(a.hot_cap, 256);
  static const int diag = [] { const char *e = getenv("RMIMO_SC_DIAG"); return e ? atoi(e) : 0; }();
  ScArgs ad = a;
  if (diag & 4) ad.hot_cap = 0;      // diagnostics: same grid, every workgroup exits at once
  // (item slot, antenna, window slot): the windows of one antenna in parallel
  const uint32_t gxr = std::min<uint32_t>(a.hot_cap, 64);
  if (!(diag & 1))
    hipLaunchKernelGGL(sc_resolve_kernel, dim3(gxr, a.N, kResWin), dim3(kScT), shm, s, ad);
  if (!(diag & 2)) hipLaunchKernelGGL(sc_finalize_kernel, dim3(gx), dim3(kScT), 0, s, a);
}

void launch_sc_finalize(const ScArgs &a, hipStream_t s) {
  if (a.hot && a.hot_cap)
    hipLaunchKernelGGL(sc_finalize_kernel, dim3(std::min<uint32_t>(a.hot_cap, 256)), dim3(kScT), 0,
                       s, a);
}

}  // namespace mimo
