// rub_mimo_amd/csrc/soft_kernels.hip -- soft-output demapping on gfx950: the per-carrier
// post-detection mean-square error and max-log LLRs of the equalised symbols of a batch
// (mimo_rx_soft_demap, DESIGN.md "Soft output").
//
// No reference counterpart: main.cc only ever slices a symbol to its hard index. A separate,
// opt-in pass over the decode's d_out_sym; nothing here is launched by the batch itself.
//
// Compiled with -ffp-contract=off: both output formats then compute the same fp32 LLR, so the
// int8 output is exactly the rounded and clamped fp32 output.
#pragma clang fp contract(off)

#include "fft.hpp"
#include "kernels.hpp"
#include "llr.hpp"

namespace mimo {

constexpr int kSoftT = 256;

// ------------------------------------------------------------------------------------
// nu[f][t][j] = g^2 s2 sum_r |W[t][r]|^2 + sum_u |g sum_r W[t][r] G[r][u] - delta_tu|^2: the
// predicted E|y_t - s_t|^2 of the decode's output on occupied carrier j (subcarrier k), noise
// enhancement plus residual inter-stream interference and bias. One thread per (t, k): it holds
// row t of W (N values) and streams G's columns, so nothing spills at 8x8. W is [t][r][k]
// (coalesced over k); a frame's G is read N times, from L2.
template <int N>
__global__ __launch_bounds__(kSoftT) void mse_kernel(MseArgs a) {
  const uint32_t f = blockIdx.y;
  const uint32_t e = blockIdx.x * kSoftT + threadIdx.x;
  if (e >= (uint32_t)N * a.M) return;
  const uint32_t t = e / a.M, k = e - t * a.M;
  const int j = a.occ_index[k];
  if (j < 0) return;
  float *out = a.nu + ((uint64_t)f * N + t) * a.M_occ + j;
  const FrameInfo &I = a.info[f];
  if (I.status != 0) {
    *out = 0.0f;
    return;
  }
  const float g = a.gain[(uint64_t)f * a.M + k];
  const float2 *__restrict__ Wf = a.W + ((uint64_t)f * N + t) * N * a.M + k;
  const float2 *__restrict__ Gk = a.G + ((uint64_t)f * a.M + k) * N * N;
  float2 w[N];
  float w2 = 0.0f;
#pragma unroll
  for (int r = 0; r < N; r++) {
    w[r] = Wf[(uint64_t)r * a.M];
    w2 += cabs2(w[r]);
  }
  float isi = 0.0f;
#pragma unroll
  for (int u = 0; u < N; u++) {
    float2 c = make_float2(0.0f, 0.0f);
#pragma unroll
    for (int r = 0; r < N; r++) c = cadd(c, cmul(w[r], Gk[r * N + u]));
    c = cscale(c, g);
    if (u == (int)t) c.x -= 1.0f;
    isi += cabs2(c);
  }
  *out = g * g * I.noise_var * w2 + isi;
}

template <int N>
static void mse_launch(const MseArgs &a, uint32_t nf, hipStream_t s) {
  const uint32_t n = (uint32_t)N * a.M;
  hipLaunchKernelGGL((mse_kernel<N>), dim3((n + kSoftT - 1) / kSoftT, nf), dim3(kSoftT), 0, s, a);
}

bool launch_mse(const MseArgs &a, uint32_t n_frames, hipStream_t s) {
  switch (a.N) {
    case 1: mse_launch<1>(a, n_frames, s); return true;
    case 2: mse_launch<2>(a, n_frames, s); return true;
    case 3: mse_launch<3>(a, n_frames, s); return true;
    case 4: mse_launch<4>(a, n_frames, s); return true;
    case 8: mse_launch<8>(a, n_frames, s); return true;
    default: return false;
  }
}

// ------------------------------------------------------------------------------------
// The demapper: the LLR arithmetic (llr_dim, llr_pack4) is llr.hpp's, shared with the SIC pass.
//
// symbol pairs per thread (16-byte loads in flight per thread); the fp32 output image of a
// workgroup is 4x the int8 one, so it takes half the pairs to stay within 32 KiB of LDS
template <bool F32>
constexpr int soft_pairs() { return F32 ? 2 : 4; }
constexpr uint32_t kSoftErased = 0xFFFFFFFFu;

// where flat row `row` of d_sym lies: its nu row f N + t, or kSoftErased (a frame that did not
// sync, a symbol the decode did not write, a row past the batch)
MIMO_DEV uint32_t soft_row(const SoftArgs &a, uint32_t row) {
  if (row >= a.rows) return kSoftErased;
  const uint32_t ns = a.N * a.max_out;
  const uint32_t f = row / ns, rem = row - f * ns;
  uint32_t t, s;
  if (a.symbol_major) {
    s = rem / a.N;
    t = rem - s * a.N;
  } else {
    t = rem / a.max_out;
    s = rem - t * a.max_out;
  }
  const FrameInfo &I = a.info[f];
  const uint32_t n_out = (I.status == 0) ? min(I.n_sym, a.max_out) : 0u;
  return s < n_out ? f * a.N + t : kSoftErased;
}

// d_sym and d_llr as flat arrays (both layouts are contiguous). A workgroup takes BLK
// consecutive symbols: thread tid loads the pairs tid, tid + kSoftT, ... (16-byte loads, a wave
// reads 1 KiB contiguously, all issued before anything waits), looks each symbol's nu up
// through the workgroup's row table, and puts the pair's 2 x 2B LLRs into an LDS image of the
// workgroup's output; the image then leaves as contiguous 16-byte stores. (A thread storing
// its own 4 x 2B values directly writes 8..96 bytes at that stride per lane: measured 2.9 TB/s
// int8 and 1.0 TB/s fp32 on the C3 batch.) No byte or short stores except in the last 16 bytes
// of a batch whose size is no multiple.
template <int B, bool F32>
__global__ __launch_bounds__(kSoftT) void soft_demap_kernel(SoftArgs a) {
  constexpr int PAIRS = soft_pairs<F32>();
  constexpr int BLK = kSoftT * PAIRS * 2;    // symbols per workgroup
  constexpr int WPP = F32 ? 4 * B : B;       // output words per symbol pair
  constexpr int BPS = F32 ? 8 * B : 2 * B;   // output bytes per symbol
  typedef uint32_t v4u __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) uint32_t stage[BLK / 2 * WPP];
  __shared__ uint32_t rowinfo[BLK + 1];
  const uint32_t tid = threadIdx.x;
  const uint64_t base = (uint64_t)blockIdx.x * BLK;
  const uint32_t nblk = (a.total - base >= (uint64_t)BLK) ? (uint32_t)BLK
                                                         : (uint32_t)(a.total - base);
  float2 y[PAIRS][2];
#pragma unroll
  for (int q = 0; q < PAIRS; q++) {
    const uint32_t s0 = 2 * (tid + q * kSoftT);
    y[q][0] = y[q][1] = make_float2(0.0f, 0.0f);
    if (s0 + 2 <= nblk) {
      const v4f u = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(a.sym + base + s0));
      y[q][0] = make_float2(u.x, u.y);
      y[q][1] = make_float2(u.z, u.w);
    } else if (s0 < nblk) {
      y[q][0] = a.sym[base + s0];
    }
  }
  const uint32_t rowb = (uint32_t)(base / a.M_occ);
  const uint32_t jb = (uint32_t)(base - (uint64_t)rowb * a.M_occ);
  const uint32_t nrows = (jb + nblk - 1) / a.M_occ + 1;   // <= BLK + 1
  for (uint32_t r = tid; r < nrows; r += kSoftT) rowinfo[r] = soft_row(a, rowb + r);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < PAIRS; q++) {
    const uint32_t pi = tid + q * kSoftT, s0 = 2 * pi;
    float llr[4 * B];
#pragma unroll
    for (int e = 0; e < 2; e++) {
      // (jj < M_occ + BLK, so the 2^40 reciprocal gives the exact quotient)
      const uint32_t jj = jb + s0 + e;
      const uint32_t dq = (uint32_t)(((uint64_t)jj * a.mocc_recip) >> 40);
      const uint32_t j = jj - dq * a.M_occ;
      const uint32_t ri = (s0 + e < nblk) ? rowinfo[dq] : kSoftErased;
      if (ri != kSoftErased) {
        const float k = a.llr_scale / fmaxf(a.nu[(uint64_t)ri * a.M_occ + j], 1e-30f);
        llr_dim<B>(y[q][e].x, a.qam_scale, k, llr + e * 2 * B);
        llr_dim<B>(y[q][e].y, a.qam_scale, k, llr + e * 2 * B + B);
      } else {
#pragma unroll
        for (int i = 0; i < 2 * B; i++) llr[e * 2 * B + i] = 0.0f;
      }
    }
#pragma unroll
    for (int c = 0; c < WPP; c++) {
      if constexpr (F32) stage[pi * WPP + c] = __float_as_uint(llr[c]);
      else stage[pi * WPP + c] = llr_pack4(llr + 4 * c);
    }
  }
  __syncthreads();
  const uint32_t nbytes = nblk * BPS;
  char *ob = reinterpret_cast<char *>(a.llr) + base * BPS;   // 16-byte aligned
  for (uint32_t c = tid; c * 16 < nbytes; c += kSoftT) {
    if (c * 16 + 16 <= nbytes) {
      const v4u v = *reinterpret_cast<const v4u *>(stage + 4 * c);
      __builtin_nontemporal_store(v, reinterpret_cast<v4u *>(ob + 16 * c));
    } else if (F32) {
      for (uint32_t w = 4 * c; w * 4 < nbytes; w++) reinterpret_cast<uint32_t *>(ob)[w] = stage[w];
    } else {
      for (uint32_t bb = 16 * c; bb < nbytes; bb++)
        ob[bb] = reinterpret_cast<const char *>(stage)[bb];
    }
  }
}

template <int B, bool F32>
static bool soft_launch(const SoftArgs &a, hipStream_t s) {
  constexpr uint64_t blk = (uint64_t)kSoftT * soft_pairs<F32>() * 2;
  const uint64_t grid = (a.total + blk - 1) / blk;
  if (grid >= 0x7FFFFFFFull) return false;
  hipLaunchKernelGGL((soft_demap_kernel<B, F32>), dim3((uint32_t)grid), dim3(kSoftT), 0, s, a);
  return true;
}

bool launch_soft_demap(SoftArgs a, hipStream_t s) {
  if (a.total == 0) return true;
  if (a.M_occ == 0) return false;
  a.mocc_recip = ((1ull << 40) + a.M_occ - 1) / a.M_occ;
  switch (a.bits) {
    case 1: return a.f32 ? soft_launch<1, true>(a, s) : soft_launch<1, false>(a, s);
    case 2: return a.f32 ? soft_launch<2, true>(a, s) : soft_launch<2, false>(a, s);
    case 3: return a.f32 ? soft_launch<3, true>(a, s) : soft_launch<3, false>(a, s);
    case 4: return a.f32 ? soft_launch<4, true>(a, s) : soft_launch<4, false>(a, s);
    default: return false;
  }
}

}  // namespace mimo
