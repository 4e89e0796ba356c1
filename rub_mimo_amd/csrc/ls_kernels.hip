// rub_mimo_amd/csrc/ls_kernels.hip -- LS channel estimate + training-residual noise variance
// (framing.cc:797-824) on gfx950, the forms that sum stored terms:
//   ls_combine_q_kernel             : from the terms the fused search stored (est_kernels.hip)
//   ls_kernel + ls_combine_kernel   : the unfused two-stage form (any M)
// The default form, ls_window_kernel, transforms the code windows on the register plan the
// fused search uses and is compiled with it (est_kernels.hip says why).
#include "est_common.hpp"
#include "fft.hpp"
#include "kernels.hpp"

namespace mimo {

// one thread per (frame, subcarrier, rx-tx pair): the codes' X/S1 of lsq in code order, G and
// this block's share of the residual variance (as ls_combine_kernel)
__global__ __launch_bounds__(256) void ls_combine_q_kernel(LsArgs a) {
  __shared__ double red[4];
  __shared__ double s_nu;
  __shared__ double2 s_rot[kLsRotCodes];
  const uint32_t rt = blockIdx.y, f = blockIdx.z;
  const FrameInfo &I = a.info[f];
  if (I.status != 0) return;
  const uint32_t M = a.M, N = a.N;
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  const uint32_t r_ = rt / N, t_ = rt % N;
  // opt-in CFO: the residual's phase at each code's window (window-relative, about the frame's
  // base), as the data region is derotated (cfo_kernels.hip stage 2) -- uniform over the
  // workgroup, so tabled once per code instead of per subcarrier
  const bool rot_tab = a.cfo_part && a.nac <= (uint32_t)kLsRotCodes;
  if (a.cfo_part) {
    if (threadIdx.x == 0) {
      s_nu = cfo_stage_eps(a.cfo_part, f, 2) / (double)M;
      if (blockIdx.x == 0 && rt == 0)   // the frame's total estimate (stage 1 + stage 2)
      {
        const double eps = cfo_stage_eps(a.cfo_part, f, 1) + s_nu * M;
        const_cast<FrameInfo &>(I).cfo_eps = (float)eps;
        const_cast<FrameInfo &>(I).cfo_E = cfo_fixed_freq(eps, M);
      }
    }
    __syncthreads();
    if (rot_tab) {
      for (uint32_t c = threadIdx.x; c < a.nac; c += 256) {
        const unsigned long long key = a.keys[((uint64_t)f * N + r_) * a.n_slots + 1 + c * N + t_];
        const double w = (double)key_index(key) + 0.5 * (double)M;
        double ph = -2.0 * s_nu * w;
        ph -= 2.0 * rint(ph * 0.5);
        double sn, cs;
        sincospi(ph, &sn, &cs);
        s_rot[c] = make_double2(cs, sn);
      }
      __syncthreads();
    }
  }
  double nv = 0.0;
  if (k < M) {
    const bool occ = a.occ_index[k] >= 0;
    const float2 *q = a.lsq + ((uint64_t)f * N * N + rt) * a.nac * M + k;
    double sr = 0.0, si = 0.0, s2 = 0.0;
    const double nu = a.cfo_part ? s_nu : 0.0;
    // the codes' terms in batches of CB loads in flight (one latency per batch instead of per
    // code), summed in code order as before
    constexpr uint32_t CB = 8;
    for (uint32_t c0 = 0; c0 < a.nac; c0 += CB) {
      float2 vb[CB];
#pragma unroll
      for (uint32_t j = 0; j < CB; j++) {   // clamped: every load unconditional; read once
        const v2f t = __builtin_nontemporal_load(reinterpret_cast<const v2f *>(q) + (uint64_t)min(c0 + j, a.nac - 1) * M);
        vb[j] = make_float2(t.x, t.y);
      }
#pragma unroll
      for (uint32_t j = 0; j < CB; j++) {
        const uint32_t c = c0 + j;
        if (c >= a.nac) break;
        float2 v = vb[j];
        if (a.cfo_part) {
          double sn, cs;
          if (rot_tab) {
            cs = s_rot[c].x;
            sn = s_rot[c].y;
          } else {   // (more codes than the table holds)
            const unsigned long long key =
                a.keys[((uint64_t)f * N + r_) * a.n_slots + 1 + c * N + t_];
            const double w = (double)key_index(key) + 0.5 * (double)M;
            double ph = -2.0 * nu * w;
            ph -= 2.0 * rint(ph * 0.5);
            sincospi(ph, &sn, &cs);
          }
          v = make_float2((float)(v.x * cs - v.y * sn), (float)(v.x * sn + v.y * cs));
        }
        sr += (double)v.x;
        si += (double)v.y;
        s2 += (double)v.x * v.x + (double)v.y * v.y;
      }
    }
    const uint32_t r = rt / N, t = rt % N;
    const double bias = (a.keep_bias && r == t) ? 1.0 : 0.0;
    a.G[(((uint64_t)f * M + k) * N + r) * N + t] =
        occ ? make_float2((float)((bias + sr) * a.scale), (float)(si * a.scale))
            : make_float2(0.0f, 0.0f);
    if (occ) nv = s2 - (sr * sr + si * si) / (double)a.nac;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) nv += __shfl_xor(nv, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = nv;
  __syncthreads();
  if (threadIdx.x == 0)
    a.nv_part[(uint64_t)f * a.n_nvp + (uint64_t)rt * gridDim.x + blockIdx.x] =
        red[0] + red[1] + red[2] + red[3];
}

// ------------------------------------------------------------------------------------
// LS estimate, two stages. ls_kernel: one workgroup per (frame, rx, tx, code group) FFTs the
// group's CB access codes as received on rx (the window at the search's corr index) and
// writes the group's per-subcarrier sums of X/S1 (S1 = +-1, framing.cc:811) and |X/S1|^2 in
// fp64. ls_combine_kernel: per (frame, subcarrier) the groups are summed in fixed order into
// G = (I + sum) * dft_normalizer / nac (framing.cc:809-824, identity bias from :309-311) and
// the training-residual variance sum |v - mean|^2 for the MMSE noise estimate.
template <int LOG2M, int T, int CB>
__global__ __launch_bounds__(T) void ls_kernel(LsArgs a) {
  constexpr int M = 1 << LOG2M, PB = lds_padded_len(M), PER = M / T;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  const uint32_t f = blockIdx.y;
  const FrameInfo &I = a.info[f];
  if (I.status != 0) return;
  const uint32_t P = a.n_groups;
  const uint32_t rt = blockIdx.x / P, grp = blockIdx.x % P;
  const uint32_t r = rt / a.N, t = rt % a.N;
  const int tid = threadIdx.x;
  const float2 *__restrict__ x = a.iq + ((uint64_t)I.cap * a.N + r) * a.stride;
  const int64_t L = (int64_t)a.frame_len;
  const uint32_t c0 = grp * CB;
  const uint32_t nb = min((uint32_t)CB, a.nac - c0);
  // every code's window start first, then all 16-byte loads in flight together, then the LDS
  // writes (a load -> ds_write loop waits out one memory latency per iteration)
  constexpr int P2 = (M / 2 + T - 1) / T;        // 16-byte pairs per thread per code
  int64_t abs0[CB];
  bool fast[CB];
#pragma unroll
  for (int b = 0; b < CB; b++) {
    abs0[b] = 0;
    if (b < (int)nb) {
      const uint32_t ac = (c0 + b) * a.N + t;
      abs0[b] = I.base + key_index(a.keys[((uint64_t)f * a.N + r) * a.n_slots + 1 + ac]);
    }
    fast[b] = b < (int)nb && abs0[b] >= 0 && abs0[b] + M <= L && (abs0[b] & 1) == 0;
  }
  float4 stg[CB][P2];
#pragma unroll
  for (int b = 0; b < CB; b++) {
    const float4 *x4 = reinterpret_cast<const float4 *>(x + (fast[b] ? abs0[b] : 0));
#pragma unroll
    for (int u = 0; u < P2; u++) {
      const int i = tid + u * T;
      stg[b][u] = (fast[b] && i < M / 2) ? x4[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
  }
#pragma unroll
  for (int b = 0; b < CB; b++) {
    if (fast[b]) {                   // 16-byte loads of two samples
#pragma unroll
      for (int u = 0; u < P2; u++) {
        const int i = tid + u * T;
        if (i < M / 2) *reinterpret_cast<float4 *>(lds + b * PB + lds_pad(2 * i)) = stg[b][u];
      }
    } else {
      for (int i = tid; i < M; i += T) {
        const int64_t n = abs0[b] + i;
        lds[b * PB + lds_pad(i)] =
            (b < (int)nb && n >= 0 && n < L) ? x[n] : make_float2(0.0f, 0.0f);
      }
    }
  }
  __syncthreads();
  fft_lds<LOG2M, T, CB, false>(lds, a.tw);
  double *pp = a.part + (((uint64_t)f * a.N * a.N + rt) * P + grp) * 3 * M;
#pragma unroll
  for (int q = 0; q < PER; q++) {
    const int k = tid + q * T;
    double sr = 0.0, si = 0.0, s2 = 0.0;
    for (int b = 0; b < (int)nb; b++) {
      const int sg = a.s1sign[((size_t)t * a.nac + c0 + b) * M + k];
      if (sg == 0) continue;                     // null subcarrier
      const float2 X = lds[b * PB + lds_pad(k)];
      const float2 v = (sg > 0) ? X : cneg(X);   // X / S1
      sr += (double)v.x;
      si += (double)v.y;
      s2 += (double)v.x * v.x + (double)v.y * v.y;
    }
    pp[k] = sr;
    pp[M + k] = si;
    pp[2 * M + k] = s2;
  }
}

// one thread per (frame, subcarrier, rx-tx pair): the code groups in fixed order, G, and this
// block's share of the residual variance (nv_part[f][rt][block], summed in order by weights)
__global__ __launch_bounds__(256) void ls_combine_kernel(LsArgs a) {
  __shared__ double red[4];
  const uint32_t rt = blockIdx.y, f = blockIdx.z;
  const FrameInfo &I = a.info[f];
  if (I.status != 0) return;
  const uint32_t M = a.M, N = a.N, P = a.n_groups;
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  double nv = 0.0;
  if (k < M) {
    const bool occ = a.occ_index[k] >= 0;
    const double *pp = a.part + ((uint64_t)f * N * N + rt) * P * 3 * M;
    double sr = 0.0, si = 0.0, s2 = 0.0;
    for (uint32_t g = 0; g < P; g++) {
      sr += pp[(uint64_t)g * 3 * M + k];
      si += pp[(uint64_t)g * 3 * M + M + k];
      s2 += pp[(uint64_t)g * 3 * M + 2 * M + k];
    }
    const uint32_t r = rt / N, t = rt % N;
    const double bias = (a.keep_bias && r == t) ? 1.0 : 0.0;
    a.G[(((uint64_t)f * M + k) * N + r) * N + t] =
        occ ? make_float2((float)((bias + sr) * a.scale), (float)(si * a.scale))
            : make_float2(0.0f, 0.0f);
    if (occ) nv = s2 - (sr * sr + si * si) / (double)a.nac;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) nv += __shfl_xor(nv, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = nv;
  __syncthreads();
  if (threadIdx.x == 0)
    a.nv_part[(uint64_t)f * a.n_nvp + (uint64_t)rt * gridDim.x + blockIdx.x] =
        red[0] + red[1] + red[2] + red[3];
}

void launch_ls_combine_q(const LsArgs &a, uint32_t n_frames, hipStream_t s) {
  hipLaunchKernelGGL(ls_combine_q_kernel, dim3((a.M + 255) / 256, a.N * a.N, n_frames), dim3(256),
                     0, s, a);
}

template <int LOG2M>
static void ls_dispatch(const LsArgs &a, int log2M, uint32_t nf, hipStream_t s) {
  if constexpr (LOG2M <= 12) {
    if (log2M == LOG2M) {
      constexpr int M = 1 << LOG2M;
      constexpr int T = M < 256 ? M : 256;
      constexpr int CB = kLsCodesPerGroup;
      const size_t shm = sizeof(float2) * lds_padded_len(M) * CB;
      (void)hipFuncSetAttribute((const void *)ls_kernel<LOG2M, T, CB>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
      hipLaunchKernelGGL((ls_kernel<LOG2M, T, CB>), dim3(a.N * a.N * a.n_groups, nf), dim3(T),
                         shm, s, a);
      hipLaunchKernelGGL(ls_combine_kernel, dim3((a.M + 255) / 256, a.N * a.N, nf), dim3(256),
                         0, s, a);
      return;
    }
    ls_dispatch<LOG2M + 1>(a, log2M, nf, s);
  }
}

void launch_ls(const LsArgs &a, int log2M, uint32_t n_frames, hipStream_t s) {
  ls_dispatch<6>(a, log2M, n_frames, s);
}

}  // namespace mimo
