// rub_mimo_amd/csrc/llr.hpp -- the max-log LLR arithmetic shared by the soft demapper
// (soft_kernels.hip) and the soft-output SIC pass (sic_kernels.hip). Both files are compiled
// with -ffp-contract=off: every output format then computes the same fp32 LLR, so the int8
// output is exactly the rounded and clamped fp32 output.
#pragma once

#include "common.hpp"

namespace mimo {

// Max-log LLRs of one dimension (x = Re y or Im y) of a square Gray QAM with L = 2^B levels
// l_m = (2 m - (L - 1)) scale: out[i] = (min_{bit_i(gray m) = 1} (x - l_m)^2 -
// min_{bit_i(gray m) = 0} (x - l_m)^2) k, bit 0 the most significant of gray(m); k =
// llr_scale / nu. Everything is unrolled: the distances and minima stay in registers, no
// tables and no divergence. A NaN (a NaN x, or inf - inf) gives 0.
template <int B>
MIMO_DEV void llr_dim(float x, float scale, float k, float *out) {
  constexpr int L = 1 << B;
  // t[] holds the minima over aligned units of 2^p levels, p = 0 first. Gray bit p of level m
  // is m_p ^ m_(p+1): over the units of 2^p levels it reads 0 1 1 0 0 1 1 0 ..., so the two
  // minima of output B-1-p are taken over the units u with u mod 4 in {1, 2} and in {0, 3};
  // the most significant bit splits the levels in halves. The same minima as a loop over
  // every (level, bit), in half the operations.
  float t[L];
#pragma unroll
  for (int m = 0; m < L; m++) {
    const float d = x - (float)(2 * m - (L - 1)) * scale;
    t[m] = d * d;
  }
#pragma unroll
  for (int p = 0; p < B; p++) {
    const int n = L >> p;   // units
    float m0 = t[0], m1 = t[1];
    if (p < B - 1) {
#pragma unroll
      for (int u = 2; u < n; u++) {
        if ((u & 1) ^ ((u >> 1) & 1)) m1 = fminf(m1, t[u]);
        else m0 = fminf(m0, t[u]);
      }
#pragma unroll
      for (int u = 0; u < n / 2; u++) t[u] = fminf(t[2 * u], t[2 * u + 1]);
    }
    const float v = (m1 - m0) * k;
    out[B - 1 - p] = (v == v) ? v : 0.0f;
  }
}

// MIMO_LLR_I8 of one value and of four: clamp(rintf(v), -127, 127) as a byte
MIMO_DEV uint32_t llr_q8(float v) {
  return (uint32_t)(int)fminf(fmaxf(rintf(v), -127.0f), 127.0f) & 0xFFu;
}
MIMO_DEV uint32_t llr_pack4(const float *v) {
  return llr_q8(v[0]) | (llr_q8(v[1]) << 8) | (llr_q8(v[2]) << 16) | (llr_q8(v[3]) << 24);
}

}  // namespace mimo
