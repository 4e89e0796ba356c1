// rub_mimo_amd/csrc/codes_kernels.hip -- code tables on gfx950:
//   codes_kernel   : S0/S1 time-domain codes and their zero-padded F-point spectra
//                    (and the spectra in the wave-local search's order)
#include "est_common.hpp"
#include "fft.hpp"
#include "kernels.hpp"

namespace mimo {

// ------------------------------------------------------------------------------------
template <int LOG2M, int LOG2F>
__global__ __launch_bounds__(kEstT) void codes_kernel(CodesArgs a) {
  constexpr int M = 1 << LOG2M, F = 1 << LOG2F;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  float2 *buf = lds;
  const int slot = blockIdx.x, tid = threadIdx.x;
  // frequency-domain code on the first M entries
  for (int i = tid; i < M; i += kEstT) {
    float v = 0.0f;
    if (a.p[i] != 0) {
      if (slot == 0) {
        if ((i & 1) == 0) v = (a.s0_bits[i] & 1) ? 1.0f : -1.0f;  // framing.cc:1077-1089
      } else {
        const int ac = slot - 1, c = ac / a.N, t = ac % a.N;
        v = (a.s1_bits[((size_t)t * a.nac + c) * M + i] & 1) ? 1.0f : -1.0f;  // :1243-1248
      }
    }
    buf[lds_pad(i)] = make_float2(v, 0.0f);
  }
  __syncthreads();
  fft_lds<LOG2M, kEstT, 1, true>(buf, a.tw);
  const float dn = (slot == 0) ? a.dn_s0 : a.dn_s1;
  for (int i = tid; i < M; i += kEstT) {
    float2 v = buf[lds_pad(i)];
    v = make_float2(v.x * dn, v.y * dn);
    a.code_time[(size_t)slot * M + i] = v;
    buf[lds_pad(i)] = v;
  }
  if (a.codespec == nullptr) return;
  __syncthreads();
  // zero-pad to F (in place: move is safe because M <= F/2 and we only clear [M, F))
  for (int i = M + tid; i < F; i += kEstT) buf[lds_pad(i)] = make_float2(0.0f, 0.0f);
  __syncthreads();
  fft_lds<LOG2F, kEstT, 1, false>(buf, a.tw);
  for (int i = tid; i < F; i += kEstT) a.codespec[(size_t)slot * F + i] = buf[lds_pad(i)];
  if constexpr (F >= 1024) {
    // the wave-local search's order: bin B k + q at q * 1024 + k (B = F / 1024)
    constexpr int B = F / 1024;
    if (a.codespec_w)
      for (int i = tid; i < F; i += kEstT)
        a.codespec_w[(size_t)slot * F + (i % B) * 1024 + i / B] = buf[lds_pad(i)];
  }
}

// ------------------------------------------------------------------------------------
template <int LOG2M, int LOG2F>
static void codes_dispatch_f(const CodesArgs &a, int log2F, hipStream_t s) {
  if constexpr (LOG2F <= 14) {
    if (log2F == LOG2F) {
      constexpr int F = 1 << LOG2F;
      const size_t shm = sizeof(float2) * lds_padded_len(F);
      (void)hipFuncSetAttribute((const void *)codes_kernel<LOG2M, LOG2F>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
      hipLaunchKernelGGL((codes_kernel<LOG2M, LOG2F>), dim3(a.n_slots), dim3(kEstT), shm, s, a);
      return;
    }
    codes_dispatch_f<LOG2M, LOG2F + 1>(a, log2F, s);
  }
}

template <int LOG2M>
static void codes_dispatch(const CodesArgs &a, int log2M, int log2F, hipStream_t s) {
  if constexpr (LOG2M <= 12) {
    if (log2M == LOG2M) { codes_dispatch_f<LOG2M, LOG2M>(a, log2F, s); return; }
    codes_dispatch<LOG2M + 1>(a, log2M, log2F, s);
  }
}

void launch_codes(const CodesArgs &a, int log2M, int log2F, hipStream_t s) {
  codes_dispatch<6>(a, log2M, log2F, s);
}

}  // namespace mimo
