// rub_mimo_amd/csrc/pic_kernels.hip -- soft-input MMSE-PIC detection on gfx950
// (mimo_rx_pic_soft, DESIGN.md "Soft-input MMSE-PIC"): the per-carrier Q = G^H G of a batch's
// frames, and the pass that turns a-priori LLRs into expected symbols and variances, cancels
// every other stream's expected symbol, filters with the MMSE filter of the residual covariance
// (one N x N solve per carrier and symbol) and writes extrinsic LLRs.
//
// No reference counterpart: framing.cc's detectors are linear and take no priors. A separate,
// opt-in pass over the decode's d_out_sym; nothing here is launched by the batch itself.
//
// Compiled with -ffp-contract=off like sic_kernels.hip: the slicer is the decode's bit for bit
// and both LLR formats compute the same fp32 value. The sums that want a fused multiply-add
// spell it out.
#pragma clang fp contract(off)

#include <type_traits>

#include "sic_pass.hpp"

namespace mimo {

// ------------------------------------------------------------------------------------
// Tables. One thread per (frame, subcarrier): Q = G^H G in fp64, stored as fp32 in the
// Hermitian-packed form (N diagonal values, then Re and Im of the N (N - 1) / 2 entries above
// the diagonal) at stride M_occ, like the SIC tables. ok = 0 erases the carrier in the pass.
constexpr int kPicTabT = 64;

template <int N>
__global__ __launch_bounds__(kPicTabT) void pic_tables_kernel(PicTableArgs a) {
  const uint32_t f = blockIdx.y;
  const uint32_t k = blockIdx.x * kPicTabT + threadIdx.x;
  if (k >= a.M) return;
  const int j = a.occ_index[k];
  if (j < 0) return;
  const uint64_t mo = a.M_occ;
  float *Qq = a.Q + (uint64_t)f * N * N * mo + j;
  const FrameInfo &I = a.info[f];
  bool ok = I.status == 0 && I.noise_var > 0.0f && isfinite(I.noise_var);
  float q[N * N];
#pragma unroll
  for (int e = 0; e < N * N; e++) q[e] = 0.0f;
  if (ok) {
    const float2 *g = a.G + ((uint64_t)f * a.M + k) * N * N;
    int row = N;
#pragma unroll
    for (int t = 0; t < N; t++)
#pragma unroll
      for (int u = t; u < N; u++) {
        double sr = 0.0, si = 0.0;
#pragma unroll
        for (int rr = 0; rr < N; rr++) {
          const double gar = g[rr * N + t].x, gai = g[rr * N + t].y;
          const double gbr = g[rr * N + u].x, gbi = g[rr * N + u].y;
          sr += gar * gbr + gai * gbi;
          si += gar * gbi - gai * gbr;
        }
        if (u == t) {
          q[t] = (float)sr;
          ok = ok && isfinite(q[t]);
        } else {
          q[row] = (float)sr;
          q[row + 1] = (float)si;
          ok = ok && isfinite(q[row]) && isfinite(q[row + 1]);
          row += 2;
        }
      }
  }
#pragma unroll
  for (int e = 0; e < N * N; e++) Qq[(uint64_t)e * mo] = ok ? q[e] : 0.0f;
  a.ok[(uint64_t)f * mo + j] = ok ? 1 : 0;
}

template <int N>
static void pic_tables_launch(const PicTableArgs &a, uint32_t nf, hipStream_t s) {
  hipLaunchKernelGGL((pic_tables_kernel<N>), dim3((a.M + kPicTabT - 1) / kPicTabT, nf),
                     dim3(kPicTabT), 0, s, a);
}

bool launch_pic_tables(const PicTableArgs &a, uint32_t n_frames, hipStream_t s) {
  if (n_frames == 0) return true;
  if (n_frames > 65535u) return false;
  switch (a.N) {
    case 1: pic_tables_launch<1>(a, n_frames, s); return true;
    case 2: pic_tables_launch<2>(a, n_frames, s); return true;
    case 4: pic_tables_launch<4>(a, n_frames, s); return true;
    default: return false;
  }
}

// ------------------------------------------------------------------------------------
// The symbol pass, pic_pass_kernel<N, B, F32>, in the frame of sic_pass_kernel (sic_pass.hpp):
// a workgroup owns (frame, tile of kSicT adjacent carriers, kSicSB symbols), thread tid holds
// carrier j's Q (N^2 floats) and s2 in registers for all of them, an iteration takes SC
// symbols, z-hat leaves as 8-byte non-temporal stores, and the index image and the LLR image
// leave through LDS exactly as there. Unlike the SIC stages a symbol's streams keep their own
// rows: there is no detection order.
//
// The priors come in the way the LLRs go out. A lane's 2 B bytes at a 2 B-byte lane stride are
// the per-lane byte pattern the soft demapper paid for, so every (symbol, stream) row's
// contiguous [carrier][2 B] run is copied into an LDS image by 16-byte non-temporal loads (the
// image row holds the run behind its own misalignment, address mod 16, so an aligned chunk of
// d_prior is an aligned chunk of the image; the chunks at either end of a run come in 2-byte
// pieces, and nothing outside the run is read), and after a barrier every lane takes its own
// bytes from the image. Rows the decode did not write and frames with noise_var <= 0 are never
// read. A null d_prior runs the same arithmetic on zero bytes, so it is bitwise the zero buffer.
//
// Per symbol and lane: the moments of every stream from B exponentials per dimension
// (pic_moments), r = lam y + Q (y - sbar), A = Q diag(v) + s2 I, then one elimination of
// [A | r Q] without pivoting in fp32 (A is a column scaling of the Hermitian positive definite
// Q + s2 diag(v)^-1, and column scaling leaves the multipliers alone; the pivots are real up to
// rounding and only their real parts are used), back-substitution for A^-1 r and for the
// diagonal of A^-1 Q. Every array index is a compile-time constant after unrolling: no scratch.
// N = 1 has nothing to cancel and takes sbar = 0, v = 1 whatever the priors say, so that its
// output does not depend on them bit for bit.
template <int N, int B, bool F32>
constexpr int pic_sc() {
  // N = 4: two symbols per iteration keep the y of an iteration and one symbol's augmented
  // system in registers together
  const int sc = sic_soft_sc<N, B, F32>();
  return (N > 2 && sc > 2) ? 2 : sc;
}

MIMO_DEV uint64_t pic_row(const PicPassArgs &a, uint32_t f, uint32_t t, uint32_t s) {
  return a.symbol_major ? ((uint64_t)f * a.max_out + s) * a.N + t
                        : ((uint64_t)f * a.N + t) * a.max_out + s;
}

// A lane's 2 B prior bytes from the image as natural LLRs: lam[i] = (int8) byte i * ips. p is
// aligned as sic_llr_put's int8 pointer is.
template <int B>
MIMO_DEV void pic_prior_get(const uint8_t *p, float ips, float *lam) {
  uint64_t w = 0;
  if constexpr (B == 4) {
    const uint2 v = *reinterpret_cast<const uint2 *>(p);
    w = (uint64_t)v.x | ((uint64_t)v.y << 32);
  } else if constexpr (B == 2) {
    w = *reinterpret_cast<const uint32_t *>(p);
  } else {
#pragma unroll
    for (int i = 0; i < B; i++)
      w |= (uint64_t) reinterpret_cast<const uint16_t *>(p)[i] << (16 * i);
  }
#pragma unroll
  for (int i = 0; i < 2 * B; i++) lam[i] = (float)(int8_t)(uint8_t)(w >> (8 * i)) * ips;
}

// Mean and variance of one dimension under independent bit priors. The reflected Gray map
// factorises: with s_i = +-1 the bit signs (+1 = bit 0),
// x = -s_0 (2^(B-1) + s_1 (2^(B-2) + ... + s_(B-1))) scale, so with t_i = E s_i = tanh(lam_i / 2)
// and c_i = 1 - t_i^2 the mean m and the variance V of the bracket follow from the innermost
// outwards: from m = 1, V = 0, V <- V + c_(i+1) m^2, m <- w + t_(i+1) m, w = 2^(B-1-i); then
// mean = -t_0 m scale and variance = (V + c_0 m^2) scale^2. That is the recursion on the second
// moment M = V + m^2 (M <- w^2 + 2 w t m + M, variance = M scale^2 - mean^2) with the
// subtraction carried out on paper: every term is >= 0, so a small variance keeps its relative
// accuracy, which the filter needs when s2 is small (the second-moment form is off by
// 2^-23 absolute, 2e-3 of nu at 30 dB). With e = exp(-|lam|) <= 1, which cannot overflow,
// t = copysign((1 - e) / (1 + e), lam) and c = 4 e / (1 + e)^2: one v_exp_f32 and one v_rcp_f32
// per bit.
template <int B>
MIMO_DEV void pic_moments(const float *lam, float scale, float *mean, float *var) {
  float t[B], c[B];
#pragma unroll
  for (int i = 0; i < B; i++) {
    const float e = __builtin_amdgcn_exp2f(fabsf(lam[i]) * -1.44269504f);
    const float r = __builtin_amdgcn_rcpf(1.0f + e);
    t[i] = copysignf((1.0f - e) * r, lam[i]);
    c[i] = ((4.0f * e) * r) * r;
  }
  float m = 1.0f, V = 0.0f;
#pragma unroll
  for (int i = B - 2; i >= 0; i--) {
    const float w = (float)(1 << (B - 1 - i));
    V = V + c[i + 1] * (m * m);
    m = w + t[i + 1] * m;
  }
  *mean = -(t[0] * m) * scale;
  *var = (V + c[0] * (m * m)) * (scale * scale);
}

MIMO_DEV float2 pic_neg_scaled(v2f a, float s) { return make_float2(-(a.x * s), -(a.y * s)); }

// One symbol of one carrier: z-hat and nu of every stream. qd the diagonal of Q, qo the entries
// above it (row-major pairs t < u).
template <int N>
MIMO_DEV void pic_detect(const float *qd, const float2 *qo, float s2, float lam, const v2f *y,
                         const v2f *sb, const float *vv, v2f *z, float *nu) {
  float2 Qf[N][N];
#pragma unroll
  for (int t = 0; t < N; t++)
#pragma unroll
    for (int u = 0; u < N; u++) {
      if (u == t) Qf[t][u] = make_float2(qd[t], 0.0f);
      else if (t < u) Qf[t][u] = qo[t * N - t * (t + 1) / 2 + (u - t - 1)];
      else Qf[t][u] = cconj(qo[u * N - u * (u + 1) / 2 + (t - u - 1)]);
    }
  // r = lam y + Q (y - sbar); [A | r Q]
  v2f A[N][N], R[N], X[N][N], d[N], dr[N];
#pragma unroll
  for (int u = 0; u < N; u++) {
    d[u] = y[u] - sb[u];
    dr[u] = sic_rot(d[u]);
  }
#pragma unroll
  for (int t = 0; t < N; t++) {
    v2f acc = v2f{lam * y[t].x, lam * y[t].y};
#pragma unroll
    for (int u = 0; u < N; u++) acc = sic_mac(acc, Qf[t][u], d[u], dr[u]);
    R[t] = acc;
#pragma unroll
    for (int c = 0; c < N; c++) {
      A[t][c] = v2f{Qf[t][c].x * vv[c], Qf[t][c].y * vv[c]};
      X[t][c] = v2f{Qf[t][c].x, Qf[t][c].y};
    }
    A[t][t].x = A[t][t].x + s2;
  }
  float ip[N];
#pragma unroll
  for (int c = 0; c < N; c++) {
    ip[c] = __builtin_amdgcn_rcpf(A[c][c].x);
#pragma unroll
    for (int rr = c + 1; rr < N; rr++) {
      const float2 nf = pic_neg_scaled(A[rr][c], ip[c]);
#pragma unroll
      for (int k = c + 1; k < N; k++) A[rr][k] = sic_mac(A[rr][k], nf, A[c][k], sic_rot(A[c][k]));
      R[rr] = sic_mac(R[rr], nf, R[c], sic_rot(R[c]));
#pragma unroll
      for (int t = 0; t < N; t++) X[rr][t] = sic_mac(X[rr][t], nf, X[c][t], sic_rot(X[c][t]));
    }
  }
  // A^-1 r
  v2f x[N];
#pragma unroll
  for (int i = N - 1; i >= 0; i--) {
    v2f acc = R[i];
#pragma unroll
    for (int k = i + 1; k < N; k++)
      acc = sic_mac(acc, make_float2(-A[i][k].x, -A[i][k].y), x[k], sic_rot(x[k]));
    x[i] = acc * ip[i];
  }
  // mu_t = (A^-1 Q)[t][t]: column t of the right-hand side, solved down to component t
#pragma unroll
  for (int t = 0; t < N; t++) {
    v2f c[N];
#pragma unroll
    for (int i = N - 1; i >= t; i--) {
      v2f acc = X[i][t];
#pragma unroll
      for (int k = i + 1; k < N; k++)
        acc = sic_mac(acc, make_float2(-A[i][k].x, -A[i][k].y), c[k], sic_rot(c[k]));
      c[i] = acc * ip[i];
    }
    const float imu = __builtin_amdgcn_rcpf(c[t].x);
    z[t] = x[t] * imu + sb[t];
    nu[t] = imu - vv[t];
  }
}

template <int N, int B, bool F32>
__global__ __launch_bounds__(kSicT) void pic_pass_kernel(PicPassArgs a) {
  constexpr int SC = pic_sc<N, B, F32>();
  constexpr int NO = N * (N - 1) / 2;
  constexpr int SLOTS = kSicT / 4 + 1;   // dwords a row's kSicT index bytes can touch
  constexpr int BPS = sic_llr_bps<B, F32>();
  constexpr int RS = sic_llr_rs<B, F32>();
  constexpr int CH = RS / 16;            // 16-byte chunks a row's LLR bytes can touch
  constexpr int PBS = 2 * B;             // prior bytes per symbol
  constexpr int PRS = kSicT * PBS + 16;  // prior image row bytes
  constexpr int PCH = PRS / 16;
  typedef uint32_t v4u __attribute__((ext_vector_type(4)));
  typedef typename std::conditional<F32, uint32_t, uint16_t>::type edge_t;   // a row end's pieces
  __shared__ __attribute__((aligned(16))) uint8_t limg[SC * N * RS];
  __shared__ __attribute__((aligned(16))) uint8_t img[SC * N * kSicT];
  __shared__ __attribute__((aligned(16))) uint8_t pimg[N > 1 ? SC * N * PRS : 16];
  const uint32_t tid = threadIdx.x;
  const uint32_t f = blockIdx.z;
  const uint32_t j0 = blockIdx.x * kSicT, j = j0 + tid;
  const uint32_t s_lo = blockIdx.y * kSicSB;
  const uint32_t s_hi = min(s_lo + (uint32_t)kSicSB, a.max_out);
  const uint32_t nj = min((uint32_t)kSicT, a.M_occ - j0);
  const bool lane = j < a.M_occ;
  const FrameInfo &I = a.info[f];
  const float s2 = I.noise_var;
  // a frame with noise_var <= 0 is erased as a whole: A can be singular there
  const uint32_t n_out = (I.status == 0 && s2 > 0.0f) ? min(I.n_sym, a.max_out) : 0u;
  const float lam = a.mmse ? s2 : 0.0f;
  const uint64_t mo = a.M_occ;
  // rows of one frame slot: stream t, symbol s at t r_ts + s r_ss
  const uint32_t r_ts = a.symbol_major ? 1u : a.max_out, r_ss = a.symbol_major ? a.N : 1u;
  const uint64_t fbase = (uint64_t)f * a.N * a.max_out * mo + j;   // (frame, carrier) in elements
  // the addresses of (frame, tile) in d_llr and d_prior mod 2^32: the images need their low 4 bits
  const uint32_t lbase = (uint32_t)(uintptr_t)a.llr + (f * a.N * a.max_out * a.M_occ + j0) * BPS;
  const uint32_t pbase = (uint32_t)(uintptr_t)a.prior + (f * a.N * a.max_out * a.M_occ + j0) * PBS;
  const bool have_prior = N > 1 && a.prior != nullptr;   // (uniform)
  const float ips = 1.0f / a.prior_scale;

  // ---- phase 1, the table prologue: a lane without work gets Q = 0 and is erased
  float qd[N];
  float2 qo[NO > 0 ? NO : 1];
  const bool work = lane && s_lo < n_out;
  const bool good = work && a.ok[(uint64_t)f * mo + j] != 0;
  const float nanv = __builtin_nanf("");
  qo[0] = make_float2(0.0f, 0.0f);
#pragma unroll
  for (int t = 0; t < N; t++)
    qd[t] = good ? a.Q[((uint64_t)f * N * N + t) * mo + j] : 0.0f;
#pragma unroll
  for (int e = 0; e < NO; e++)
    qo[e] = good ? make_float2(a.Q[((uint64_t)f * N * N + N + 2 * e) * mo + j],
                               a.Q[((uint64_t)f * N * N + N + 2 * e + 1) * mo + j])
                 : make_float2(0.0f, 0.0f);

  for (uint32_t s0 = s_lo; s0 < s_hi; s0 += SC) {
    const uint32_t rows = min((uint32_t)SC, s_hi - s0) * N;
    v2f y[SC][N];
#pragma unroll
    for (int q = 0; q < SC; q++)
#pragma unroll
      for (int u = 0; u < N; u++) y[q][u] = v2f{0.0f, 0.0f};
    if (lane) {
#pragma unroll
      for (int q = 0; q < SC; q++) {
        if (s0 + q >= n_out) break;     // (uniform)
#pragma unroll
        for (int u = 0; u < N; u++)
          y[q][u] = __builtin_nontemporal_load(reinterpret_cast<const v2f *>(
              a.sym + fbase + ((uint64_t)u * r_ts + (uint64_t)(s0 + q) * r_ss) * mo));
      }
    }
    // ---- phase 2, the prior image: the mirror of the LLR drain
    if constexpr (N > 1) {
      if (have_prior) {
        const uint32_t nb = nj * PBS;   // a row's prior bytes in this tile
        for (uint32_t w = tid; w < rows * PCH; w += kSicT) {
          const uint32_t r = w / PCH, c = w - r * PCH;
          const uint32_t q = r / N, t = r - q * N;
          if (s0 + q >= n_out) continue;            // an erased row's priors are not read
          const uint8_t *src = reinterpret_cast<const uint8_t *>(a.prior) +
                               (pic_row(a, f, t, s0 + q) * mo + j0) * PBS;
          const uint32_t mis = (uint32_t)((uintptr_t)src & 15u);
          const uint8_t *al = src - mis;            // the aligned span: image byte b is al[b]
          uint8_t *dst = pimg + r * PRS;
          const uint32_t b0 = 16 * c;
          if (b0 >= mis && b0 + 16 <= mis + nb) {
            *reinterpret_cast<v4u *>(dst + b0) =
                __builtin_nontemporal_load(reinterpret_cast<const v4u *>(al + b0));
          } else {
            for (uint32_t bb = b0; bb < b0 + 16; bb += 2)
              if (bb >= mis && bb < mis + nb)
                *reinterpret_cast<uint16_t *>(dst + bb) = *reinterpret_cast<const uint16_t *>(al + bb);
          }
        }
        __syncthreads();
      }
    }
#pragma unroll
    for (int q = 0; q < SC; q++) {
      const uint32_t s = s0 + q;
      if (s >= s_hi || !lane) break;    // (s uniform; idle lanes' image bytes are never stored)
      // ---- phase 3, one symbol (or an erased row)
      const uint64_t sbase = fbase + (uint64_t)s * r_ss * mo;
      const uint32_t lsym = lbase + s * r_ss * a.M_occ * BPS;   // the symbol's rows, mod 2^32
      const uint32_t psym = pbase + s * r_ss * a.M_occ * PBS;
      v2f z[N];
      float nu[N];
#pragma unroll
      for (int t = 0; t < N; t++) { z[t] = v2f{0.0f, 0.0f}; nu[t] = 0.0f; }
      const bool live = s < n_out;      // (uniform)
      if (live) {
        v2f sb[N];
        float vv[N];
#pragma unroll
        for (int t = 0; t < N; t++) {
          if constexpr (N > 1) {
            float lm[2 * B];
#pragma unroll
            for (int i = 0; i < 2 * B; i++) lm[i] = 0.0f;
            if (have_prior)
              pic_prior_get<B>(pimg + (q * N + t) * PRS +
                                   ((psym + (uint32_t)t * r_ts * a.M_occ * PBS) & 15u) + tid * PBS,
                               ips, lm);
            float mr, vr, mi, vi;
            pic_moments<B>(lm, a.qam.scale, &mr, &vr);
            pic_moments<B>(lm + B, a.qam.scale, &mi, &vi);
            sb[t] = v2f{mr, mi};
            vv[t] = vr + vi;
          } else {
            sb[t] = v2f{0.0f, 0.0f};
            vv[t] = 1.0f;
          }
        }
        pic_detect<N>(qd, qo, s2, lam, y[q], sb, vv, z, nu);
      }
#pragma unroll
      for (int t = 0; t < N; t++) {
        const bool on = live && good;   // an erased row or carrier: z = 0, idx = 0, LLRs 0
        v2f pt;
        const v2f zt = on ? z[t] : v2f{0.0f, 0.0f};
        const uint32_t idx = on ? sic_slice(zt, a.qam, &pt) : 0u;
        const uint32_t to = (uint32_t)t * r_ts * a.M_occ;
        if (a.out_sym)
          __builtin_nontemporal_store(zt, reinterpret_cast<v2f *>(a.out_sym + sbase + to));
        img[(q * N + t) * kSicT + tid] = (uint8_t)idx;
        const float w = on ? a.llr_scale / fmaxf(nu[t], 1e-30f) : 0.0f;
        float lv[2 * B];
        llr_dim<B>(on ? zt.x : nanv, a.qam.scale, w, lv);
        llr_dim<B>(on ? zt.y : nanv, a.qam.scale, w, lv + B);
        sic_llr_put<B, F32>(limg + (q * N + t) * RS + ((lsym + to * BPS) & 15u) + tid * BPS, lv);
      }
    }
    __syncthreads();
    // ---- phase 4, the LLR image to d_llr: 16-byte chunks, narrower pieces at a row's ends
    {
      const uint32_t nb = nj * BPS;     // a row's LLR bytes in this tile
      for (uint32_t w = tid; w < rows * CH; w += kSicT) {
        const uint32_t r = w / CH, c = w - r * CH;
        const uint32_t q = r / N, t = r - q * N;
        uint8_t *dst = reinterpret_cast<uint8_t *>(a.llr) + (pic_row(a, f, t, s0 + q) * mo + j0) * BPS;
        const uint32_t mis = (uint32_t)((uintptr_t)dst & 15u);
        const uint8_t *src = limg + r * RS;           // image byte mis is dst[0]
        uint8_t *al = dst - mis;                      // the aligned span: image byte b is al[b]
        const uint32_t b0 = 16 * c;
        if (b0 >= mis && b0 + 16 <= mis + nb) {
          const v4u v = *reinterpret_cast<const v4u *>(src + b0);
          __builtin_nontemporal_store(v, reinterpret_cast<v4u *>(al + b0));
        } else {
          for (uint32_t bb = b0; bb < b0 + 16; bb += sizeof(edge_t))
            if (bb >= mis && bb < mis + nb)
              *reinterpret_cast<edge_t *>(al + bb) = *reinterpret_cast<const edge_t *>(src + bb);
        }
      }
    }
    // ---- phase 5, the index image to out_idx: dwords, single bytes at a row's ends
    if (a.out_idx) {                    // (uniform)
      for (uint32_t w = tid; w < rows * SLOTS; w += kSicT) {
        const uint32_t r = w / SLOTS, c = w - r * SLOTS;
        const uint32_t q = r / N, t = r - q * N;
        uint8_t *dst = a.out_idx + pic_row(a, f, t, s0 + q) * mo + j0;   // the row's nj bytes
        const uint8_t *src = img + r * kSicT;
        const uint32_t mis = (uint32_t)((uintptr_t)dst & 3u);
        const int b0 = (int)(4 * c) - (int)mis;    // dword c of the aligned span: bytes b0..b0+3
        if (b0 >= 0 && b0 + 4 <= (int)nj) {
          uint32_t v;
          if (mis == 0) v = *reinterpret_cast<const uint32_t *>(src + b0);
          else v = (uint32_t)src[b0] | ((uint32_t)src[b0 + 1] << 8) |
                   ((uint32_t)src[b0 + 2] << 16) | ((uint32_t)src[b0 + 3] << 24);
          __builtin_nontemporal_store(v, reinterpret_cast<uint32_t *>(dst + b0));
        } else {
          for (int b = 0; b < 4; b++) {
            const int bb = b0 + b;
            if (bb >= 0 && bb < (int)nj) dst[bb] = src[bb];
          }
        }
      }
    }
    __syncthreads();
  }
}

template <int N, int B, bool F32>
static void pic_pass_launch(const PicPassArgs &a, uint32_t nf, hipStream_t s) {
  const dim3 grid((a.M_occ + kSicT - 1) / kSicT, (a.max_out + kSicSB - 1) / kSicSB, nf);
  hipLaunchKernelGGL((pic_pass_kernel<N, B, F32>), grid, dim3(kSicT), 0, s, a);
}

template <int N>
static bool pic_pass_bits(const PicPassArgs &a, uint32_t nf, hipStream_t s) {
  switch (a.bits * 2 + (a.f32 ? 1 : 0)) {
    case 2: pic_pass_launch<N, 1, false>(a, nf, s); return true;
    case 3: pic_pass_launch<N, 1, true>(a, nf, s); return true;
    case 4: pic_pass_launch<N, 2, false>(a, nf, s); return true;
    case 5: pic_pass_launch<N, 2, true>(a, nf, s); return true;
    case 6: pic_pass_launch<N, 3, false>(a, nf, s); return true;
    case 7: pic_pass_launch<N, 3, true>(a, nf, s); return true;
    case 8: pic_pass_launch<N, 4, false>(a, nf, s); return true;
    case 9: pic_pass_launch<N, 4, true>(a, nf, s); return true;
    default: return false;
  }
}

bool launch_pic_pass(const PicPassArgs &a, uint32_t n_frames, hipStream_t s) {
  if (a.llr == nullptr) return false;
  if (n_frames == 0 || a.max_out == 0 || a.M_occ == 0) return true;
  if (n_frames > 65535u || (a.max_out + kSicSB - 1) / kSicSB > 65535u) return false;
  if ((uint64_t)a.N * a.max_out * a.M_occ >= 0xFFFFFFFFull) return false;
  switch (a.N) {
    case 1: return pic_pass_bits<1>(a, n_frames, s);
    case 2: return pic_pass_bits<2>(a, n_frames, s);
    case 4: return pic_pass_bits<4>(a, n_frames, s);
    default: return false;
  }
}

}  // namespace mimo
