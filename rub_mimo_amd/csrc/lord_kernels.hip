// rub_mimo_amd/csrc/lord_kernels.hip -- layered tree-search soft detection on gfx950
// (mimo_rx_lord_soft, DESIGN.md "Layered tree search"): per carrier and target stream the order
// of the other streams and the Cholesky factor of the permuted, regularised Gram matrix, and
// the pass that enumerates every value of the target's symbol, detects the other streams by
// hard successive cancellation under each and writes max-log LLRs over the L^2 candidates.
//
// No reference counterpart: framing.cc's detectors are linear. A separate, opt-in pass over
// the decode's d_out_sym; nothing here is launched by the batch itself.
//
// Compiled with -ffp-contract=off like pic_kernels.hip: the slicer is the decode's bit for bit
// and both LLR formats compute the same fp32 value. The sums that want a fused multiply-add
// spell it out.
#pragma clang fp contract(off)

#include "sic_pass.hpp"

namespace mimo {

// ------------------------------------------------------------------------------------
// Tables. One thread per (frame, subcarrier): Q = G^H G in fp64, stored as fp32 in
// pic_tables_kernel's Hermitian-packed form; then per target t the permutation p (the other
// streams by increasing stored Q[u][u], ties to the higher index, then t: read from the back
// it is the detection order) and the upper factor U of P (Q + r I) P^T (r = s2, and 0 at N = 2,
// where the one sliced stream has to be the exact minimiser of the metric), eliminated in fp64
// from the stored fp32 Q and stored as fp32: N diagonal values, their N reciprocals, then Re and
// Im of the N (N - 1) / 2 entries above the diagonal, row-major. Everything at stride M_occ.
// ok = 0 erases the carrier in the pass. The permuted matrix is indexed at run time, so this
// kernel, unlike the pass, keeps its small fp64 matrices in scratch: it runs once per call on
// F x M_occ threads.
constexpr int kLordTabT = 64;

template <int N>
__global__ __launch_bounds__(kLordTabT) void lord_tables_kernel(LordTableArgs a) {
  constexpr int UR = lord_u_rows(N);
  const uint32_t f = blockIdx.y;
  const uint32_t k = blockIdx.x * kLordTabT + threadIdx.x;
  if (k >= a.M) return;
  const int j = a.occ_index[k];
  if (j < 0) return;
  const uint64_t mo = a.M_occ;
  float *Qq = a.Q + (uint64_t)f * N * N * mo + j;
  float *Uq = a.U + (uint64_t)f * N * UR * mo + j;
  const FrameInfo &I = a.info[f];
  bool ok = I.status == 0 && I.noise_var > 0.0f && isfinite(I.noise_var);
  float q[N * N];
  double Ar[N][N], Ai[N][N];
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
          Ar[t][t] = (double)q[t] + (N > 2 ? (double)I.noise_var : 0.0);
          Ai[t][t] = 0.0;
        } else {
          q[row] = (float)sr;
          q[row + 1] = (float)si;
          ok = ok && isfinite(q[row]) && isfinite(q[row + 1]);
          Ar[t][u] = q[row]; Ai[t][u] = q[row + 1];
          Ar[u][t] = q[row]; Ai[u][t] = -(double)q[row + 1];
          row += 2;
        }
      }
  }
  float uf[N * UR];
  uint32_t pw[N];
#pragma unroll
  for (int e = 0; e < N * UR; e++) uf[e] = 0.0f;
  for (int t = 0; t < N; t++) {
    int p[N];
    p[N - 1] = t;
    pw[t] = 0;
    if (!ok) continue;
    for (int u = 0; u < N; u++) {
      if (u == t) continue;
      int rank = 0;      // streams detected before u
      for (int v = 0; v < N; v++)
        if (v != t && v != u && (q[v] > q[u] || (q[v] == q[u] && v < u))) rank++;
      p[N - 2 - rank] = u;
    }
    for (int i = 0; i < N; i++) pw[t] |= (uint32_t)p[i] << (8 * i);
    double Ur[N][N], Ui[N][N];
    float *o = uf + t * UR;
    int e = 2 * N;
    for (int r = 0; r < N; r++) {
      double d = Ar[p[r]][p[r]];
      for (int c = 0; c < r; c++) d -= Ur[c][r] * Ur[c][r] + Ui[c][r] * Ui[c][r];
      const bool pos = d > 0.0 && isfinite(d);
      const double urr = pos ? sqrt(d) : 1.0, ir = 1.0 / urr;
      o[r] = (float)urr;
      o[N + r] = (float)ir;
      ok = ok && pos && isfinite(o[r]) && isfinite(o[N + r]) && o[r] > 0.0f;
      Ur[r][r] = urr; Ui[r][r] = 0.0;
      for (int i = r + 1; i < N; i++) {
        double xr = Ar[p[r]][p[i]], xi = Ai[p[r]][p[i]];
        for (int c = 0; c < r; c++) {    // - conj(U[c][r]) U[c][i]
          xr -= Ur[c][r] * Ur[c][i] + Ui[c][r] * Ui[c][i];
          xi -= Ur[c][r] * Ui[c][i] - Ui[c][r] * Ur[c][i];
        }
        Ur[r][i] = xr * ir; Ui[r][i] = xi * ir;
        o[e] = (float)Ur[r][i];
        o[e + 1] = (float)Ui[r][i];
        ok = ok && isfinite(o[e]) && isfinite(o[e + 1]);
        e += 2;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < N * N; e++) Qq[(uint64_t)e * mo] = ok ? q[e] : 0.0f;
  for (int e = 0; e < N * UR; e++) Uq[(uint64_t)e * mo] = ok ? uf[e] : 0.0f;
  for (int t = 0; t < N; t++) a.perm[((uint64_t)f * N + t) * mo + j] = ok ? pw[t] : 0u;
  a.ok[(uint64_t)f * mo + j] = ok ? 1 : 0;
}

template <int N>
static void lord_tables_launch(const LordTableArgs &a, uint32_t nf, hipStream_t s) {
  hipLaunchKernelGGL((lord_tables_kernel<N>), dim3((a.M + kLordTabT - 1) / kLordTabT, nf),
                     dim3(kLordTabT), 0, s, a);
}

bool launch_lord_tables(const LordTableArgs &a, uint32_t n_frames, hipStream_t s) {
  if (n_frames == 0) return true;
  if (n_frames > 65535u) return false;
  switch (a.N) {
    case 1: lord_tables_launch<1>(a, n_frames, s); return true;
    case 2: lord_tables_launch<2>(a, n_frames, s); return true;
    case 4: lord_tables_launch<4>(a, n_frames, s); return true;
    default: return false;
  }
}

// ------------------------------------------------------------------------------------
// The symbol pass, lord_pass_kernel<N, B, F32>, in the frame of pic_pass_kernel: a workgroup
// owns (frame, tile of kSicT adjacent carriers, kSicSB symbols), thread tid holds carrier j's Q
// for all of them, an iteration takes SC symbols, and the index image and the LLR image leave
// through LDS by sic_pass.hpp's drains.
//
// Inside an iteration the target stream t is the outer loop and the symbol the inner one, both
// at run time: the lane loads target t's factor U (N^2 + N floats) and permutation once per
// iteration and keeps them in registers, and per symbol it reads y (N complex values) and Q
// (N^2 floats; both from the cache after the first target), forms m = lam y + Q y, P m by
// selects on the lane's own permutation, and yt = U^-H P m by forward substitution on the
// stored reciprocals. Every load is a uniform row pointer indexed by the lane's carrier.
//
// The candidate c = (gI << B) | gQ: the index's halves are the Gray codes of the two levels.
// Both candidate loops run at run time and are not unrolled: gI and gQ are uniform, so their
// levels and their bits are scalar, the body exists once, and every array index is a
// compile-time constant: no scratch. Unrolling the inner loop was measured and is slower: the
// 4x4 64-QAM int8 instance took 99.9 ms on the C3 x 64 batch not unrolled (163 VGPRs, three
// waves per SIMD), 126.5 ms unrolled by two (172, two waves) and 111.8 ms fully unrolled with
// the minima in static registers (255, two waves; 181.8 ms where two AGPRs on top left one
// wave). What depends on the target's symbol alone is hoisted: yt_k - U_k,N-1 Re c per gI, then
// one multiply-add per component for Im c. Per candidate the chain is k = N-2 .. 0: the
// multiply-adds of the streams already sliced, the decode's slicer (sic_slice), the residual,
// and its square and the point's energy into the metric.
//
// The minima are kept per dimension: min over the candidates with bit i of the real half = v is
// a minimum over whole gI rows, and of the imaginary half over whole gQ columns. A candidate
// updates, per bit of the imaginary half, the one of the two running minima its scalar bit
// selects, and the row's minimum and its argument by a compare and two selects; a row then
// updates the real half's minima the same way. The hard decision takes a row's argument only on
// a strict improvement, and rows and columns are visited in index order: the lowest c wins a
// tie. A NaN metric enters no minimum; if every metric is NaN the minima stay +inf, inf - inf
// is NaN and the LLR is 0.
template <int N, int B, bool F32>
__global__ __launch_bounds__(kSicT) void lord_pass_kernel(LordPassArgs a) {
  constexpr int SC = sic_soft_sc<N, B, F32>();
  constexpr int NO = N * (N - 1) / 2;
  constexpr int L = 1 << B;
  constexpr int UR = lord_u_rows(N);
  constexpr int BPS = sic_llr_bps<B, F32>();
  constexpr int RS = sic_llr_rs<B, F32>();
  __shared__ __attribute__((aligned(16))) uint8_t limg[SC * N * RS];
  __shared__ __attribute__((aligned(16))) uint8_t img[SC * N * kSicT];
  const uint32_t tid = threadIdx.x;
  const uint32_t f = blockIdx.z;
  const uint32_t j0 = blockIdx.x * kSicT, j = j0 + tid;
  const uint32_t s_lo = blockIdx.y * kSicSB;
  const uint32_t s_hi = min(s_lo + (uint32_t)kSicSB, a.max_out);
  const uint32_t nj = min((uint32_t)kSicT, a.M_occ - j0);
  const bool lane = j < a.M_occ;
  const FrameInfo &I = a.info[f];
  const float s2 = I.noise_var;
  // a frame with noise_var <= 0 or not finite is erased as a whole
  const uint32_t n_out = (I.status == 0 && s2 > 0.0f && isfinite(s2)) ? min(I.n_sym, a.max_out) : 0u;
  const float lam = a.mmse ? s2 : 0.0f;
  const uint64_t mo = a.M_occ;
  const uint32_t r_ts = a.symbol_major ? 1u : a.max_out, r_ss = a.symbol_major ? a.N : 1u;
  // the address of (frame, tile) in d_llr mod 2^32: the image needs its low 4 bits
  const uint32_t lbase = (uint32_t)(uintptr_t)a.llr + (f * a.N * a.max_out * a.M_occ + j0) * BPS;
  const float scale = a.qam.scale;
  const float inf = __builtin_inff();
  const float kw = a.llr_scale / s2;    // (only used where s2 > 0)
  const float reg = N > 2 ? s2 : 0.0f;  // the factor's regularisation

  // ---- phase 1, the table prologue: a lane without work is erased
  const bool work = lane && s_lo < n_out;
  const bool good = work && a.ok[(uint64_t)f * mo + j] != 0;
  // every load below is a uniform row pointer indexed by the lane's carrier: a scalar base and a
  // 32-bit lane offset, not a 64-bit address per load and lane
  const float *Qf = a.Q + (uint64_t)f * N * N * mo;
  const float2 *symf = a.sym + (uint64_t)f * a.N * a.max_out * mo;
  auto row_of = [&](uint32_t q, uint32_t t, uint32_t s0) -> uint64_t {
    return a.symbol_major ? ((uint64_t)f * a.max_out + (s0 + q)) * a.N + t
                          : ((uint64_t)f * a.N + t) * a.max_out + (s0 + q);
  };

  for (uint32_t s0 = s_lo; s0 < s_hi; s0 += SC) {
    const uint32_t nq = min((uint32_t)SC, s_hi - s0);
    const uint32_t rows = nq * N;
    if (lane) {
#pragma unroll 1
      for (uint32_t t = 0; t < (uint32_t)N; t++) {
        // ---- phase 2, target t's factor and permutation
        float ud[N], ur[N];
        float2 uo[NO > 0 ? NO : 1];
        uint32_t pw = 0;
        uo[0] = make_float2(0.0f, 0.0f);
        const bool any = good && s0 < n_out;
        const float *Ut = a.U + ((uint64_t)f * N + t) * UR * mo;     // (uniform)
#pragma unroll
        for (int k = 0; k < N; k++) {
          ud[k] = any ? (Ut + (uint64_t)k * mo)[j] : 1.0f;
          ur[k] = any ? (Ut + (uint64_t)(N + k) * mo)[j] : 1.0f;
        }
#pragma unroll
        for (int e = 0; e < NO; e++)
          uo[e] = any ? make_float2((Ut + (uint64_t)(2 * N + 2 * e) * mo)[j],
                                    (Ut + (uint64_t)(2 * N + 2 * e + 1) * mo)[j])
                      : make_float2(0.0f, 0.0f);
        if (any) pw = (a.perm + ((uint64_t)f * N + t) * mo)[j];
        const uint32_t to = t * r_ts * a.M_occ;
#pragma unroll 1
        for (uint32_t q = 0; q < nq; q++) {
          const uint32_t s = s0 + q;
          const uint32_t lsym = lbase + s * r_ss * a.M_occ * BPS;   // the symbol's rows, mod 2^32
          float lv[2 * B];
#pragma unroll
          for (int i = 0; i < 2 * B; i++) lv[i] = 0.0f;
          uint32_t bidx = 0;
          if (s < n_out && good) {       // (s < n_out uniform) else an erased row or carrier
            // ---- phase 3, one symbol of one target: m, P m, yt
            // (Q is read here, per target and symbol, and not held across the candidate loop)
            float qd[N];
            float2 qo[NO > 0 ? NO : 1];
            qo[0] = make_float2(0.0f, 0.0f);
#pragma unroll
            for (int u = 0; u < N; u++) qd[u] = (Qf + (uint64_t)u * mo)[j];
#pragma unroll
            for (int e = 0; e < NO; e++)
              qo[e] = make_float2((Qf + (uint64_t)(N + 2 * e) * mo)[j],
                                  (Qf + (uint64_t)(N + 2 * e + 1) * mo)[j]);
            v2f y[N], m[N];
#pragma unroll
            for (int u = 0; u < N; u++)
              y[u] = reinterpret_cast<const v2f *>(
                  symf + ((uint64_t)u * r_ts + (uint64_t)s * r_ss) * mo)[j];
#pragma unroll
            for (int u = 0; u < N; u++) {
              v2f acc = v2f{lam * y[u].x, lam * y[u].y};
#pragma unroll
              for (int v = 0; v < N; v++) {
                float2 qv;
                if (v == u) qv = make_float2(qd[u], 0.0f);
                else if (u < v) qv = qo[u * N - u * (u + 1) / 2 + (v - u - 1)];
                else qv = cconj(qo[v * N - v * (v + 1) / 2 + (u - v - 1)]);
                acc = sic_mac(acc, qv, y[v], sic_rot(y[v]));
              }
              m[u] = acc;
            }
            float r0[B], r1[B], c0[B], c1[B];
#pragma unroll
            for (int i = 0; i < B; i++) r0[i] = r1[i] = c0[i] = c1[i] = inf;
            float best = inf;
            v2f yt[N];
            if constexpr (N > 1) {
#pragma unroll
              for (int k = 0; k < N; k++) {
                const uint32_t pk = (pw >> (8 * k)) & 0xFFu;
                v2f acc = m[0];
#pragma unroll
                for (int u = 1; u < N; u++) acc = pk == (uint32_t)u ? m[u] : acc;
#pragma unroll
                for (int i = 0; i < k; i++) {     // - conj(U[i][k]) yt[i]
                  const float2 u = uo[i * N - i * (i + 1) / 2 + (k - i - 1)];
                  acc = sic_mac(acc, make_float2(-u.x, u.y), yt[i], sic_rot(yt[i]));
                }
                yt[k] = acc * ur[k];
              }
            } else {
              yt[0] = m[0];
            }
            // ---- phase 4, the L^2 candidates
#pragma unroll 1
            for (uint32_t gI = 0; gI < (uint32_t)L; gI++) {
              const uint32_t mI = gray_dec(gI);
              const float cr = (float)(int32_t)(2 * mI - (L - 1)) * scale;
              const float cr2 = cr * cr;
              v2f base[N];
              if constexpr (N > 1) {
#pragma unroll
                for (int k = 0; k < N - 1; k++) {
                  const float2 u = uo[k * N - k * (k + 1) / 2 + (N - 1 - k - 1)];
                  base[k] = v2f{__builtin_fmaf(-cr, u.x, yt[k].x), __builtin_fmaf(-cr, u.y, yt[k].y)};
                }
                base[N - 1] = v2f{__builtin_fmaf(-cr, ud[N - 1], yt[N - 1].x), yt[N - 1].y};
              } else {
                base[0] = v2f{cr * yt[0].x, 0.0f};     // Re c Re m
              }
              float rmin = inf;
              uint32_t rarg = 0;
#pragma unroll 1
              for (uint32_t gQ = 0; gQ < (uint32_t)L; gQ++) {
                const float ci = (float)(int32_t)(2 * gray_dec(gQ) - (L - 1)) * scale;
                float en = __builtin_fmaf(ci, ci, cr2);
                float D;
                if constexpr (N == 1) {
                  const float dot = __builtin_fmaf(ci, yt[0].y, base[0].x);
                  D = __builtin_fmaf(qd[0], en, -2.0f * dot);
                } else {
                  v2f sv[N];
                  const float ry = __builtin_fmaf(-ci, ud[N - 1], base[N - 1].y);
                  float acc = __builtin_fmaf(ry, ry, base[N - 1].x * base[N - 1].x);
#pragma unroll
                  for (int k = N - 2; k >= 0; k--) {
                    const float2 u = uo[k * N - k * (k + 1) / 2 + (N - 1 - k - 1)];
                    v2f av = v2f{__builtin_fmaf(ci, u.y, base[k].x), __builtin_fmaf(-ci, u.x, base[k].y)};
#pragma unroll
                    for (int i = N - 2; i > k; i--) {
                      const float2 w = uo[k * N - k * (k + 1) / 2 + (i - k - 1)];
                      av = sic_mac(av, make_float2(-w.x, -w.y), sv[i], sic_rot(sv[i]));
                    }
                    v2f pt;
                    (void)sic_slice(av * ur[k], a.qam, &pt);
                    sv[k] = pt;
                    const float rx = __builtin_fmaf(-ud[k], pt.x, av.x);
                    const float rz = __builtin_fmaf(-ud[k], pt.y, av.y);
                    acc = __builtin_fmaf(rx, rx, acc);
                    acc = __builtin_fmaf(rz, rz, acc);
                    en = __builtin_fmaf(pt.x, pt.x, en);
                    en = __builtin_fmaf(pt.y, pt.y, en);
                  }
                  D = N > 2 ? __builtin_fmaf(-reg, en, acc) : acc;
                }
#pragma unroll
                for (int i = 0; i < B; i++) {
                  const bool one = (gQ >> (B - 1 - i)) & 1u;   // (uniform)
                  c1[i] = one ? fminf(c1[i], D) : c1[i];
                  c0[i] = one ? c0[i] : fminf(c0[i], D);
                }
                const bool lt = D < rmin;
                rmin = lt ? D : rmin;
                rarg = lt ? gQ : rarg;
              }
#pragma unroll
              for (int i = 0; i < B; i++) {
                const bool one = (gI >> (B - 1 - i)) & 1u;     // (uniform)
                r1[i] = one ? fminf(r1[i], rmin) : r1[i];
                r0[i] = one ? r0[i] : fminf(r0[i], rmin);
              }
              const bool lt = rmin < best;
              best = lt ? rmin : best;
              bidx = lt ? ((gI << B) | rarg) : bidx;
            }
            // ---- phase 5, the LLRs of the target's 2 B bits
#pragma unroll
            for (int i = 0; i < B; i++) {
              const float vr = (r1[i] - r0[i]) * kw, vi = (c1[i] - c0[i]) * kw;
              lv[i] = (vr == vr) ? vr : 0.0f;
              lv[B + i] = (vi == vi) ? vi : 0.0f;
            }
          }
          img[(q * N + t) * kSicT + tid] = (uint8_t)bidx;
          sic_llr_put<B, F32>(limg + (q * N + t) * RS + ((lsym + to * BPS) & 15u) + tid * BPS, lv);
        }
      }
    }
    __syncthreads();
    // ---- phase 6, the LLR image to d_llr and the index image to out_idx
    sic_llr_drain<N, B, F32>(limg, a.llr, rows, nj, mo, j0, tid,
                             [&](uint32_t q, uint32_t t) { return row_of(q, t, s0); });
    if (a.out_idx)                      // (uniform)
      sic_idx_drain<N>(img, a.out_idx, rows, nj, mo, j0, tid,
                       [&](uint32_t q, uint32_t t) { return row_of(q, t, s0); });
    __syncthreads();
  }
}

template <int N, int B, bool F32>
static void lord_pass_launch(const LordPassArgs &a, uint32_t nf, hipStream_t s) {
  const dim3 grid((a.M_occ + kSicT - 1) / kSicT, (a.max_out + kSicSB - 1) / kSicSB, nf);
  hipLaunchKernelGGL((lord_pass_kernel<N, B, F32>), grid, dim3(kSicT), 0, s, a);
}

template <int N>
static bool lord_pass_bits(const LordPassArgs &a, uint32_t nf, hipStream_t s) {
  switch (a.bits * 2 + (a.f32 ? 1 : 0)) {
    case 2: lord_pass_launch<N, 1, false>(a, nf, s); return true;
    case 3: lord_pass_launch<N, 1, true>(a, nf, s); return true;
    case 4: lord_pass_launch<N, 2, false>(a, nf, s); return true;
    case 5: lord_pass_launch<N, 2, true>(a, nf, s); return true;
    case 6: lord_pass_launch<N, 3, false>(a, nf, s); return true;
    case 7: lord_pass_launch<N, 3, true>(a, nf, s); return true;
    case 8: lord_pass_launch<N, 4, false>(a, nf, s); return true;
    case 9: lord_pass_launch<N, 4, true>(a, nf, s); return true;
    default: return false;
  }
}

bool launch_lord_pass(const LordPassArgs &a, uint32_t n_frames, hipStream_t s) {
  if (a.llr == nullptr) return false;
  if (n_frames == 0 || a.max_out == 0 || a.M_occ == 0) return true;
  if (n_frames > 65535u || (a.max_out + kSicSB - 1) / kSicSB > 65535u) return false;
  if ((uint64_t)a.N * a.max_out * a.M_occ >= 0xFFFFFFFFull) return false;
  switch (a.N) {
    case 1: return lord_pass_bits<1>(a, n_frames, s);
    case 2: return lord_pass_bits<2>(a, n_frames, s);
    case 4: return lord_pass_bits<4>(a, n_frames, s);
    default: return false;
  }
}

}  // namespace mimo
