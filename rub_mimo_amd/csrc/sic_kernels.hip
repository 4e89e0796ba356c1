// rub_mimo_amd/csrc/sic_kernels.hip -- ordered MMSE-SIC detection on gfx950: the per-carrier
// detection order and tables of a batch's frames, and the pass that applies them to the batch's
// equalised symbols (mimo_rx_sic_detect, DESIGN.md "SIC detection"), alone or with the
// max-log LLRs of every stage (mimo_rx_sic_soft, DESIGN.md "Soft-output SIC"), and that soft
// output with expected-symbol cancellation (mimo_rx_sic_soft_fb, DESIGN.md "Soft-feedback SIC").
//
// No reference counterpart: framing.cc's detectors are linear. A separate, opt-in pass over the
// decode's d_out_sym; nothing here is launched by the batch itself.
//
// Compiled with -ffp-contract=off: the slicer computes exactly floorf((z inv_scale + L) 0.5f),
// which the tests restate bit for bit. The complex sums spell their fused multiply-adds out.
// Both LLR formats compute the same fp32 value for the same reason (llr.hpp).
// A frame slot is taken to hold fewer than 2^32 symbols (launch_sic_pass checks).
#pragma clang fp contract(off)

#include <type_traits>

#include "sic_pass.hpp"

namespace mimo {

// ------------------------------------------------------------------------------------
// Tables. One thread per (frame, subcarrier), everything in fp64: Q = G^H G, one Gauss-Jordan
// solve with partial pivoting for E = (Q + s2 I)^-1, then N stages. Stage k picks the stream
// pi of S with the smallest E[t][t], writes row k of T and C from row pi of E, and removes pi
// from S without a new inversion: E_(S \ pi) = E[S',S'] - E[S',pi] E[pi,S'] / E[pi][pi].
// Every array index is a loop counter (the row and column of pi are picked out by compares), so
// for N <= 4 the loops unroll and Q and E live in registers. At N = 8 they stay loops and the
// two 8x8 complex double matrices are runtime-indexed scratch (2 KiB per thread): accepted, the
// kernel runs once per frame on N^2 M values and is not the hot path (DESIGN.md has the time).
struct cdd { double re, im; };
MIMO_DEV cdd cdd_mul(cdd a, cdd b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
MIMO_DEV bool cdd_finite(cdd a) { return isfinite(a.re) && isfinite(a.im); }

constexpr int kSicTabT = 64;
template <int N>
constexpr int sic_unroll() { return N <= 4 ? N : 1; }

// Gauss-Jordan with partial pivoting on [A | B], as the weights' cd_solve; false on a zero pivot
template <int N>
MIMO_DEV bool sic_solve(cdd (&A)[N][N], cdd (&B)[N][N]) {
  constexpr int U = sic_unroll<N>();
#pragma unroll U
  for (int c = 0; c < N; c++) {
    int piv = c;
    double best = -1.0;
#pragma unroll U
    for (int rr = 0; rr < N; rr++) {
      const double m = A[rr][c].re * A[rr][c].re + A[rr][c].im * A[rr][c].im;
      if (rr >= c && m > best) { best = m; piv = rr; }
    }
#pragma unroll U
    for (int rr = 0; rr < N; rr++) {
      if (rr > c && rr == piv) {
#pragma unroll U
        for (int k = 0; k < N; k++) {
          const cdd t1 = A[c][k]; A[c][k] = A[rr][k]; A[rr][k] = t1;
          const cdd t2 = B[c][k]; B[c][k] = B[rr][k]; B[rr][k] = t2;
        }
      }
    }
    const cdd d = A[c][c];
    const double dd = d.re * d.re + d.im * d.im;
    if (!(dd > 0.0)) return false;
    const cdd inv = {d.re / dd, -d.im / dd};
#pragma unroll U
    for (int k = 0; k < N; k++) {
      A[c][k] = cdd_mul(A[c][k], inv);
      B[c][k] = cdd_mul(B[c][k], inv);
    }
#pragma unroll U
    for (int rr = 0; rr < N; rr++) {
      if (rr == c) continue;
      const cdd fct = A[rr][c];
#pragma unroll U
      for (int k = 0; k < N; k++) {
        const cdd x = cdd_mul(fct, A[c][k]), y = cdd_mul(fct, B[c][k]);
        A[rr][k].re -= x.re; A[rr][k].im -= x.im;
        B[rr][k].re -= y.re; B[rr][k].im -= y.im;
      }
    }
  }
  return true;
}

template <int N>
__global__ __launch_bounds__(kSicTabT) void sic_tables_kernel(SicTableArgs a) {
  constexpr int U = sic_unroll<N>();
  constexpr int NC = (int)sic_c_rows(N);
  const uint32_t f = blockIdx.y;
  const uint32_t k = blockIdx.x * kSicTabT + threadIdx.x;
  if (k >= a.M) return;
  const int j = a.occ_index[k];
  if (j < 0) return;
  const uint64_t mo = a.M_occ;
  float2 *Tq = a.T + (uint64_t)f * N * N * mo + j;        // [stage][u], stride M_occ
  float2 *Cq = a.C + (uint64_t)f * NC * mo + j;           // [k (k - 1) / 2 + i]
  uint8_t *oq = a.order + ((uint64_t)f * mo + j) * N;
  float *nq = a.nu + (uint64_t)f * N * mo + j;            // [stream]
  const FrameInfo &I = a.info[f];
  bool fail = false;
  if (I.status == 0) {
    const double s2 = (double)I.noise_var;
    const double lam = (a.detector == 2) ? s2 : 0.0;
    const float2 *g = a.G + ((uint64_t)f * a.M + k) * N * N;
    cdd Q[N][N], E[N][N];
    {
      cdd A[N][N];
#pragma unroll U
      for (int v = 0; v < N; v++)
#pragma unroll U
        for (int u = 0; u < N; u++) {
          double sr = 0.0, si = 0.0;
#pragma unroll U
          for (int rr = 0; rr < N; rr++) {
            const double gar = g[rr * N + v].x, gai = g[rr * N + v].y;
            const double gbr = g[rr * N + u].x, gbi = g[rr * N + u].y;
            sr += gar * gbr + gai * gbi;
            si += gar * gbi - gai * gbr;
          }
          Q[v][u] = {sr, si};
          A[v][u] = {sr + ((v == u) ? s2 : 0.0), si};
          E[v][u] = {(v == u) ? 1.0 : 0.0, 0.0};
        }
      fail = !sic_solve<N>(A, E);
    }
    uint32_t active = (1u << N) - 1u;
    int stage_of[N];
#pragma unroll U
    for (int t = 0; t < N; t++) stage_of[t] = 0;
#pragma unroll U
    for (int st = 0; st < N; st++) {
      if (fail) break;
      // the stream of S with the smallest real diagonal entry, the lowest index on a tie
      int pi = -1;
      double best = 0.0;
#pragma unroll U
      for (int t = 0; t < N; t++) {
        const bool in = (active >> t) & 1u;
        if (in && (pi < 0 || E[t][t].re < best)) { best = E[t][t].re; pi = t; }
      }
      // row and column pi of E
      cdd row[N], col[N];
#pragma unroll U
      for (int t = 0; t < N; t++) {
        row[t] = col[t] = {0.0, 0.0};
#pragma unroll U
        for (int v = 0; v < N; v++) {
          if (v == pi) { row[t] = E[v][t]; col[t] = E[t][v]; }
        }
        if (!((active >> t) & 1u)) row[t] = col[t] = {0.0, 0.0};
        if (!cdd_finite(row[t])) fail = true;
      }
      const double beta = 1.0 - s2 * best;
      if (!(best > 0.0) || !(beta > 0.0)) fail = true;
      if (fail) break;
      const double ib = 1.0 / beta;
#pragma unroll U
      for (int u = 0; u < N; u++) {
        cdd rq = {0.0, 0.0};          // sum_{v in S} r_v Q[v][u] (row is zero off S)
#pragma unroll U
        for (int v = 0; v < N; v++) {
          const cdd p = cdd_mul(row[v], Q[v][u]);
          rq.re += p.re; rq.im += p.im;
        }
        if (!((active >> u) & 1u))    // u = pi_i, i = stage_of[u] < st
          Cq[(uint64_t)(st * (st - 1) / 2 + stage_of[u]) * mo] =
              make_float2((float)(rq.re * ib), (float)(rq.im * ib));
        Tq[(uint64_t)(st * N + u) * mo] = make_float2((float)((rq.re + lam * row[u].re) * ib),
                                                      (float)((rq.im + lam * row[u].im) * ib));
        if (u == pi) {
          nq[(uint64_t)u * mo] = (float)(s2 * best * ib);
          stage_of[u] = st;
        }
      }
      oq[st] = (uint8_t)pi;
      // E of S \ pi
      const double id = 1.0 / best;
#pragma unroll U
      for (int r = 0; r < N; r++)
#pragma unroll U
        for (int c = 0; c < N; c++) {
          const cdd p = cdd_mul(col[r], row[c]);
          E[r][c].re -= p.re * id;
          E[r][c].im -= p.im * id;
        }
      active &= ~(1u << pi);
    }
  }
  if (I.status != 0 || fail) {
    // an unsynced slot: all zero; a failed solve: zero tables, order 0..N-1, nu 0
    const float2 z = make_float2(0.0f, 0.0f);
    for (int e = 0; e < N * N; e++) Tq[(uint64_t)e * mo] = z;
    for (int e = 0; e < NC; e++) Cq[(uint64_t)e * mo] = z;
    for (int t = 0; t < N; t++) {
      oq[t] = (I.status == 0) ? (uint8_t)t : (uint8_t)0;
      nq[(uint64_t)t * mo] = 0.0f;
    }
  }
  // what tells a failed solve (LLRs 0) from a good carrier with nu = 0 because s2 = 0
  a.ok[(uint64_t)f * mo + j] = (I.status == 0 && !fail) ? 1 : 0;
}

template <int N>
static void sic_tables_launch(const SicTableArgs &a, uint32_t nf, hipStream_t s) {
  hipLaunchKernelGGL((sic_tables_kernel<N>), dim3((a.M + kSicTabT - 1) / kSicTabT, nf),
                     dim3(kSicTabT), 0, s, a);
}

bool launch_sic_tables(const SicTableArgs &a, uint32_t n_frames, hipStream_t s) {
  if (n_frames == 0) return true;
  if (n_frames > 65535u) return false;
  switch (a.N) {
    case 1: sic_tables_launch<1>(a, n_frames, s); return true;
    case 2: sic_tables_launch<2>(a, n_frames, s); return true;
    case 3: sic_tables_launch<3>(a, n_frames, s); return true;
    case 4: sic_tables_launch<4>(a, n_frames, s); return true;
    case 8: sic_tables_launch<8>(a, n_frames, s); return true;
    default: return false;
  }
}

// ------------------------------------------------------------------------------------
// The symbol pass, one kernel for both outputs: sic_pass_kernel<N, B, F32>, B = 0 the hard
// output (mimo_rx_sic_detect), B = 1..4 bits per dimension the soft output (mimo_rx_sic_soft).
// A workgroup owns (frame, tile of kSicT adjacent carriers, kSicSB symbols);
// thread tid holds carrier j's order and tables (N^2 + N (N - 1) / 2 complex values) in
// registers for all of them. Per iteration it takes SC symbols: all SC N loads of y (8 bytes per
// lane, a wave reads 512 contiguous bytes of a row) are issued before the first stage waits,
// then per symbol the N stages run in order (packed fp32 fused multiply-adds, C held negated),
// each one's z stored straight to the row of its stream (pi differs per lane, but changes
// slowly along the carriers). z leaves as 8-byte stores. The indices do not leave as one byte
// per lane (a byte store per lane costs a write transaction each, see soft_demap_kernel): every
// thread puts its bytes into an LDS image [symbol][stream][carrier] of the iteration, and the
// image leaves as dword stores, at most 3 single bytes at either end of a row whose address or
// length is no multiple of 4. Loads and stores are non-temporal: every byte is touched once.
//
// Soft output (B > 0) adds to that and changes none of it (one body: z and idx are the hard
// pass's bit for bit): per stage the 2 B max-log LLRs of its z weighted by
// llr_scale / max(nu_sic, 1e-30) of the stage's stream (N weights in registers). B = 0
// compiles none of it: no read of nu, ok or llr, no LLR image, no barrier unless out_idx is set.
// A lane's 2 B values at a 2 B-element lane stride are the store pattern that cost the soft
// demapper 2.49 ms (int8) and 16.2 ms (fp32) before its LDS image, so they leave the same way:
// every thread puts them into an LDS image [symbol][stream][carrier][2 B] of the iteration, at
// the row of its own pi_k like the index image, and the image leaves as contiguous 16-byte
// non-temporal stores per row. A row of d_llr starts at any multiple of its M_occ 2 B (4)
// bytes: the image row holds the row's bytes behind its own misalignment (address mod 16), so a
// 16-byte chunk of the image is a 16-byte aligned chunk of d_llr, and only the chunks at
// either end of a row whose address or length is no multiple of 16 leave in narrower pieces.
// The image sets the symbols per iteration: sic_sc<N>() halved until it fits kSicLlrImg.
//
// Soft feedback (FB, a form of B > 0 for N = 2, 4, 8: mimo_rx_sic_soft_fb) changes phase 2
// alone, behind if constexpr (FB), so that the other instances compile to what they compiled to
// without it: after the slicer, stage k < N - 1 replaces its point sh[k] by the posterior mean
// of its symbol and keeps the posterior variance (sic_soft_symbol), and stage k >= 1 weights its
// LLRs by llr_scale / max(nu_k, 1e-30) with nu_k = nu_sic + sum_{i<k} |C[k][i]|^2 var[i], one
// division per stage and symbol (stage 0 keeps the precomputed weight and is the soft output's
// bit for bit). Loads, stores, both images and both drains are the soft output's; the int8
// instances take half its symbols per iteration (SC in the kernel says why).
//
// The four phases (table prologue, one symbol's stages, LLR drain, index drain) are marked in
// the body, not split into functions. Each was tried as a MIMO_DEV function on a per-lane
// struct, one at a time: the symbol phase changed occupancy or scratch of 10 of the 45
// instances, the LLR drain of 4, the prologue of 1 (N = 8 64-QAM fp32, 12 -> 20 B of scratch);
// the index drain alone kept all three figures but changed every instance's instruction
// stream. Inline, on plain arrays, all 45 instances compile to the instruction streams of the
// two kernels this one replaced, so their measured times stand. (kSicT, kSicSB, sic_sc, the
// multiply-add, the slicer and the LLR image are in sic_pass.hpp: pic_kernels.hip shares them.)
MIMO_DEV uint64_t sic_row(const SicPassArgs &a, uint32_t f, uint32_t t, uint32_t s) {
  return a.symbol_major ? ((uint64_t)f * a.max_out + s) * a.N + t
                        : ((uint64_t)f * a.N + t) * a.max_out + s;
}

// Soft feedback (FB, mimo_rx_sic_soft_fb): the posterior mean and variance of one stage's symbol
// given its z and the stage's error power nu, per dimension p_m ~ exp(-(x - l_m)^2 / nu) over
// the L levels. On entry *pt is the slicer's point l_c of z, on return the mean; *var the sum of
// both dimensions' variances. The exponents are taken relative to l_c: with t = x - l_c and
// o_m = l_m - l_c, (x - l_m)^2 - (x - l_c)^2 = o_m (o_m - 2 t) = e_m >= 0 up to the slicer's
// rounding at a boundary (floored at 0), so every weight is at most 1, the slicer's own is
// exactly 1, and the sums can neither overflow nor vanish however far z lies outside the grid
// or however small nu is. Both dimensions run side by side as one packed value; the L levels
// are a loop over three running sums (sum w, sum w o, sum w o^2), not L live weights. exp is
// one v_exp_f32 on e_m (-log2 e / nu): its arguments are <= 0, so a result below the normal
// range may flush to 0, as a term that small vanishes in the sums anyway. The two reciprocals
// are v_rcp_f32 (1 ulp).
template <int B>
MIMO_DEV void sic_soft_symbol(v2f z, float nu, float scale, v2f *pt, float *var) {
  constexpr int L = 1 << B;
  const float g = -1.44269504f * __builtin_amdgcn_rcpf(fmaxf(nu, 1e-30f));
  const v2f lc = *pt;
  v2f t2 = z - lc;
  t2 = t2 + t2;
  v2f sw = v2f{0.0f, 0.0f}, swo = v2f{0.0f, 0.0f}, swoo = v2f{0.0f, 0.0f};
#pragma unroll
  for (int m = 0; m < L; m++) {
    const float lm = (float)(2 * m - (L - 1)) * scale;
    const v2f o = v2f{lm, lm} - lc;
    const v2f e = o * (o - t2);
    v2f w;
    w.x = __builtin_amdgcn_exp2f(fmaxf(e.x, 0.0f) * g);
    w.y = __builtin_amdgcn_exp2f(fmaxf(e.y, 0.0f) * g);
    const v2f wo = w * o;
    sw = sw + w;
    swo = swo + wo;
    swoo = __builtin_elementwise_fma(wo, o, swoo);
  }
  v2f r;
  r.x = __builtin_amdgcn_rcpf(sw.x);
  r.y = __builtin_amdgcn_rcpf(sw.y);
  const v2f mo = swo * r;
  const v2f vv = swoo * r - mo * mo;
  *pt = lc + mo;
  *var = fmaxf(vv.x, 0.0f) + fmaxf(vv.y, 0.0f);
}

template <int N, int B, bool F32, bool FB = false>
__global__ __launch_bounds__(kSicT) void sic_pass_kernel(SicPassArgs a) {
  static_assert(!FB || (B > 0 && N > 1), "soft feedback is a form of the soft output at N > 1");
  // FB int8 takes half the symbols per iteration: with the full count 64-QAM at N = 4 needs
  // 256 VGPRs + 20 AGPRs and falls to one wave per SIMD (6.95 ms at C3 x 64 against 4.59 ms
  // with half); FB fp32 fits two waves with the full count and is slower with half (4.98 ms
  // against 5.65 ms)
  constexpr int SC0 = B > 0 ? sic_soft_sc<N, B, F32>() : sic_sc<N>();
  constexpr int SC = (FB && !F32 && SC0 > 1) ? SC0 / 2 : SC0;
  constexpr int NC = (int)sic_c_rows(N);
  constexpr int SLOTS = kSicT / 4 + 1;   // dwords a row's kSicT index bytes can touch
  constexpr int BPS = sic_llr_bps<B, F32>();
  constexpr int RS = sic_llr_rs<B, F32>();
  constexpr int CH = RS / 16;            // 16-byte chunks a row's LLR bytes can touch
  typedef uint32_t v4u __attribute__((ext_vector_type(4)));
  typedef typename std::conditional<F32, uint32_t, uint16_t>::type edge_t;   // a row end's pieces
  // B = 0 never names limg, so it is not allocated: the hard pass's LDS is the index image
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
  const uint32_t n_out = (I.status == 0) ? min(I.n_sym, a.max_out) : 0u;
  const uint64_t mo = a.M_occ;
  // rows of one frame slot: stream t, symbol s at t r_ts + s r_ss
  const uint32_t r_ts = a.symbol_major ? 1u : a.max_out, r_ss = a.symbol_major ? a.N : 1u;
  const uint64_t fbase = (uint64_t)f * a.N * a.max_out * mo + j;   // (frame, carrier) in elements
  // d_llr's address of (frame, tile) mod 2^32: its low 4 bits are all the image needs
  uint32_t lbase = 0;
  if constexpr (B > 0)
    lbase = (uint32_t)(uintptr_t)a.llr + (f * a.N * a.max_out * a.M_occ + j0) * BPS;

  // ---- phase 1, the table prologue: a lane without work gets zero tables, order 0..N-1
  float2 T[N][N], C[NC > 0 ? NC : 1];
  uint32_t ord[N];       // stage k's stream as its element offset pi_k r_ts M_occ, and pi_k
  uint32_t pis[N];
  float wk[N];           // B > 0: stage k's weight llr_scale / max(nu_sic of pi_k, 1e-30)
  float nus[FB ? N : 1]; // FB: nu_sic of pi_k (the weight of a stage k > 0 is per symbol there)
  C[0] = make_float2(0.0f, 0.0f);
  const bool work = lane && s_lo < n_out;
  // a failed solve (or an unsynced slot): NaN in place of z makes every LLR exactly 0
  bool good = false;
  if constexpr (B > 0) good = work && a.ok[(uint64_t)f * mo + j] != 0;
  const float nanv = __builtin_nanf("");
#pragma unroll
  for (int k = 0; k < N; k++) {
    pis[k] = work ? min((uint32_t)a.order[((uint64_t)f * mo + j) * N + k], (uint32_t)(N - 1))
                  : (uint32_t)k;
    ord[k] = pis[k] * r_ts * a.M_occ;
    if constexpr (FB) {
      nus[k] = work ? a.nu[((uint64_t)f * N + pis[k]) * mo + j] : 0.0f;
      if (k == 0) wk[0] = work ? a.llr_scale / fmaxf(nus[0], 1e-30f) : 0.0f;
    } else if constexpr (B > 0) {
      wk[k] = work ? a.llr_scale / fmaxf(a.nu[((uint64_t)f * N + pis[k]) * mo + j], 1e-30f) : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < N; u++)
      T[k][u] = work ? a.T[((uint64_t)f * N * N + k * N + u) * mo + j] : make_float2(0.0f, 0.0f);
  }
#pragma unroll
  for (int e = 0; e < NC; e++)
    C[e] = work ? cneg(a.C[((uint64_t)f * NC + e) * mo + j]) : make_float2(0.0f, 0.0f);

  for (uint32_t s0 = s_lo; s0 < s_hi; s0 += SC) {
    v2f y[SC][N];
#pragma unroll
    for (int q = 0; q < SC; q++)
#pragma unroll
      for (int u = 0; u < N; u++) y[q][u] = v2f{0.0f, 0.0f};
    if (lane) {                         // one masked region for the loads, one for the stages
#pragma unroll
      for (int q = 0; q < SC; q++) {
        if (s0 + q >= n_out) break;     // (uniform)
#pragma unroll
        for (int u = 0; u < N; u++)
          y[q][u] = __builtin_nontemporal_load(reinterpret_cast<const v2f *>(
              a.sym + fbase + ((uint64_t)u * r_ts + (uint64_t)(s0 + q) * r_ss) * mo));
      }
    }
#pragma unroll
    for (int q = 0; q < SC; q++) {
      const uint32_t s = s0 + q;
      if (s >= s_hi || !lane) break;    // (s uniform; idle lanes' image bytes are never stored)
      // ---- phase 2, one symbol's stages (or an erased row)
      const uint64_t sbase = fbase + (uint64_t)s * r_ss * mo;
      const uint32_t lsym = lbase + s * r_ss * a.M_occ * BPS;   // the symbol's rows, mod 2^32
      if (s < n_out) {                  // (uniform)
        // stage k's z and index go straight to the row of its stream pi_k: the order changes
        // slowly along the carriers, so a wave's store still covers whole runs of a row
        v2f yr[N], sh[N], shr[N];
        float var[FB ? N : 1];          // FB: the variance of the symbol stage k cancels
#pragma unroll
        for (int u = 0; u < N; u++) yr[u] = sic_rot(y[q][u]);
#pragma unroll
        for (int k = 0; k < N; k++) {
          v2f z = v2f{0.0f, 0.0f};
#pragma unroll
          for (int u = 0; u < N; u++) z = sic_mac(z, T[k][u], y[q][u], yr[u]);
#pragma unroll
          for (int i = 0; i < k; i++) z = sic_mac(z, C[k * (k - 1) / 2 + i], sh[i], shr[i]);
          const uint32_t idx = sic_slice(z, a.qam, &sh[k]);
          float w = wk[FB ? 0 : k];
          if constexpr (FB) {
            // the error power with the cancelled symbols' variances in it, the weight from it,
            // and the expected symbol in place of the point (the last stage cancels nothing)
            float nuk = nus[k];
#pragma unroll
            for (int i = 0; i < k; i++) {
              const float2 c = C[k * (k - 1) / 2 + i];
              nuk = __builtin_fmaf(__builtin_fmaf(c.x, c.x, c.y * c.y), var[i], nuk);
            }
            if (k > 0) w = a.llr_scale / fmaxf(nuk, 1e-30f);
            if (k < N - 1) sic_soft_symbol<B>(z, nuk, a.qam.scale, &sh[k], &var[k]);
          }
          shr[k] = sic_rot(sh[k]);
          if (a.out_sym)
            __builtin_nontemporal_store(z, reinterpret_cast<v2f *>(a.out_sym + sbase + ord[k]));
          img[(q * N + pis[k]) * kSicT + tid] = (uint8_t)idx;
          if constexpr (B > 0) {
            float lv[2 * B];
            llr_dim<B>(good ? z.x : nanv, a.qam.scale, w, lv);
            llr_dim<B>(good ? z.y : nanv, a.qam.scale, w, lv + B);
            sic_llr_put<B, F32>(limg + (q * N + pis[k]) * RS + ((lsym + ord[k] * BPS) & 15u) +
                                    tid * BPS, lv);
          }
        }
      } else {                          // an erased row: z = 0, idx = 0, LLRs 0
        float lv[B > 0 ? 2 * B : 1];
#pragma unroll
        for (int i = 0; i < 2 * B; i++) lv[i] = 0.0f;
#pragma unroll
        for (int t = 0; t < N; t++) {
          if (a.out_sym)
            __builtin_nontemporal_store(v2f{0.0f, 0.0f}, reinterpret_cast<v2f *>(
                a.out_sym + sbase + (uint64_t)t * r_ts * mo));
          img[(q * N + t) * kSicT + tid] = 0;
          if constexpr (B > 0)
            sic_llr_put<B, F32>(limg + (q * N + t) * RS +
                                    ((lsym + (uint32_t)t * r_ts * a.M_occ * BPS) & 15u) + tid * BPS, lv);
        }
      }
    }
    // hard output: no barrier unless out_idx is set, then one before and one after its drain;
    // soft output: one before the LLR drain, one after the index drain
    const bool drain = B > 0 || a.out_idx;   // (uniform)
    if (drain) __syncthreads();
    const uint32_t rows = min((uint32_t)SC, s_hi - s0) * N;
    // ---- phase 3, the LLR image to d_llr: 16-byte chunks, narrower pieces at a row's ends
    if constexpr (B > 0) {
      const uint32_t nb = nj * BPS;     // a row's LLR bytes in this tile
      for (uint32_t w = tid; w < rows * CH; w += kSicT) {
        const uint32_t r = w / CH, c = w - r * CH;
        const uint32_t q = r / N, t = r - q * N;
        uint8_t *dst = reinterpret_cast<uint8_t *>(a.llr) + (sic_row(a, f, t, s0 + q) * mo + j0) * BPS;
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
    // ---- phase 4, the index image to out_idx: dwords, single bytes at a row's ends
    if (a.out_idx) {                    // (uniform)
      for (uint32_t w = tid; w < rows * SLOTS; w += kSicT) {
        const uint32_t r = w / SLOTS, c = w - r * SLOTS;
        const uint32_t q = r / N, t = r - q * N;
        uint8_t *dst = a.out_idx + sic_row(a, f, t, s0 + q) * mo + j0;   // the row's nj bytes
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
    if (drain) __syncthreads();
  }
}

template <int N, int B, bool F32, bool FB>
static void sic_pass_launch(const SicPassArgs &a, uint32_t nf, hipStream_t s) {
  const dim3 grid((a.M_occ + kSicT - 1) / kSicT, (a.max_out + kSicSB - 1) / kSicSB, nf);
  hipLaunchKernelGGL((sic_pass_kernel<N, B, F32, FB>), grid, dim3(kSicT), 0, s, a);
}

template <int N, bool FB>
static bool sic_pass_bits(const SicPassArgs &a, uint32_t nf, hipStream_t s) {
  switch (a.bits * 2 + (a.f32 ? 1 : 0)) {
    case 0:
      if constexpr (FB) return false;
      else { sic_pass_launch<N, 0, false, false>(a, nf, s); return true; }
    case 2: sic_pass_launch<N, 1, false, FB>(a, nf, s); return true;
    case 3: sic_pass_launch<N, 1, true, FB>(a, nf, s); return true;
    case 4: sic_pass_launch<N, 2, false, FB>(a, nf, s); return true;
    case 5: sic_pass_launch<N, 2, true, FB>(a, nf, s); return true;
    case 6: sic_pass_launch<N, 3, false, FB>(a, nf, s); return true;
    case 7: sic_pass_launch<N, 3, true, FB>(a, nf, s); return true;
    case 8: sic_pass_launch<N, 4, false, FB>(a, nf, s); return true;
    case 9: sic_pass_launch<N, 4, true, FB>(a, nf, s); return true;
    default: return false;
  }
}

bool launch_sic_pass(const SicPassArgs &a, uint32_t n_frames, hipStream_t s) {
  if ((a.llr == nullptr) != (a.bits == 0)) return false;
  if (n_frames == 0 || a.max_out == 0 || a.M_occ == 0) return true;
  if (n_frames > 65535u || (a.max_out + kSicSB - 1) / kSicSB > 65535u) return false;
  if ((uint64_t)a.N * a.max_out * a.M_occ >= 0xFFFFFFFFull) return false;
  if (a.feedback && a.bits == 0) return false;
  // soft feedback: N = 1 has nothing to cancel and is the soft output's instance; N = 3 (no
  // receiver takes it) has none
  if (a.feedback && a.N > 1) {
    switch (a.N) {
      case 2: return sic_pass_bits<2, true>(a, n_frames, s);
      case 4: return sic_pass_bits<4, true>(a, n_frames, s);
      case 8: return sic_pass_bits<8, true>(a, n_frames, s);
      default: return false;
    }
  }
  switch (a.N) {
    case 1: return sic_pass_bits<1, false>(a, n_frames, s);
    case 2: return sic_pass_bits<2, false>(a, n_frames, s);
    case 3: return sic_pass_bits<3, false>(a, n_frames, s);
    case 4: return sic_pass_bits<4, false>(a, n_frames, s);
    case 8: return sic_pass_bits<8, false>(a, n_frames, s);
    default: return false;
  }
}

}  // namespace mimo
