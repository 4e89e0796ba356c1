/*
 * include/mimo_rx.h -- C-ABI of librub_mimo_amd.so, the MI355X (gfx950) OFDM-MIMO receive
 * pipeline. Plain pointers and sizes only; no torch or C++ types cross this boundary.
 *
 * Each entry point replaces a piece of the reference C++ API in /root/reference/mimo/framing.h
 * (cited per function). The C++ facade include/framing.h re-exposes the reference classes
 * rx_beamforming::framesync / framegen on top of these calls, so mimo/main.cc-style callers
 * compile unchanged.
 *
 * Conventions
 *   - complex samples are interleaved fp32 (re, im) = std::complex<float> = gr_complex.
 *   - antenna buffers are planar: one array per antenna (framing.cc:481-484 reads in_buff[s][i]).
 *   - every function returns MIMO_OK (0) or a negative MIMO_ERR_*; nothing calls exit()
 *     (the reference exits at framing.cc:497-499, 1020-1022).
 *   - a handle owns one HIP stream (or the caller's) and is single-caller-thread.
 *   - device pointers (d_*) are HIP device memory (e.g. torch tensor data_ptr()).
 */
#ifndef RUB_MIMO_AMD_MIMO_RX_H
#define RUB_MIMO_AMD_MIMO_RX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIMO_OK 0
#define MIMO_ERR_ARG (-1)
#define MIMO_ERR_HIP (-2)
#define MIMO_ERR_STATE (-3)
#define MIMO_ERR_NOMEM (-4)
#define MIMO_ERR_SCTYPE (-5)
#define MIMO_ERR_UNSUPPORTED (-6)

#define MIMO_MAX_STREAMS 8

/* framesync_states_t, framing.h:34-39 */
enum { MIMO_STATE_SEEK_PLATEAU = 0, MIMO_STATE_SAVE_ACCESS_CODES = 1, MIMO_STATE_WAIT = 2,
       MIMO_STATE_MIMO = 3 };

/* detectors: ZF2 = reference 2x2 adjugate*conj(det) + gain 1/|det|^2 (framing.cc:1344-1367);
 * ZF / MMSE = NxN in fp64, stored fp32; SISO = X/G[rx][tx] on one stream (framing.cc:508-533) */
enum { MIMO_DET_ZF2 = 0, MIMO_DET_ZF = 1, MIMO_DET_MMSE = 2, MIMO_DET_SISO = 3 };

/* per-frame status of the batched path. RESCAN (back-to-back streams only): the re-arm at this
 * frame's origin could not be proven equal to a fresh framesync there (a plateau or window
 * reaching back across the re-arm point); the caller resumes the capture at `origin` as a
 * fresh capture. NONE: an unused frame slot after the end of a stream. */
enum { MIMO_FRAME_OK = 0, MIMO_FRAME_NO_SYNC = 1, MIMO_FRAME_INCOMPLETE = 2,
       MIMO_FRAME_RESCAN = 3, MIMO_FRAME_NONE = 4 };

/* subcarrier types, liquid OFDMFRAME_SCTYPE_{NULL,PILOT,DATA} */
enum { MIMO_SC_NULL = 0, MIMO_SC_PILOT = 1, MIMO_SC_DATA = 2 };

/* Receiver configuration: the framesync constructor arguments (framing.h:189-196) plus the
 * config.h constants the reference reads at compile time (PID_MAX, PLATEAU_THREASHOLD). */
typedef struct mimo_rx_config {
  uint32_t M;                 /* _M, number of subcarriers (power of two, 64..4096) */
  uint32_t cp_len;            /* _cp_len */
  uint32_t num_streams;       /* _num_streams (1..8) */
  uint32_t num_access_codes;  /* _num_access_codes */
  uint32_t pid_max;           /* PID_MAX (config.h:92): data symbols per frame window */
  const uint8_t *p;           /* _p, M subcarrier types; copied */
  const uint8_t *s0_bits;     /* M draws msequence_generate_symbol(ms_S0,1)&1 (framing.cc:1075) */
  const uint8_t *s1_bits;     /* num_streams*num_access_codes*M draws, stream-major
                                 (framing.cc:1240, one generator per stream) */
  int32_t detector;           /* MIMO_DET_* (INVERT_CHANNEL, config.h:102) */
  float noise_var;            /* MMSE sigma^2; < 0: estimate from the training residuals */
  int32_t keep_identity_bias; /* 1 = reference: G starts at identity (framing.cc:309-311) */
  uint32_t siso_tx, siso_rx;  /* set_siso_tx / set_siso_rx (framing.h:211-212) */
  double plateau_threshold;   /* PLATEAU_THREASHOLD (config.h:87), 0.95 */
  uint32_t qam_order;         /* square Gray QAM for the fused demap/EVM stage (4..256) */
  int32_t cfo_correct;        /* batched path, opt-in (absent from the reference: FIXME at
                                 framing.cc:486): 1 = estimate each synced frame's CFO (eps0
                                 from the S0 half-period correlation ending at its trigger,
                                 delta from the data symbols' cyclic prefixes, both summed
                                 over the antennas) and derotate before search, LS and decode
                                 (in the loads where the fused search and the streaming
                                 decode run, else into a device scratch copy; the caller's
                                 capture is not modified); where the streaming decode takes
                                 the batch with reference indices from HBM, each symbol's
                                 common phase is also measured from its own decisions and
                                 removed (mimo_rx_get_cfo_mode). The stages are restated in
                                 oracle/mimo_ref.c (cfo_mode). 0 = off (the reference's
                                 behaviour). Scratch-path batches with frames_per_capture > 1
                                 are refused with MIMO_ERR_UNSUPPORTED. */
} mimo_rx_config;

typedef struct mimo_rx mimo_rx;

/* callback, framing.h:30-31: eq[t] points at M_occ equalised symbols of stream t, valid
 * only during the call (framing.cc:587). */
typedef void (*mimo_rx_symbol_cb)(const float *const *eq, uint32_t n_streams, uint32_t m_occ,
                                  void *user);

/* framesync::framesync (framing.cc:268-436). hip_stream: hipStream_t or NULL (own stream). */
int mimo_rx_create(const mimo_rx_config *cfg, void *hip_stream, mimo_rx **out);
/* framesync::~framesync (framing.cc:916-943) */
int mimo_rx_destroy(mimo_rx *h);
/* the mimo_callback argument of the constructor (framing.h:196) */
int mimo_rx_set_callback(mimo_rx *h, mimo_rx_symbol_cb cb, void *user);
/* framesync::execute (framing.cc:471-506): host planar complex64 input, any chunking;
 * state persists across calls; *state_out receives the framesync_states_t. */
int mimo_rx_execute(mimo_rx *h, const float *const *iq_planar, uint32_t n_ant, uint64_t n,
                    int32_t *state_out);
/* framesync::reset (framing.cc:461-464): back to STATE_SEEK_PLATEAU */
int mimo_rx_reset(mimo_rx *h);
int mimo_rx_set_siso(mimo_rx *h, uint32_t siso_tx, uint32_t siso_rx);
int mimo_rx_get_state(const mimo_rx *h, int32_t *state);
/* get_sync_index / get_num_samples_processed / get_plateau_start|end (framing.h:200-206) */
int mimo_rx_get_sync_index(const mimo_rx *h, uint64_t *out);
int mimo_rx_get_num_samples_processed(const mimo_rx *h, uint64_t *out);
int mimo_rx_get_plateau(const mimo_rx *h, uint32_t stream, uint64_t *start, uint64_t *end);
/* get_G (framing.h:201): [M][N][N] complex64 ([sc][rx][tx]); W likewise ([sc][out][rx]) */
int mimo_rx_get_G(mimo_rx *h, float *G);
int mimo_rx_get_W(mimo_rx *h, float *W);
/* normalize_gain (framing.cc:404-409), M_occ floats */
int mimo_rx_get_gain(mimo_rx *h, float *gain);
int mimo_rx_get_noise_var(mimo_rx *h, float *out);
/* corr_indices [N][N*nac] (window index, framing.cc:737) and s0_corr_index [N] (:720) */
int mimo_rx_get_corr(mimo_rx *h, uint32_t *corr_idx, uint32_t *s0_idx);
int mimo_rx_get_m_occ(const mimo_rx *h, uint32_t *m_occ);

/* ---------------- batched device-resident frames (the hot path the bench times) ---------
 * n_frames independent captures, each num_streams planar antenna arrays of frame_len
 * complex64 at d_iq + (f*num_streams + s)*stride (complex units). Every frame runs the whole
 * receive chain (S&C + plateau, access-code search, LS, weights, decode, demap, EVM) with
 * no host synchronisation.
 *
 * frames_per_capture = K > 1 makes each capture a stream of back-to-back frames (a live
 * 20 MS/s stream, BASELINE config C5): frame k + 1 is what a fresh framesync (framing.cc:268)
 * finds in the samples after frame k, i.e. starting at origin
 *   r_{k+1} = r_k + get_num_samples_processed()   (framing.cc:471-506, r_0 = 0).
 * The reference itself stops at STATE_MIMO and its reset() keeps stale filter state
 * (framing.cc:461-464, 494-496), so this re-arm is defined as that fresh construction. Frame
 * slots are then [capture][K]: outputs, results and d_ref_idx rows are per slot. */
typedef struct mimo_batch {
  const void *d_iq;
  uint64_t stride;        /* complex samples between antenna arrays (>= frame_len) */
  uint64_t frame_len;
  uint32_t n_frames;
  uint32_t max_out_syms;  /* symbols kept per frame (main.cc keeps PID_MAX, main.cc:106) */
  void *d_out_sym;        /* [n_frames][N][max_out_syms][M_occ] complex64 (out_layout), or NULL */
  void *d_out_idx;        /* same layout, uint8 demapped index, or NULL */
  int32_t ref_mode;       /* 0: decision-directed EVM; 1: d_ref_idx; 2: synthetic hash */
  const void *d_ref_idx;  /* ref_mode 1: same layout as d_out_idx */
  uint64_t ref_seed;      /* ref_mode 2: seed of mimo_synth_frames */
  uint64_t frame_id0;     /* ref_mode 2: frame id of frame 0 */
  uint32_t frames_per_capture;  /* 0 or 1: one frame per capture; K > 1: back-to-back streams */
  uint32_t ref_stride;          /* entries per capture in d_ref_starts (0: frames_per_capture) */
  /* streams with ref_mode 1/2, or NULL: [n_frames][ref_stride] capture sample where each
   * transmitted frame starts (UINT64_MAX after the last). A decoded frame whose sync index
   * lies in [start_j, start_{j+1}) takes reference row / frame id capture*ref_stride + j;
   * NULL: its slot. */
  const uint64_t *d_ref_starts;
  /* MIMO_SAMPLE_FC32 (0): d_iq holds complex64. MIMO_SAMPLE_SC16 (1): d_iq holds the UHD sc16
   * wire format (interleaved int16 I/Q, mimo/config.h:52; 4 bytes per sample, strides and
   * lengths still in samples), read as float(i16) * sc16_scale -- bit-identical to widening
   * with mimo_ingest_sc16 first. The S&C, fused search + LS and streaming decode kernels read
   * it directly (C3-type geometries); other configurations widen it into an internal buffer. */
  uint32_t sample_format;
  float sc16_scale;
  /* MIMO_LAYOUT_STREAM_MAJOR (0): d_out_sym, d_out_idx and d_ref_idx are
   * [n_frames][N][max_out_syms][M_occ]. MIMO_LAYOUT_SYMBOL_MAJOR (1): [n_frames][max_out_syms][N][M_occ],
   * each symbol's N stream rows together -- the order the reference's callback hands them out in
   * (one call per symbol with the N stream arrays, framing.cc:587) -- and a sequential write
   * stream per decode workgroup (fewer concurrent HBM write streams: the C3 decode ~7% faster) */
  uint32_t out_layout;
  /* MIMO_STAGES_ALL (0): the whole receive chain. MIMO_STAGES_FRONT (1): S&C, plateau, search,
   * LS and weights only; MIMO_STAGES_DECODE (2): the replay decode and EVM only, of the batch
   * the same handle last ran MIMO_STAGES_FRONT on (same arguments). The two halves may run on
   * different streams (the caller orders them with events), e.g. batch i's decode on one CU
   * partition beside batch i+1's front stages on another handle and partition. Not with
   * cfo_correct. */
  uint32_t stages;
} mimo_batch;

enum { MIMO_SAMPLE_FC32 = 0, MIMO_SAMPLE_SC16 = 1 };
enum { MIMO_LAYOUT_STREAM_MAJOR = 0, MIMO_LAYOUT_SYMBOL_MAJOR = 1 };
enum { MIMO_STAGES_ALL = 0, MIMO_STAGES_FRONT = 1, MIMO_STAGES_DECODE = 2 };

/* Positions are those a framesync started at `origin` reports (origin 0 for one frame per
 * capture): add origin for the capture sample. */
typedef struct mimo_frame_result {
  int32_t status;                          /* MIMO_FRAME_* */
  uint32_t n_sym;                          /* decode callbacks (PID+2 in the reference) */
  uint64_t trigger;                        /* sample where the plateau rule fired */
  uint64_t sync_index;
  uint64_t num_samples_processed;          /* as one framesync::execute over the frame */
  uint64_t plateau_start[MIMO_MAX_STREAMS];
  uint64_t plateau_end[MIMO_MAX_STREAMS];
  float noise_var;
  float cfo_eps;                           /* cfo_correct: estimated CFO, subcarrier spacings */
  double evm_num[MIMO_MAX_STREAMS];        /* sum |y - s|^2 over kept symbols */
  double evm_den[MIMO_MAX_STREAMS];        /* sum |s|^2 */
  uint64_t errors[MIMO_MAX_STREAMS];       /* symbol errors (ref_mode 1/2) */
  uint64_t origin;                         /* capture sample where this frame's framesync began */
  uint32_t capture;                        /* capture (stream) index */
  uint32_t ref_frame;                      /* reference row / frame id offset used for the EVM */
} mimo_frame_result;

int mimo_rx_process_batch(mimo_rx *h, const mimo_batch *b, void *hip_stream);
/* copies the last batch's per-frame results to host (synchronises the stream); n_frames
 * counts frame slots (captures x frames_per_capture) */
int mimo_rx_batch_results(mimo_rx *h, mimo_frame_result *out, uint32_t n_frames);
/* per-frame detail of the last batch, host copies: corr [F][N][N*nac], G [F][M][N][N] */
int mimo_rx_batch_corr(mimo_rx *h, uint32_t *corr_idx, uint32_t *s0_idx, uint32_t n_frames);
int mimo_rx_batch_G(mimo_rx *h, float *G, uint32_t n_frames);
int mimo_rx_batch_W(mimo_rx *h, float *W, uint32_t n_frames);
/* normalize_gain of every frame slot, [n_frames][M_occ] floats (1 except with MIMO_DET_ZF2 and
 * MIMO_DET_SISO at 2x2, where it is 1 / |det G|^2; mimo_rx_get_gain reads slot 0 only); rows of
 * slots that did not sync are not meaningful; a host copy, synchronises */
int mimo_rx_batch_gain(mimo_rx *h, float *gain, uint32_t n_frames);

/* ---------------- soft output (absent from the reference: main.cc slices to a hard index) ----
 * An opt-in pass after mimo_rx_process_batch (MIMO_STAGES_ALL or _DECODE) over that batch's
 * equalised symbols; the batch itself launches nothing for it. Both calls read the handle's G,
 * W, gain and per-frame noise variance of the batch it last ran; they work with cfo_correct
 * and with frames_per_capture > 1 (frame slots as mimo_rx_batch_results counts them).
 *
 * Post-detection MSE of output stream t on occupied carrier j (subcarrier k) of frame f, the
 * predicted E|y_t - s_t|^2 for X = G s + n, n ~ CN(0, s2 I), s2 = the frame's noise_var, and the
 * decode's y_t = g_k sum_r W[t][r] X_r:
 *   nu[f][t][j] = g_k^2 s2 sum_r |W[t][r]|^2 + sum_u |g_k sum_r W[t][r] G[r][u] - delta_tu|^2
 * (noise enhancement, plus residual inter-stream interference and the MMSE bias as noise).
 *
 * Max-log LLRs of a square Gray QAM of order L^2, b = log2 L bits per dimension, 2b values per
 * symbol: value i belongs to bit i of the demapped index counted from its most significant bit
 * (the index is (gray(mI) << b) | gray(mQ)), so values 0..b-1 depend on Re y and b..2b-1 on
 * Im y. With levels l_m = (2m - (L-1)) scale and x the part of y the bit depends on,
 *   LLR_i = llr_scale (min_{m: bit_i(gray m) = 1} (x - l_m)^2
 *                      - min_{m: bit_i(gray m) = 0} (x - l_m)^2) / max(nu, 1e-30)
 * positive = bit 0 more likely, taken on y as delivered (not unbiased), so a non-zero LLR's
 * sign is the matching bit of d_out_idx. MIMO_LLR_F32 stores the value, MIMO_LLR_I8
 * clamp(rintf(value), -127, 127) (round half to even). A NaN y gives 0, and so does every row
 * the decode does not write (frames with status != MIMO_FRAME_OK, symbols >= min(n_sym,
 * max_out_syms)): the whole d_llr is defined after the call.
 *
 * MIMO_DET_SISO returns MIMO_ERR_UNSUPPORTED: the handle's W is not the SISO weight
 * (the SISO decode divides by G[rx][tx]), and one stream's LLRs are left to a later change. */
enum { MIMO_LLR_I8 = 0, MIMO_LLR_F32 = 1 };
typedef struct mimo_soft_demap {
  const void *d_sym;      /* the last batch's d_out_sym (same out_layout, max_out_syms) */
  void *d_llr;            /* [d_out_sym's rows][M_occ][2b] int8 or float */
  uint32_t n_frames;      /* frame slots, as mimo_rx_batch_results counts them */
  uint32_t max_out_syms;
  uint32_t out_layout;    /* MIMO_LAYOUT_* of d_sym; d_llr follows it */
  uint32_t format;        /* MIMO_LLR_* */
  float llr_scale;        /* finite, > 0 */
} mimo_soft_demap;
/* Asynchronous on hip_stream (NULL: the handle's), no host synchronisation; the caller orders
 * it after the batch that wrote d_sym. Allocates only when the slot count grows, so it can be
 * captured into a graph after one warm-up call. d_sym and d_llr 16-byte aligned; n_frames and
 * max_out_syms must equal the last batch's (MIMO_ERR_ARG); MIMO_ERR_STATE before any batch. */
int mimo_rx_soft_demap(mimo_rx *h, const mimo_soft_demap *a, void *hip_stream);
/* host copy of nu, [n_frames][N][M_occ] floats; rows of unsynced slots are 0; synchronises */
int mimo_rx_batch_mse(mimo_rx *h, float *mse, uint32_t n_frames);

/* ---------------- ordered MMSE-SIC detection (absent from the reference: its detectors are
 * linear) ----
 * An opt-in pass after mimo_rx_process_batch over that batch's equalised symbols, like the soft
 * output: the batch launches nothing for it, and the pass never modifies d_sym, the batch's
 * d_out_idx, its results or the handle's G / W. It works with cfo_correct, with
 * frames_per_capture > 1 and after MIMO_STAGES_DECODE.
 *
 * Per synced frame f and occupied carrier j (subcarrier k): G the frame's estimate [rx][tx], s2
 * its noise_var (as mimo_rx_batch_results reports it), Q = G^H G, lambda = s2 for MIMO_DET_MMSE
 * and 0 for MIMO_DET_ZF (and MIMO_DET_ZF2 at N = 2), R = Q + lambda I. The linear decode
 * delivered y = g W X with g W = (Q + lambda I)^-1 G^H, so R y = G^H X: the matched-filter
 * statistic comes back from y without the capture and without inverting W.
 *
 * N stages k = 0..N-1; S the undetected streams (all at k = 0), pi_0..pi_(k-1) the detected:
 *   1. E = (Q[S,S] + s2 I)^-1, in fp64.
 *   2. pi_k = the stream of S with the smallest real diagonal entry of E, ties to the lowest
 *      stream index.
 *   3. r = that row of E, beta = 1 - s2 E[pi_k][pi_k].
 *   4. T[k][u] = (sum_{v in S} r_v R[v][u]) / beta, u = 0..N-1;
 *      C[k][i] = (sum_{v in S} r_v Q[v][pi_i]) / beta, i < k   (fp64, stored as fp32).
 *   5. nu_sic of stream pi_k = (1 - beta) / beta, the unbiased MMSE estimate's error power
 *      (0 when s2 = 0).
 *   6. per symbol: z_(pi_k) = sum_u T[k][u] y_u - sum_{i<k} C[k][i] s^_(pi_i); idx = the
 *      decode's own slicer of z_(pi_k), s^_(pi_k) = the constellation point of idx.
 * With MMSE, stage 0 is z = y_(pi_0) / beta_0, the unbiased linear output. A carrier whose fp64
 * solve fails at any stage gets all-zero tables, order 0..N-1 and nu_sic 0 (as the linear
 * path's W). Rows the decode does not write (frames with status != MIMO_FRAME_OK, symbols >=
 * min(n_sym, max_out_syms)) get z = 0 and idx = 0: both outputs are fully defined after the
 * call. A NaN in y gives a NaN z and whatever the slicer gives (level 0).
 *
 * MIMO_DET_SISO, and MIMO_DET_ZF2 at N != 2 (W is the identity there), return
 * MIMO_ERR_UNSUPPORTED. */
typedef struct mimo_sic_detect {
  const void *d_sym;      /* the last batch's d_out_sym (same out_layout, max_out_syms) */
  void *d_out_sym;        /* z, complex64, same shape and layout as d_sym, or NULL */
  void *d_out_idx;        /* uint8 demapped index of z, same layout, or NULL (not both NULL) */
  uint32_t n_frames;      /* frame slots, as mimo_rx_batch_results counts them */
  uint32_t max_out_syms;
  uint32_t out_layout;    /* MIMO_LAYOUT_* of the last batch */
} mimo_sic_detect;
/* Asynchronous on hip_stream (NULL: the handle's), no host synchronisation; the caller orders
 * it after the batch that wrote d_sym. Allocates only when the slot count grows, so it can be
 * captured into a graph after one warm-up call. Pointers 16-byte aligned; d_out_sym must not
 * overlap d_sym; n_frames, max_out_syms and out_layout must equal the last batch's
 * (MIMO_ERR_ARG); MIMO_ERR_STATE before any batch. */
int mimo_rx_sic_detect(mimo_rx *h, const mimo_sic_detect *a, void *hip_stream);
/* host copies of the last batch's detection order pi, [n_frames][M_occ][N] uint8, and of
 * nu_sic, [n_frames][N][M_occ] floats indexed by stream; they work after any batch, with or
 * without a detect call; rows of unsynced slots are 0; both synchronise */
int mimo_rx_sic_order(mimo_rx *h, uint8_t *order, uint32_t n_frames);
int mimo_rx_sic_mse(mimo_rx *h, float *mse, uint32_t n_frames);

/* ---------------- soft-output SIC: per-bit LLRs from the ordered MMSE-SIC pass ----
 * One fused launch that runs the stages of mimo_rx_sic_detect and writes the max-log LLRs of
 * every stage's z, weighted by that stage's nu_sic, without z going through memory. Opt-in and
 * after the batch like the two passes it combines; the same conditions and side-effect rules as
 * mimo_rx_sic_detect hold.
 *
 * The order, the tables T and C, z, idx and s^ are exactly steps 1-6 above; every stage still
 * cancels its hard decision. For stream pi_k of a row the decode wrote, the 2b values are
 *   LLR_i = llr_scale delta_i(z_(pi_k)) / max(nu_sic[f][pi_k][j], 1e-30)
 * with delta_i the soft output's numerator: min over the levels with bit i = 1 minus min over
 * the levels with bit i = 0 of (x - l_m)^2, bit i counted from the index's most significant
 * bit, values 0..b-1 from x = Re z and b..2b-1 from x = Im z, the levels qam_point's fp32
 * levels; positive = bit 0 more likely. z is unbiased, so nothing is unbiased again, and a
 * non-zero LLR's sign is the matching bit of this call's idx. MIMO_LLR_F32 stores the fp32
 * value, MIMO_LLR_I8 clamp(rintf(value), -127, 127) of that same fp32 value. A NaN z gives 0.
 *
 * d_llr is fully defined after the call. These get 0: rows the decode did not write (frames
 * with status != MIMO_FRAME_OK, symbols >= min(n_sym, max_out_syms)), and every carrier whose
 * fp64 solve failed (all-zero tables). The latter is not the good carrier with nu_sic = 0
 * because s2 = 0: that one takes the 1e-30 floor.
 *
 * nu_sic is the error power of stage k's estimate when the earlier decisions were right
 * (perfect cancellation): error propagation is not in the weight, so the LLRs of the later
 * stages are optimistic where an earlier stage decided wrongly. mimo_rx_sic_soft_fb below
 * carries that into the weight: call it for calibrated LLRs. */
typedef struct mimo_sic_soft {
  const void *d_sym;      /* the last batch's d_out_sym */
  void *d_llr;            /* [d_sym's rows][M_occ][2b] int8 or float; required */
  void *d_out_sym;        /* z, as mimo_sic_detect.d_out_sym, or NULL */
  void *d_out_idx;        /* uint8 index of z, as mimo_sic_detect.d_out_idx, or NULL */
  uint32_t n_frames, max_out_syms, out_layout;
  uint32_t format;        /* MIMO_LLR_I8 / MIMO_LLR_F32 */
  float llr_scale;        /* finite, > 0 */
} mimo_sic_soft;
/* Asynchronous on hip_stream (NULL: the handle's), no host synchronisation; the caller orders
 * it after the batch that wrote d_sym. Allocates only when the slot count grows, so it can be
 * captured into a graph after one warm-up call. Every pointer 16-byte aligned; d_out_sym must
 * not overlap d_sym; n_frames, max_out_syms and out_layout must equal the last batch's; a bad
 * format, out_layout or llr_scale and a null d_sym or d_llr are MIMO_ERR_ARG too;
 * MIMO_ERR_STATE before any batch; MIMO_DET_SISO, and MIMO_DET_ZF2 at N != 2, return
 * MIMO_ERR_UNSUPPORTED. */
int mimo_rx_sic_soft(mimo_rx *h, const mimo_sic_soft *a, void *hip_stream);

/* ---------------- soft-feedback SIC: expected-symbol cancellation, calibrated LLRs ----
 * mimo_rx_sic_soft with two changes: a stage cancels the posterior mean of the earlier symbols
 * instead of their hard decisions, and its weight carries their posterior variance. The same
 * argument struct, conditions, errors and side-effect rules as mimo_rx_sic_soft; the order pi,
 * T, C and nu_sic are steps 1-5 above, unchanged; mimo_rx_sic_detect stays the hard detector.
 *
 * l_m the L fp32 levels of qam_point. Per symbol, stage k = 0..N-1:
 *   z_k   = sum_u T[k][u] y_u - sum_{i<k} C[k][i] sbar_i
 *   nu_k  = nu_sic[pi_k] + sum_{i<k} |C[k][i]|^2 v_i
 *   idx_k = the decode's own slicer of z_k
 *   LLR_i = llr_scale delta_i(z_k) / max(nu_k, 1e-30)     (delta, formats, NaN -> 0 as above)
 *   for x = Re z_k and x = Im z_k: p_m ~ exp(-(x - l_m)^2 / max(nu_k, 1e-30)) over the L levels
 *     (the complex error power nu_k is nu_k / 2 per real dimension), normalised to sum 1;
 *     mean = sum_m p_m l_m, variance = max(sum_m p_m l_m^2 - mean^2, 0)
 *   sbar_k = (mean of Re) + j (mean of Im), v_k = (variance of Re) + (variance of Im)
 * (the last stage needs neither). The posterior is evaluated relative to the slicer's level l_c
 * of x: with t = x - l_c and o_m = l_m - l_c, w_m = exp(-max(o_m (o_m - 2 t), 0) / nu_k),
 * mean = l_c + sum w o / sum w, variance = sum w o^2 / sum w - (sum w o / sum w)^2. That is the
 * same posterior (l_c is the nearest level, so the exponent is >= 0 but for the slicer's
 * rounding at a boundary); no weight exceeds 1 and the slicer's own is 1, so it neither
 * overflows nor gives 0/0 for any z or nu. As nu_k -> 0, sbar_k is the hard point and v_k = 0.
 *
 * Stage 0 cancels nothing: its z, idx and LLRs are mimo_rx_sic_soft's bit for bit, and at N = 1
 * the whole call is. Failed-solve carriers (all-zero tables, LLRs 0), erased rows (z = 0, idx =
 * 0, LLRs 0) and a NaN y (every stage's z is NaN) are as in mimo_rx_sic_soft. Instances exist
 * for N = 1, 2, 4, 8; N = 3 returns MIMO_ERR_UNSUPPORTED. The weight is calibrated for the
 * linear filter at hand: T and C are not recomputed from the residual variances. */
int mimo_rx_sic_soft_fb(mimo_rx *h, const mimo_sic_soft *a, void *hip_stream);

/* ---------------- soft-input MMSE-PIC: decoder priors into the detector ----
 * The detector of an iterative receiver: it takes a-priori LLRs of the coded bits (such as
 * mimo_fec_siso's MIMO_FEC_SISO_EXT output, which sits at the row positions of a soft pass's
 * d_llr), turns them into each stream's expected symbol and variance, cancels every other
 * stream's expected symbol (parallel interference cancellation), filters what is left with the
 * MMSE filter of the residual covariance, recomputed per carrier and symbol, and writes extrinsic
 * per-bit LLRs in the usual row layout. Opt-in and after the batch; unless stated otherwise the
 * conditions, side-effect rules, shape checks and erased rows of mimo_rx_sic_soft apply, and it
 * works with cfo_correct, with frames_per_capture > 1 and after MIMO_STAGES_DECODE.
 *
 * Per synced frame and occupied carrier, G, s2, Q = G^H G, lambda and R = Q + lambda I are as in
 * the SIC section, and m = R y is the matched-filter statistic recovered from the decode's y.
 * Per written symbol, for stream t = 0..N-1:
 *   1. natural prior LLRs lam_i = prior[t][i] / prior_scale, from the plain int8 value (-128
 *      means -128); positive = bit 0; bit order as the soft passes write it: values 0..b-1
 *      belong to Re, most significant bit first, values b..2b-1 to Im.
 *   2. prior moments per dimension over the L levels l_m of qam_point:
 *      P(m) ~ exp(sum_i (bit_i(gray m) ? -lam_i / 2 : +lam_i / 2)), mean = sum P l,
 *      variance = max(sum P l^2 - mean^2, 0); sbar_t = mean(Re) + j mean(Im),
 *      v_t = variance(Re) + variance(Im).
 *   3. A = Q diag(v) + s2 I, r = m - Q sbar, mu_t = (A^-1 Q)[t][t] (real).
 *   4. z^_t = (A^-1 r)_t / mu_t + sbar_t, nu_t = 1 / mu_t - v_t.
 *   5. idx_t = the decode's slicer of z^_t; LLR_i = llr_scale delta_i(z^_t) / max(nu_t, 1e-30),
 *      with delta, the formats, the rounding and NaN -> 0 exactly those of mimo_rx_sic_soft.
 * Steps 3-4 are the unbiased MMSE estimate of s_t from X - sum_{u != t} g_u sbar_u, whose
 * residual covariance is G diag(v, with v_t := 1) G^H + s2 I, brought into the N x N domain by
 * the push-through identity. Stream t's own priors enter neither z^_t nor nu_t: the output is
 * extrinsic and can go straight back into the decoder.
 *
 * The moments are evaluated in the factorised form of the reflected Gray map (b exponentials per
 * dimension, equal to the sum over the levels), and the solve is an elimination of A in fp32
 * without pivoting: A is a column scaling of the Hermitian positive definite Q + s2 diag(v)^-1.
 *
 * Limits: d_prior NULL or all zero gives sbar = 0, v = 1 and every stream's unbiased linear MMSE
 * output with nu_t = 1 / beta_t - 1 (for stream pi_0 that is mimo_rx_sic_soft's stage 0, as a
 * mathematical identity, not a bitwise one; NULL is bitwise the zero buffer). Certain priors
 * give nu_t = s2 / Q[t][t], the matched-filter bound. At N = 1 the priors cancel out of the
 * result and are not read.
 *
 * These get LLR 0, z^ 0 and idx 0, and their priors are never read: rows the decode did not
 * write, every carrier whose Q is not finite, and every frame with noise_var <= 0 (A can be
 * singular there).
 *
 * MIMO_ERR_ARG: mimo_rx_sic_soft's cases, a prior_scale that is not finite and positive, a
 * d_prior that is not 16-byte aligned or overlaps d_llr. MIMO_ERR_UNSUPPORTED: MIMO_DET_SISO,
 * MIMO_DET_ZF2 at N != 2, N = 3, and N = 8: a per-symbol 8 x 8 solve does not fit the register
 * file next to the rest of the pass. Instances exist for N = 1, 2, 4, b = 1..4, both formats. */
typedef struct mimo_pic_soft {
  const void *d_sym;      /* the last batch's d_out_sym */
  const void *d_prior;    /* int8 a-priori LLRs, shape and layout of d_llr (MIMO_LLR_I8), or NULL = all 0 */
  void *d_llr;            /* extrinsic LLRs, [d_sym's rows][M_occ][2b] int8 or float; required */
  void *d_out_sym;        /* z^, complex64, as mimo_sic_soft.d_out_sym, or NULL */
  void *d_out_idx;        /* the decode's slicer of z^, or NULL */
  uint32_t n_frames, max_out_syms, out_layout;
  uint32_t format;        /* MIMO_LLR_I8 / MIMO_LLR_F32, of d_llr */
  float llr_scale;        /* of d_llr; finite, > 0 */
  float prior_scale;      /* natural prior LLR = value / prior_scale; finite, > 0 */
} mimo_pic_soft;
/* Asynchronous on hip_stream (NULL: the handle's), no host synchronisation; allocates only when
 * the slot count grows, so it can be captured into a graph after one warm-up call. */
int mimo_rx_pic_soft(mimo_rx *h, const mimo_pic_soft *a, void *hip_stream);

/* ---------------- layered tree search (LORD): near-ML soft detection ----
 * The one detector here that searches the lattice and does not only filter it: for every target
 * stream t it enumerates all L^2 values of s_t, detects the other N - 1 streams by hard
 * successive cancellation under each value, and takes max-log LLRs of s_t's bits over those L^2
 * candidate vectors. Every bit has both hypotheses in the list (no clipping); at N = 2 the
 * result is exactly the max-log ML detector's. No priors and no z output. Opt-in and after the
 * batch; unless stated otherwise the conditions, side-effect rules, shape checks, erased rows,
 * alignment, asynchrony and graph-capture rules of mimo_rx_sic_soft apply, and it works with
 * cfo_correct, with frames_per_capture > 1 and after MIMO_STAGES_DECODE.
 *
 * Per synced frame and occupied carrier, as in the SIC and PIC sections: G and s2 = noise_var;
 * Q = G^H G, accumulated in fp64 and stored as fp32; lam = s2 for MMSE, 0 for ZF and for ZF2 at
 * N = 2; m = (Q + lam I) y, the matched-filter statistic recovered from the decode's y. The
 * metric of a symbol vector s is D(s) = s^H Q s - 2 Re(s^H m), which is |X - G s|^2 up to a
 * constant. Per target stream t = 0..N-1:
 *   1. Order. The other streams by decreasing Q[u][u] are o_0, o_1, ...; the order is decided on
 *      the stored fp32 values and ties go to the lower index. Permutation
 *      p = (o_(N-2), ..., o_0, t): the target sits in the last position, o_0 is detected first.
 *   2. Factor. U upper triangular with a real positive diagonal, U^H U = P (Q + r I) P^T,
 *      computed per carrier and frame in fp64 from the stored Q and stored as fp32. r = s2
 *      whatever the detector, like the PIC pass's A; at N = 2, r = 0: there the one sliced
 *      stream has to be the exact minimiser of D for the result to be the max-log ML
 *      detector's, and with r = s2 the chain would slice the biased estimate, the minimiser of
 *      D(s) + s2 |s|^2 (equal for QPSK, not for 16-QAM and up).
 *   3. Candidates. Per written symbol yt = U^-H (P m). Each of the L^2 values c of s_t, in the
 *      index order of the decode's slicer, is a candidate: s_(N-1) = c, and for k = N-2 .. 0
 *      e_k = (yt_k - sum_{j>k} U_kj s_j) / U_kk, s_k = qam_point(the decode's slicer of e_k).
 *   4. Metric. D_c = sum_k |yt_k - sum_{j>=k} U_kj s_j|^2 - r sum_k |s_k|^2, which is
 *      D(s) + |yt|^2 for the completed vector; the residuals come out of step 3.
 *   5. LLR_i(t) = llr_scale (min_{c: bit_i(c) = 1} D_c - min_{c: bit_i(c) = 0} D_c) / s2; bit
 *      order, positive = bit 0, the formats MIMO_LLR_I8 / MIMO_LLR_F32, the rounding and
 *      NaN -> 0 are exactly mimo_rx_sic_soft's, and the int8 output is bitwise the rounded and
 *      clamped fp32 output.
 *   6. idx_t = the candidate c with the smallest D_c; the lowest c wins a tie.
 * At N = 1 there is no chain: D_c = Q |c|^2 - 2 Re(c* m), the max-log LLRs of z = m / Q with
 * error power s2 / Q.
 *
 * These get LLR 0 and idx 0, and nothing of them is read: rows the decode did not write,
 * carriers whose Q or U is not finite, and frames with noise_var <= 0 or not finite.
 *
 * MIMO_ERR_ARG: mimo_rx_sic_soft's cases. MIMO_ERR_UNSUPPORTED (mimo_last_error names the pass):
 * MIMO_DET_SISO, MIMO_DET_ZF2 at N != 2, N = 3 and N = 8. Instances exist for N = 1, 2, 4,
 * b = 1..4, both layouts, both formats. */
typedef struct mimo_lord_soft {
  const void *d_sym;      /* the last batch's d_out_sym */
  void *d_llr;            /* LLRs, [d_sym's rows][M_occ][2b] int8 or float; required */
  void *d_out_idx;        /* the best candidate's index per (row, carrier), or NULL */
  uint32_t n_frames, max_out_syms, out_layout;
  uint32_t format;        /* MIMO_LLR_I8 / MIMO_LLR_F32, of d_llr */
  float llr_scale;        /* of d_llr; finite, > 0 */
} mimo_lord_soft;
/* Asynchronous on hip_stream (NULL: the handle's), no host synchronisation; allocates only when
 * the slot count grows, so it can be captured into a graph after one warm-up call. */
int mimo_rx_lord_soft(mimo_rx *h, const mimo_lord_soft *a, void *hip_stream);

/* ---------------- channel code over the int8 LLR rows: K = 7 Viterbi decoder (absent from the
 * reference: it stops at modem_demodulate and has no channel code) ----
 * An opt-in pass over a buffer of int8 LLRs such as a soft pass's d_llr (MIMO_LLR_I8); it needs
 * no mimo_rx handle and the batch launches nothing for it. Integer arithmetic throughout: the
 * output is defined to the bit (rub_mimo_amd/fec.py is this text as numpy).
 *
 * Encoder: the 802.11 mother code, K = 7, generators 133 / 171 octal. Info bits
 * u_0..u_(n_info-1), then six zero tail bits: T = n_info + 6 trellis steps, u_t = 0 for t < 0;
 * the trellis starts and ends in the all-zero state.
 *   A_t = u_t ^ u_(t-2) ^ u_(t-3) ^ u_(t-5) ^ u_(t-6)     (133)
 *   B_t = u_t ^ u_(t-1) ^ u_(t-2) ^ u_(t-3) ^ u_(t-6)     (171)
 * Rates (the 802.11 puncturing patterns): MIMO_FEC_R12 sends every A_t and B_t; MIMO_FEC_R23 has
 * period 2 and keeps A in steps {1,1}, B in {1,0}; MIMO_FEC_R34 has period 3 and keeps A in
 * {1,1,0}, B in {1,0,1} (sent order A1 B1 A2 B3). Sent order: for t = 0..T-1, A_t if kept, then
 * B_t if kept: coded bits k = 0..n_tx-1, so n_tx is 2T, floor(T/2) 3 + (T mod 2) 2 and
 * floor(T/3) 4 + {0,2,3}[T mod 3].
 *
 * Rows: a codeword is one row of n_c values (one row of the soft passes' LLR buffers has
 * n_c = M_occ 2b, contiguous in both output layouts). T is the largest step count with
 * n_tx <= n_c; n_info = T - 6. Coded bit k is read at row position perm[k] (perm NULL: k); row
 * positions no coded bit refers to are ignored. mimo_fec_create returns MIMO_ERR_ARG for a bad
 * rate, T < 7, n_c > 32768 and a perm whose n_tx entries are not distinct values < n_c.
 *
 * Decoder: maximum likelihood over the terminated trellis with a full traceback from state 0,
 * no truncation window. LLRs are positive for bit 0, as everywhere here; a punctured bit has
 * LLR 0. The metric of a transition with outputs (a, b) is (a ? -L_A : L_A) + (b ? -L_B : L_B),
 * L the plain int8 value (-128 is allowed and means -128) widened to int32. Path metrics are
 * int32, 0 in state 0 and -2^30 in every other state at the start; the largest reachable
 * magnitude is 2 128 24576 (6.3 M), so nothing is normalised and nothing wraps. At each state
 * the larger metric survives; on equality the predecessor whose oldest bit u_(t-6) is 0.
 *
 * Outputs per row: the n_info decoded bits packed MSB first (bit k in byte k >> 3, mask
 * 0x80 >> (k & 7)) at d_bits + row bits_pitch, every other bit and byte up to the pitch 0, and
 * optionally the final path metric of state 0. A row of all-zero LLRs (what the soft passes
 * write for unsynced frames and unwritten symbols) decodes to all-zero bits and metric 0. */
enum { MIMO_FEC_R12 = 0, MIMO_FEC_R23 = 1, MIMO_FEC_R34 = 2 };
typedef struct mimo_fec_config {
  uint32_t rate;          /* MIMO_FEC_* */
  uint32_t n_c;           /* values per row */
  const uint16_t *perm;   /* host, n_tx entries, copied; or NULL (identity) */
} mimo_fec_config;
typedef struct mimo_fec mimo_fec;
/* create, destroy, geometry and encode run on the host and touch no GPU */
int mimo_fec_create(const mimo_fec_config *c, mimo_fec **out);
int mimo_fec_destroy(mimo_fec *f);
int mimo_fec_geometry(const mimo_fec *f, uint32_t *steps, uint32_t *n_info, uint32_t *n_tx);
/* setup / test time: info[n_info] (0/1 bytes) -> row[n_c] (0/1 bytes at row positions, i.e.
 * after perm; unreferenced positions 0) */
int mimo_fec_encode(const mimo_fec *f, const uint8_t *info, uint8_t *row);
typedef struct mimo_fec_decode_args {
  const void *d_llr;      /* [n_rows][n_c] int8, 16-byte aligned */
  void *d_bits;           /* [n_rows][bits_pitch] uint8, 16-byte aligned */
  void *d_metric;         /* [n_rows] int32, or NULL */
  uint32_t n_rows;
  uint32_t bits_pitch;    /* bytes per output row: a multiple of 4, >= ceil(n_info / 8) */
} mimo_fec_decode_args;
/* Asynchronous on hip_stream (NULL: the default stream), no host synchronisation; the caller
 * orders it after whatever wrote d_llr. The first decode of a handle creates the device copy of
 * the position table and the survivor-decision workspace, both sized by the launch grid (the
 * device's CU count) and never by n_rows; later calls allocate nothing and can be captured into
 * a graph. MIMO_ERR_ARG for a null f, a, d_llr or d_bits, a misaligned pointer, n_rows = 0 and a
 * bad bits_pitch; MIMO_ERR_HIP / MIMO_ERR_NOMEM as elsewhere. Single-caller-thread per handle,
 * and one decode of a handle in flight at a time (the workspace is the handle's). */
int mimo_fec_decode(mimo_fec *f, const mimo_fec_decode_args *a, void *hip_stream);

/* ---- soft-output (max-log-MAP) decoder for the same code: soft in, soft out ----
 * Same code, rates, rows, perm, geometry and mimo_fec handle as mimo_fec_decode. LLRs are
 * positive for bit 0, a punctured bit has LLR 0, and the int8 values are used plain (-128 is
 * -128).
 *
 * Branch metric: same as Viterbi. g_t(p->s) = (a ? -L_A : L_A) + (b ? -L_B : L_B) for the
 *   outputs (a, b) of the transition.
 * Forward: alpha_0 = 0 in state 0 and NEG elsewhere. alpha_(t+1)(s) = max over the two
 *   predecessors of alpha_t(p) + g_t(p->s).
 * Backward: beta_T = 0 in state 0 and NEG elsewhere. beta_t(p) = max over the two successors of
 *   g_t(p->s) + beta_(t+1)(s).
 * NEG = -2^29, not Viterbi's -2^30. For T < 12 a state can be unreachable from both ends, so
 *   alpha + g + beta goes down to about -2^30. With -2^30 as the start it would wrap int32. The
 *   model's minimum over T = 7..13 is -2^30 - 140 and fits.
 * No normalisation. Everything is int32 (the model computes in int64 and asserts the int32
 *   range). Max and plus without overflow are exact in any order. So any evaluation order on the
 *   GPU gives the same integers.
 * Per-bit APP. For x in {u_t, A_t, B_t}: M_t^x(v) = max over transitions with x = v of
 *   alpha_t(p) + g_t(p->s) + beta_(t+1)(s), and Lambda_t^x = M(0) - M(1). Where one hypothesis
 *   has no path through the terminated trellis (this occurs for a few coded bits only at T = 7,
 *   8), Lambda is about +-2^29 with the right sign. The integer arithmetic defines it.
 *
 * Outputs per row:
 *   d_out[row][pos], int8, for every row position that a kept coded bit refers to. With
 *     MIMO_FEC_SISO_APP the value is clamp(Lambda, -127, 127). With MIMO_FEC_SISO_EXT it is
 *     clamp(Lambda - L_in, -127, 127), with the subtraction done in int32 before the clamp.
 *     Positions no coded bit refers to are not written. d_out must not overlap d_llr;
 *     overlapping ranges return MIMO_ERR_ARG.
 *   d_bits (optional): info bit k = (Lambda_k^u < 0). Packing, pitch and zero padding are exactly
 *     those of mimo_fec_decode. A tie (Lambda = 0) gives bit 0. This is not Viterbi's tie rule, so
 *     the bits equal mimo_fec_decode's only in rows without a zero Lambda^u.
 *   d_info_llr (optional): [n_rows][info_pitch] int8, clamp(Lambda_k^u, +-127) for k < n_info.
 *     Bytes up to the pitch are 0. info_pitch is a multiple of 4 and >= n_info.
 *   d_metric (optional): alpha_T(0). This is bitwise the metric mimo_fec_decode writes for the
 *     same row.
 * All-zero row. It gives all-zero d_out values at the used positions, zero bits, zero info LLRs
 * and metric 0 (for T >= 12). At T < 12 the impossible-hypothesis positions saturate to +-127.
 *
 * At least one of d_out, d_bits and d_info_llr must be non-null. Error codes, alignment rules
 * and threading are those of mimo_fec_decode: d_llr, d_out, d_bits and d_info_llr 16-byte and
 * d_metric 4-byte aligned; MIMO_ERR_ARG for a null f, a or d_llr, all three outputs null, a
 * misaligned pointer, n_rows = 0, a bad mode, a bad bits_pitch (with d_bits) or info_pitch (with
 * d_info_llr) and overlapping d_out / d_llr. Asynchronous on hip_stream, single caller thread per
 * handle, one call of a handle in flight. The first call allocates; later calls allocate nothing
 * and can be captured into a graph. The workspace (alpha checkpoints every 64 steps, sized by the
 * launch grid and never by n_rows) is the soft-output pass's own, created by a handle's first
 * mimo_fec_siso call: a handle that never calls it pays nothing. */
enum { MIMO_FEC_SISO_APP = 0, MIMO_FEC_SISO_EXT = 1 };
typedef struct mimo_fec_siso_args {
  const void *d_llr;    /* [n_rows][n_c] int8 */
  void *d_out;          /* [n_rows][n_c] int8, or NULL */
  void *d_bits;         /* [n_rows][bits_pitch] uint8, or NULL */
  void *d_info_llr;     /* [n_rows][info_pitch] int8, or NULL */
  void *d_metric;       /* [n_rows] int32, or NULL */
  uint32_t n_rows, bits_pitch, info_pitch, mode;
} mimo_fec_siso_args;
int mimo_fec_siso(mimo_fec *f, const mimo_fec_siso_args *a, void *hip_stream);

/* ---- the encoder on the device, with the bit mapper: the transmit side of the same code ----
 * Same code, rates, rows, perm, geometry and mimo_fec handle as mimo_fec_decode. Integer
 * arithmetic: the output is defined to the bit.
 *
 * Per row, row[0..n_c) is mimo_fec_encode applied to the info bits k = 0..n_info-1, bit k read at
 * byte k >> 3 with mask 0x80 >> (k & 7) of d_info + row bits_pitch: the format mimo_fec_decode
 * and mimo_fec_siso write to d_bits. The rest of d_info up to bits_pitch, the low bits of the
 * last info byte included, is ignored whatever it holds.
 *   MIMO_FEC_ENC_BITS writes row: all n_c bytes, 0 at positions no coded bit refers to.
 *   MIMO_FEC_ENC_QAM writes idx[j] = sum over i < 2b of row[2b j + i] << (2b - 1 - i), the
 *     inverse of the order in which the soft passes write a carrier's 2b LLRs (values 0..b-1 are
 *     Re, MSB first, then Im; the index is (gray(mI) << b) | gray(mQ)). With n_c = M_occ 2b a
 *     QAM row is one [M_occ] row of d_tx_idx, and n_rows = F N pid rows are a whole
 *     [F][N][pid][M_occ] payload of mimo_synth_frames_payload.
 *
 * Alignment, pitch rules, error codes, asynchrony and threading are those of mimo_fec_decode:
 * MIMO_ERR_ARG for a null f, a, d_info or d_out, a pointer that is not 16-byte aligned,
 * n_rows = 0, a bad bits_pitch, a bad form, qam_bits outside 1..4 with QAM or non-zero with
 * BITS, n_c not a multiple of 2b, and overlapping d_info and d_out; all checked before anything
 * touches the GPU. The first call of a handle creates the encoder's own device table (the
 * inverse position map, n_c uint16); later calls allocate nothing and can be captured into a
 * graph. The encoder shares no workspace with the decoders, so an encode and a decode of one
 * handle may be in flight together. */
enum { MIMO_FEC_ENC_BITS = 0, MIMO_FEC_ENC_QAM = 1 };
typedef struct mimo_fec_encode_args {
  const void *d_info;   /* [n_rows][bits_pitch] uint8, info bits packed MSB first */
  void *d_out;          /* BITS: [n_rows][n_c] uint8, 0/1 at row positions
                           QAM:  [n_rows][n_c / (2 b)] uint8 QAM indices */
  uint32_t n_rows, bits_pitch;
  uint32_t form;        /* MIMO_FEC_ENC_* */
  uint32_t qam_bits;    /* b = 1..4 with QAM (n_c must be a multiple of 2 b); 0 with BITS */
} mimo_fec_encode_args;
int mimo_fec_encode_rows(mimo_fec *f, const mimo_fec_encode_args *a, void *hip_stream);

/* stage timing with HIP events on the handle's launch stream (for the roofline line).
 * stages: 0 S&C, 1 plateau, 2 search, 3 LS, 4 weights, 5 decode, 6 EVM reduce; an sc16 batch
 * that is widened internally (not read in place) adds its widening launch to stage 0 */
#define MIMO_NUM_STAGES 7
int mimo_rx_set_timing(mimo_rx *h, int enable);
/* sums of stage durations (ms) and launch counts since the last call; synchronises */
int mimo_rx_get_stage_times(mimo_rx *h, double *ms, uint32_t *launches);
/* S&C samples whose fp64 metric fell within the decision band and were recomputed with the
 * oracle's exact fp32 order, since the last call (diagnostic; synchronises) */
int mimo_rx_get_sc_exact_count(mimo_rx *h, uint64_t *out);
/* the replay-decode kernel family the last batch or execute launched (diagnostic, no sync):
 * STREAM = decode_stream_kernel (persistent, 2x2/4x4), SPLIT = spectra_kernel +
 * apply_split_kernel (8x8 at M >= 512), SYMBOL = the per-symbol kernels, NONE = no decode yet */
enum { MIMO_DECODE_NONE = 0, MIMO_DECODE_STREAM = 1, MIMO_DECODE_SPLIT = 2,
       MIMO_DECODE_SYMBOL = 3 };
int mimo_rx_get_decode_path(const mimo_rx *h, int32_t *path);
/* persistent grids (the streaming and split decodes) sized for n_cu CUs instead of the device's
 * count (diagnostic: a handle whose stream is CU-masked; 0 restores the device's count). Call
 * before the handle's first batch (captured graphs keep the grid they were captured with). */
int mimo_rx_set_grid_cus(mimo_rx *h, uint32_t n_cu);
/* roofline probe (diagnostic, no reference counterpart): the streaming decode's memory pattern
 * without its arithmetic -- per symbol N rows of M + 2 complex64 samples staged by LDS-DMA and
 * N x M uint8 reference indices, N x M complex64 + N x M uint8 written symbol-major, on the
 * decode's persistent grid -- over n_frames x spf symbols of the caller's captures ([n_caps][N]
 * [stride] complex64), reference rows and output buffers ([n_frames][spf][N][M]); reps timed
 * launches after one warm-up, the mean in *ms_per_launch. N x M in {4 x 2048, 4 x 1024,
 * 2 x 4096, 2 x 2048, 2 x 1024} (the streaming decode's geometries, every subcarrier occupied).
 * Returns 0, or 1 (arguments), 2 (HIP), 3 (geometry). */
int mimo_probe_decode_pattern(const void *d_iq, uint64_t stride, uint32_t n_caps, uint32_t N,
                              uint32_t M, uint32_t cp, uint32_t n_frames, uint32_t spf,
                              const void *d_ref, void *d_out_sym, void *d_out_idx, int reps,
                              void *hip_stream, float *ms_per_launch);
/* the CFO stages the last batch ran (diagnostic, no sync): 0 off, 1 estimate and derotation,
 * 2 the same plus the per-symbol common phase (the streaming decode's CPE variant) -- the
 * oracle's cfo_mode for the same batch */
int mimo_rx_get_cfo_mode(const mimo_rx *h, int32_t *mode);
/* streaming execute: the device capture's capacity and the samples it holds per antenna
 * (diagnostic). While seeking, only the samples a later trigger can still reach are kept
 * (the reference's bounded window ring, framing.cc:387-388), so the capture stays near the
 * window size however long an unsynchronised stream runs. */
int mimo_rx_get_stream_capacity(const mimo_rx *h, uint64_t *capacity, uint64_t *held);
/* DEBUG_LOG (mimo/config.h:84-86, off by default here): the streaming execute writes the
 * reference's debug traces into directory `dir` (NULL or "" turns them off):
 *   f_sc_<k>.dat     float32 Schmidl-Cox metric y of every sample processed while seeking,
 *                    antenna k from 1, appended per call (framing.cc:390-402, 598-600);
 *   corr_<k>_<ac>.dat  float32 search metric over window indices [0, ACB - M), ac from 1, and
 *                    corr_<k>_0.dat for S0 (framing.cc:675-696, 716-737, 873-883).
 * The files mimo/apps/plot.py reads. Opening happens here (the reference opens them in its
 * constructor); they are closed by the next call or mimo_rx_destroy. */
int mimo_rx_set_debug_log(mimo_rx *h, const char *dir);

/* ---------------- transmitter: framegen (framing.h:42-103) ---------------- */
typedef struct mimo_tx mimo_tx;
int mimo_tx_create(uint32_t M, uint32_t cp_len, uint32_t num_streams,
                   uint32_t num_access_codes, const uint8_t *p, const uint8_t *s0_bits,
                   const uint8_t *s1_bits, mimo_tx **out);
int mimo_tx_destroy(mimo_tx *h);
/* framegen::write_sync_words (framing.cc:169-208): host buffers, (nac*N+1)*SL each */
int mimo_tx_write_sync_words(mimo_tx *h, float *const *tx, uint32_t *n_written);
/* framegen::assemble_mimo_packet (framing.cc:210-235): in[t] M_occ symbols -> SL samples */
int mimo_tx_assemble_mimo_packet(mimo_tx *h, float *const *tx, const float *const *in,
                                 uint32_t *n_written);
int mimo_tx_get_codes(mimo_tx *h, float *s0 /* M */, float *s1 /* N*nac*M */);

/* ---------------- synthetic captures on the GPU (tx_worker layout + channel + AWGN) -----
 * [lead zeros SL*(N*nac+1)+u][sync words][pid data symbols][tail zeros], x0.25 baseband
 * gain (main.cc:1048-1053), flat Rayleigh H ~ CN(0,1) per frame, AWGN. */
typedef struct mimo_synth_config {
  uint32_t M, cp_len, num_streams, num_access_codes, pid, qam_order;
  uint64_t seed;
  float snr_db;
  uint32_t tail_syms;
  int32_t identity_channel;
  int32_t offset;         /* lead offset u; < 0: drawn per frame from the seed in [0, SL) */
  const uint8_t *p, *s0_bits, *s1_bits;
} mimo_synth_config;
/* length of frame `frame_id` (depends on its offset u) */
int mimo_synth_frame_len(const mimo_synth_config *c, uint64_t frame_id, uint64_t *len);
/* writes n_frames captures into d_out (layout of mimo_batch; samples past a frame's own
 * length are zero-padded noise), optional d_tx_idx [F][N][pid][M_occ] and d_H [F][N][N] */
int mimo_synth_frames(const mimo_synth_config *c, uint64_t frame_id0, uint32_t n_frames,
                      void *d_out, uint64_t stride, uint64_t frame_len, void *d_tx_idx,
                      void *d_H, void *hip_stream);
/* mimo_synth_frames in every respect (offset, sync words, channel, noise, frame grouping, error
 * codes) with the caller's data symbols: qam_point(d_tx_idx[...] & (L^2 - 1)) for the input
 * d_tx_idx [F][N][pid][M_occ] uint8, in place of the hash draw. Fed the d_tx_idx that
 * mimo_synth_frames wrote, it writes the same capture bit for bit. MIMO_ERR_ARG for a null
 * d_tx_idx unless pid = 0. */
int mimo_synth_frames_payload(const mimo_synth_config *c, uint64_t frame_id0, uint32_t n_frames,
                              void *d_out, uint64_t stride, uint64_t frame_len,
                              const void *d_tx_idx, void *d_H, void *hip_stream);

/* ---------------- helpers (setup-time, host) ---------------- */
int mimo_sctype_default(uint8_t *p, uint32_t M);   /* ofdmframe_init_default_sctype */
int mimo_sctype_liquid(uint8_t *p, uint32_t M);    /* compiled-out guard/pilot variant */
int mimo_sctype_validate(const uint8_t *p, uint32_t M, uint32_t *M_null, uint32_t *M_pilot,
                         uint32_t *M_data);        /* ofdmframe_validate_sctype */
int mimo_msequence_draw_bits(uint32_t m, uint32_t g, uint32_t a, uint32_t count,
                             uint8_t *out);        /* liquid msequence draws */
/* 2x2 invert (framing.cc:1344-1367) on host arrays: returns gain */
float mimo_invert2(float *W /* 4 complex */, const float *G /* 4 complex */);

/* device memory / stream helpers so callers need no HIP headers */
int mimo_dev_alloc(void **ptr, size_t bytes);
int mimo_dev_free(void *ptr);
int mimo_memcpy_h2d(void *dst, const void *src, size_t bytes, void *hip_stream);
int mimo_memcpy_d2h(void *dst, const void *src, size_t bytes, void *hip_stream);
int mimo_memcpy_d2d(void *dst, const void *src, size_t bytes, void *hip_stream);
int mimo_memset_d(void *dst, int value, size_t bytes, void *hip_stream);
/* Capture ingest at the wire format (UHD sc16, mimo/config.h:52) instead of the host fc32
 * the reference's rx worker receives (mimo/main.cc:837-848). d_sc16 holds n_arrays rows of n
 * interleaved int16 I/Q samples, src_stride samples apart; row r is widened to complex64
 * float(i16)*scale at d_fc32 + r*dst_stride (complex units), i.e. straight into the planar
 * layout of mimo_batch. Rows must not overlap. Asynchronous on hip_stream. */
int mimo_ingest_sc16(const void *d_sc16, uint64_t src_stride, void *d_fc32, uint64_t dst_stride,
                     uint32_t n_arrays, uint64_t n, float scale, void *hip_stream);
/* ---------------- pinned-host capture ring ----------------
 * Replaces the rx worker's malloc'd fc32 rx_buffer and its /tmp round trip
 * (mimo/main.cc:842-848, 872-898, 906-918): the recv loop writes UHD sc16 wire samples
 * (CPU format "sc16", mimo/config.h:52) straight into pinned host chunks, and every commit is
 * uploaded asynchronously (one 2-D copy on the ring's own HIP stream) into a device capture
 * [n_ant][stride] of sc16 samples -- the layout mimo_batch takes with sample_format =
 * MIMO_SAMPLE_SC16. A chunk is reused only after its upload has completed, so n_chunks >= 2
 * overlaps the next recv with the previous upload. One producer thread calls acquire/commit;
 * the consumer calls bind/publish (both may run concurrently with the producer). */
typedef struct mimo_ring mimo_ring;
int mimo_ring_create(uint32_t n_ant, uint32_t chunk_samples, uint32_t n_chunks, mimo_ring **out);
int mimo_ring_destroy(mimo_ring *r);   /* waits for the uploads in flight */
/* target of the following commits: d_capture rows of `capacity` samples, `stride` apart
 * (samples; capacity <= stride); write position 0. The uploads are not ordered against
 * readers of d_capture: rebinding a capture that a published batch may still be reading needs
 * the caller to synchronise first, or mimo_ring_bind_after. */
int mimo_ring_bind(mimo_ring *r, void *d_capture, uint64_t stride, uint64_t capacity);
/* mimo_ring_bind, and the uploads into the new binding wait (on the device) for the work
 * enqueued on consumer_stream so far: a capture can be refilled while its batch runs */
int mimo_ring_bind_after(mimo_ring *r, void *d_capture, uint64_t stride, uint64_t capacity,
                         void *consumer_stream);
/* the next chunk: rows[a] = host pointer of antenna a's chunk_samples interleaved int16 I/Q
 * (UHD's per-channel buffer vector, main.cc:874); waits for that chunk's previous upload */
int mimo_ring_acquire(mimo_ring *r, void **rows, uint32_t *max_samples);
/* n <= max_samples samples were written to every row of the acquired chunk: upload them at
 * the write position (MIMO_ERR_ARG past capacity or with no bound capture) */
int mimo_ring_commit(mimo_ring *r, uint32_t n);
/* make hip_stream wait, on the device, for every upload committed so far; *n_written = the
 * bound capture's samples per antenna so far */
int mimo_ring_publish(mimo_ring *r, void *hip_stream, uint64_t *n_written);

/* Carrier-frequency offset (absent from the reference: FIXME at framing.cc:486). Over the S0
 * body starting at sample `start` of each antenna row (period M/2, framing.cc:1054-1111),
 * P = sum_{n<M/2} conj(x[start+n]) x[start+n+M/2]; eps = arg(P)/pi in subcarrier spacings.
 * eps[0..n_ant-1] per antenna, eps[n_ant] from the sum of the antennas' P. Synchronous. */
int mimo_cfo_estimate(const void *d_iq, uint64_t stride, uint32_t n_ant, uint64_t start,
                      uint32_t M, double *eps, void *hip_stream);
/* x[n] *= exp(-j 2 pi (eps/M) (n - n0)) for n < n on every row, in place. Asynchronous. */
int mimo_cfo_derotate(void *d_iq, uint64_t stride, uint32_t n_ant, uint64_t n, int64_t n0,
                      double eps, uint32_t M, void *hip_stream);
int mimo_stream_sync(void *hip_stream);
int mimo_device_count(int *n);
const char *mimo_last_error(void);
const char *mimo_version(void);

#ifdef __cplusplus
}
#endif
#endif
