// rub_mimo_amd/csrc/engine_internal.hpp -- what the engine's translation units share: the
// mimo_rx / mimo_tx handles, the small host utilities, and the entry points of each file.
//   engine.cpp         handles' life cycle, setters, plain getters, device/memcpy helpers
//   engine_stages.cpp  workspace growth and the stage drivers (sync, estimate, decode)
//   engine_batch.cpp   mimo_rx_process_batch, the HIP-graph cache, batch getters, soft output
//   engine_sic.cpp     mimo_rx_sic_detect, mimo_rx_sic_soft(_fb) and the getters: the SIC passes
//   engine_pic.cpp     mimo_rx_pic_soft: the soft-input MMSE-PIC pass
//   engine_lord.cpp    mimo_rx_lord_soft: the layered tree-search pass
//   engine_fec.cpp     mimo_fec_*: the channel code's handle, host encoder, Viterbi and
//                      soft-output decoder launches
//   engine_stream.cpp  mimo_rx_execute: the streaming framesync state machine, DEBUG_LOG
//   engine_tx.cpp      transmitter, synthesiser, subcarrier-type and m-sequence helpers
//   engine_diag.cpp    the RMIMO_* environment switches and the diagnostic reports
// Not part of the library's interface (include/mimo_rx.h is).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mimo_rx.h"
#include "kernels.hpp"

using namespace mimo;   // (engine files only)

#pragma GCC visibility push(hidden)   // internal to the library: not in its symbol table
namespace mimo {

// this thread's mimo_last_error() slot (host_fail, engine.cpp)
inline int fail(int code, const std::string &msg) { return host_fail(code, msg.c_str()); }

#define HIPCHK(x)                                                                       \
  do {                                                                                  \
    hipError_t e_ = (x);                                                                \
    if (e_ != hipSuccess)                                                               \
      return fail(MIMO_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));        \
  } while (0)

template <class T>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  hipError_t ensure(size_t cnt) {
    if (cnt <= n && p) return hipSuccess;
    release();
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), sizeof(T) * std::max<size_t>(cnt, 1));
    if (e == hipSuccess) n = cnt;
    return e;
  }
  // grow and keep: own the fresh block np (cnt elements); the caller has copied what survives
  void adopt(T *np, size_t cnt) {
    release();
    p = np;
    n = cnt;
  }
};

inline int ilog2(uint32_t v) {
  int l = 0;
  while ((1u << l) < v) l++;
  return ((1u << l) == v) ? l : -1;
}

struct StageTimer {
  bool on = false;
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> ev;
  hipEvent_t begin(hipStream_t s) {
    if (!on) return nullptr;
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    (void)hipEventRecord(e, s);
    return e;
  }
  void end(int stage, hipEvent_t b, hipStream_t s) {
    if (!on || !b) return;
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, s);
    ev.push_back({stage, {b, e}});
  }
};

// code tables common to the receiver and the transmitter
struct Codes {
  DevBuf<float2> code_time;   // [n_slots][M]
  DevBuf<float2> codespec;    // [n_slots][F]
  DevBuf<float2> codespec_w;  // [n_slots][F], the wave-local search's bin order
};

// The samples a stage reads: F captures of N antenna rows, `stride` complex samples apart,
// frame_len of them valid; fc32, or sc16 wire samples (float(i16) * scale) read in place.
struct Capture {
  const float2 *iq;
  uint64_t stride, frame_len;
  int sc16;
  float scale;
};

// the capture fields of a kernel-argument struct (ScArgs, ScreenArgs, PlateauArgs, SearchArgs,
// LsArgs, DecodeArgs)
template <class Args>
void set_capture(Args &a, const Capture &c) {
  a.iq = c.iq; a.stride = c.stride; a.frame_len = c.frame_len;
  a.sc16 = c.sc16; a.iq_scale = c.scale;
}

// The batch workspace. Rule: what run_batch can launch with lives in ws -- every device buffer
// that a launch issued from run_batch or from the streaming execute's stages may reallocate
// between calls. A captured batch graph holds these pointers in its kernel arguments, so they
// move through grow() only (rec also in ensure_workspace, which bumps gen itself), and the
// graph cache keys on gen (engine_batch.cpp). Sizes are computed next to the launches.
struct Workspace {
  uint64_t gen = 0;   // bumped exactly when a buffer below is (re)allocated
  template <class T>
  hipError_t grow(DevBuf<T> &b, size_t cnt) {
    if (cnt <= b.n && b.p) return hipSuccess;
    gen++;
    return b.ensure(cnt);
  }
  // rec is [rec_frames][rec_stride] S&C chunk records; the per-frame arrays hold rec_frames too
  uint32_t rec_frames = 0;
  uint64_t rec_stride = 0;
  DevBuf<unsigned long long> trig, keys;
  DevBuf<ScRecord> rec;
  DevBuf<FrameInfo> info;
  DevBuf<float2> G, W;
  DevBuf<float> gain;
  DevBuf<double> nvp, evm_part, evm_out, evm_chunk, lspart;
  DevBuf<uint32_t> evm_cnt;             // per-frame chunk counters of evm_kernel (self-resetting)
  DevBuf<uint32_t> nrec;                // per-frame EVM records of the streaming decode
  DevBuf<float2> lsq;                   // fused search + LS: X/S1 per access code
  DevBuf<unsigned long long> n_exact;   // S&C exact fp32 recomputes (diagnostic)
  DevBuf<uint32_t> queue;               // S&C work-queue head, hot-item count
  DevBuf<ScHot> hot;                    // S&C items awaiting exact resolution
  DevBuf<uint32_t> scr_flag;            // S&C screen: chunk listed [F][nchunks]
  DevBuf<unsigned long long> scr_min, scr_max;   // first / last unproven position per chunk
  DevBuf<unsigned long long> cand;      // streams: first S&C candidate per chunk [cap][chunks]
  DevBuf<unsigned long long> certfail;  // streams: re-arm certificate failures [cap] (bit = slot)
  DevBuf<float2> spec;                  // 8x8 split decode: spectra scratch
  DevBuf<float2> wide;                  // sc16 batches the fused kernels do not take: widened
  DevBuf<float2> cfo_iq;                // derotated scratch capture
  DevBuf<double> cfo_eps;
};

}  // namespace mimo
#pragma GCC visibility pop

// ======================================================================================
struct mimo_rx {
  // ---- configuration (framesync ctor arguments + config.h constants) ----
  uint32_t M = 0, cp = 0, SL = 0, N = 0, nac = 0, pid = 0;
  uint32_t M_null = 0, M_pilot = 0, M_data = 0, M_occ = 0;
  int log2M = 0, log2F = 0;
  uint32_t F = 0, lagc = 0, n_lagc = 0, n_slots = 0;
  bool search_ls = false;               // fused search + LS (search_ls_kernel) for this geometry
  bool cfo = false;                     // opt-in CFO estimate + derotation (batched path)
  uint32_t n_cu = 256;
  int det = 0;
  float noise_var = -1.0f;
  int keep_bias = 1;
  uint32_t siso_tx = 0, siso_rx = 0;
  double thr = 0.95;
  Qam qam{};
  uint64_t acb = 0, txl = 0, win_len = 0;
  float dn = 1.0f, ls_scale = 1.0f;
  double nv_norm = 0.0;
  std::vector<uint8_t> p;
  std::vector<int32_t> occ_index;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // ---- device tables: written by mimo_rx_create, immutable for the handle's life ----
  float2 *tw = nullptr;
  Codes codes;
  DevBuf<float> vscale;
  DevBuf<int8_t> s1sign, s1sign_w;   // signs [N][nac][M]; ls_window_kernel's order
  DevBuf<int32_t> occ;
  // ---- batch workspace: what run_batch can launch with lives in ws ----
  Workspace ws;
  // ---- last-batch facts and the post-pass buffers (in no captured graph) ----
  uint32_t last_frames = 0, last_max_out = 0;
  int last_decode_path = MIMO_DECODE_NONE;   // kernel family of the last decode launch
  int last_cfo_mode = 0;                     // CFO stages of the last batch (get_cfo_mode)
  uint32_t last_layout = 0;                  // out_layout of the last batch
  DevBuf<float> nu;                          // soft output: post-detection MSE [F][N][M_occ]
  // SIC detection (engine_sic.cpp): tables T [F][N][N][M_occ], C [F][N(N-1)/2][M_occ], the
  // detection order [F][M_occ][N], the post-SIC MSE [F][N][M_occ] and the solved-carrier flags
  // [F][M_occ] of the last batch
  DevBuf<float2> sic_T, sic_C;
  DevBuf<uint8_t> sic_order, sic_ok;
  DevBuf<float> sic_nu;
  // soft-input MMSE-PIC (engine_pic.cpp): the packed Q = G^H G [F][N^2][M_occ] and the carrier
  // flags [F][M_occ] of the last batch
  DevBuf<float> pic_Q;
  DevBuf<uint8_t> pic_ok;
  // layered tree search (engine_lord.cpp): Q as above, the N factors U [F][N][N^2 + N][M_occ],
  // the N permutations [F][N][M_occ] and the carrier flags [F][M_occ] of the last batch
  DevBuf<float> lord_Q, lord_U;
  DevBuf<uint32_t> lord_perm;
  DevBuf<uint8_t> lord_ok;
  // ---- streaming state (facade) and debug buffers (in no captured graph) ----
  // The device capture holds samples [origin, origin + total) of the stream since
  // construction/reset (positions inside it are capture-relative).
  DevBuf<float2> capbuf;
  uint64_t cap_len = 0, total = 0, origin = 0;
  uint64_t trim_clo = ~0ull;   // stream position of the S&C chunk of the last trim probe
  DevBuf<uint32_t> probe;               // trim probe: per antenna, a proven metric zero
  int state = MIMO_STATE_SEEK_PLATEAU;
  uint64_t nsp = 0;
  bool have_sync = false, have_est = false;
  FrameInfo sinfo{};
  DevBuf<float2> symbuf;
  std::vector<float2> symhost;
  mimo_rx_symbol_cb cb = nullptr;
  void *user = nullptr;
  // DEBUG_LOG files of the streaming execute (framing.cc:390-402, 598-600, 675-696, 873-883)
  std::string dbg_dir;
  std::vector<FILE *> dbg_fsc;
  DevBuf<float> dbg_y, dbg_corr;
  DevBuf<unsigned long long> sc_prof;   // RMIMO_SC_PROF=1 cycle counters
  StageTimer timer;
  // ---- graph cache ----
  // captured batch pipelines (see mimo_rx_process_batch): a few recent batch keys, so that
  // callers alternating between capture buffers (double-buffered ingest) replay graphs too
  struct GraphEntry {
    mimo_batch key{};
    hipStream_t stream = nullptr;
    uint64_t gen = 0;             // ws.gen the entry was recorded or captured at
    hipGraphExec_t exec = nullptr;
    uint64_t used = 0;            // 0: empty slot
  };
  std::array<GraphEntry, 4> graphs{};
  uint64_t graph_tick = 0;
};

struct mimo_tx {
  uint32_t M = 0, cp = 0, SL = 0, N = 0, nac = 0, M_occ = 0;
  int log2M = 0;
  float dn = 1.0f;
  hipStream_t stream = nullptr;
  Codes codes;
  std::vector<float2> s0, s1;  // host copies of the time-domain codes
  DevBuf<int32_t> occ_list;
  DevBuf<float2> din, dout;
  float2 *tw = nullptr;
};

#pragma GCC visibility push(hidden)
namespace mimo {

// ---- engine.cpp ----
int get_twiddles(float2 **out);   // tw[k] = exp(-2 pi i k / kTwN), shared by all handles
Qam make_qam(uint32_t order);
int validate_sctype(const uint8_t *p, uint32_t M, uint32_t *n0, uint32_t *n1, uint32_t *n2);
int build_codes(Codes &c, uint32_t M, uint32_t N, uint32_t nac, const uint8_t *p,
                const uint8_t *s0_bits, const uint8_t *s1_bits, int log2F, bool spectra,
                hipStream_t s);
int copy_W(mimo_rx *h, uint32_t f, float *W);                            // frame f's W, [M][N][N]
int copy_corr(mimo_rx *h, uint32_t F, uint32_t *corr, uint32_t *s0);     // search argmax indices

// ---- engine_stages.cpp ----
int ensure_workspace(mimo_rx *h, uint32_t F, uint64_t chunks);   // F slots, F x chunks records
double sc_band(uint32_t M);
// run_sync's optional inputs (the plain case: SyncRequest{} with fpc = 1)
struct SyncRequest {
  uint64_t chunk_lo;            // first S&C chunk to (re)compute; earlier ones are final
  bool reset_trig;              // captures start at their framesync's origin: clear the triggers
  uint32_t fpc;                 // frames per capture (> 1: the stream walk, F * fpc frame slots)
  const uint64_t *ref_starts;   // fpc > 1: transmitted frame starts [capture][ref_stride], or null
  uint32_t ref_stride;          // 0: fpc
  bool zero_keys;               // also zero the search's argmax keys (one fill launch)
};
// S&C + plateau over chunks [chunk_lo, end) of every capture
int run_sync(mimo_rx *h, const Capture &c, uint32_t F, const SyncRequest &q, hipStream_t s);
// search, LS and weights of F frame slots; cfo: the opt-in CFO's stage-1 arguments (stage 2 is
// launched here) or null; corr_trace: DEBUG_LOG lag metrics or null
int run_estimate(mimo_rx *h, const Capture &c, uint32_t F, bool keys_zeroed, CfoBatchArgs *cfo,
                 float *corr_trace, hipStream_t s);
// what a decode writes and compares against
struct DecodeRequest {
  uint32_t max_out;
  float2 *out_sym;
  uint8_t *out_idx;
  uint32_t layout;              // MIMO_LAYOUT_*
  int ref_mode;
  const uint8_t *ref_idx;
  uint64_t ref_seed, frame_id0;
  uint32_t n_caps;              // captures the F frame slots point into (0: F)
  const double *cfo_fold_part;  // folded CFO: the stage partials the kernel derotates by, or null
};
int run_decode(mimo_rx *h, const Capture &c, uint32_t F, const DecodeRequest &q, hipStream_t s);

// ---- engine_batch.cpp ----
// A captured batch graph bakes every host scalar of the launch arguments (siso indices,
// detector, noise variance, threshold) into its kernel nodes: any setter of such a scalar
// drops the graphs so the next batch is launched (and later re-captured) with the new value.
void invalidate_graph(mimo_rx *h);

// ---- engine_sic.cpp ----
// MIMO_OK when the handle's detector delivers y = (Q + lambda I)^-1 G^H X
int sic_supported(const mimo_rx *h);
// what the passes over the last batch's symbols ask of the handle and of the arguments they share
int sic_pass_check(const mimo_rx *h, const void *d_sym, const void *d_out_sym, uint32_t n_frames,
                   uint32_t max_out_syms, uint32_t out_layout);

// ---- engine_diag.cpp ----
struct DiagEnv {          // the engine's RMIMO_* switches, read once per process
  int sc_diag;            // RMIMO_SC_DIAG: ScArgs::diag bits
  bool sc_prof;           // RMIMO_SC_PROF=1: S&C cycle counters (PROFILE=1 build)
  bool sc_one_phase;      // RMIMO_SC_PHASES=1: screened S&C in one pass
  bool sc_count;          // RMIMO_SC_COUNT=1: print the S&C work-list size
  bool sc_count_items;    // RMIMO_SC_COUNT=1+: and every item
  bool ls_terms;          // RMIMO_LS_FORM=terms: fused LS terms + ls_combine_q_kernel
  bool dec_prof;          // RMIMO_DEC_PROF=1: decode cycle counters (PROFILE=1 build)
  bool cfo_debug;         // RMIMO_CFO_DEBUG=1: print the per-frame CFO state
  bool no_graph;          // RMIMO_NO_GRAPH=1, or a profile above: no HIP-graph replay
};
const DiagEnv &diag_env();
// Each returns MIMO_OK at once unless its switch is on. The reports synchronise the stream.
int diag_sc_prof_arm(mimo_rx *h, bool screen, hipStream_t s, unsigned long long **prof);
int diag_sc_count(mimo_rx *h, uint32_t F, uint64_t nchunks, bool screen, uint32_t hot_cap,
                  hipStream_t s);   // (not while the stream is capturing)
int diag_sc_prof_report(mimo_rx *h, bool screen, hipStream_t s);
int diag_dec_prof_arm(mimo_rx *h, hipStream_t s, unsigned long long **prof);
int diag_dec_prof_report(mimo_rx *h, hipStream_t s);
int diag_cfo_frames(mimo_rx *h, uint32_t F, hipStream_t s);

}  // namespace mimo
#pragma GCC visibility pop
