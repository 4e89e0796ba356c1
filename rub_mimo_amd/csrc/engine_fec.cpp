// rub_mimo_amd/csrc/engine_fec.cpp -- the channel code over the int8 LLR rows: the mimo_fec
// handle (geometry, position table, host encoder), mimo_fec_decode, the launch of the
// wave-per-row Viterbi decoder (fec_kernels.hip), and mimo_fec_siso, the launch of the
// max-log-MAP decoder on the same grid (fec_siso_kernels.hip), and mimo_fec_encode_rows, the
// launch of the encoder and bit mapper (fec_enc_kernels.hip). Independent of mimo_rx: opt-in
// passes over a buffer of LLRs that the batch launches nothing for. create, geometry, encode and
// destroy touch no GPU.
#include <new>

#include "engine_internal.hpp"

struct mimo_fec {
  uint32_t rate = 0, n_c = 0, T = 0, n_info = 0, n_tx = 0, chunks = 0;
  // row position of A_t | of B_t << 16 per step (kFecPunctured: not sent), perm and puncturing
  // resolved; chunks * kFecChunk entries, the steps past T punctured
  std::vector<uint32_t> pos;
  // ---- created by the first decode or soft-output call, sized by the grid ----
  uint32_t grid_blocks = 0;        // the persistent grid; set once d_pos is uploaded
  DevBuf<uint32_t> d_pos;
  // ---- created by the first decode ----
  uint32_t max_blocks = 0;
  DevBuf<unsigned long long> ws;   // [max_blocks * waves per block][chunks * kFecChunk]
  // ---- created by the first soft-output call ----
  uint32_t siso_blocks = 0;
  // [siso_blocks * waves per block][(chunks + kFecChunk) * kFecChunk]
  DevBuf<int32_t> ws_siso;
  // ---- created by the first mimo_fec_encode_rows (the encoder's own: no decoder state) ----
  uint32_t enc_blocks = 0;         // the most workgroups a launch uses
  std::vector<uint16_t> inv;       // [n_c] the inverse position map (FecEncArgs::inv)
  DevBuf<uint16_t> d_inv;
};

namespace {

constexpr uint32_t kFecTail = 6;
constexpr uint32_t kFecMaxNc = 32768;
// resident waves per CU the persistent grid is sized for (DESIGN.md "Viterbi decoder");
// RMIMO_FEC_WAVES overrides it (diagnostic, 4..32, read at a handle's first decode)
constexpr uint32_t kFecWavesPerCu = 16;

// kept (1) / punctured (0) per step of the period
struct Pattern { uint32_t period; uint8_t a[3], b[3]; };
const Pattern kPatterns[3] = {{1, {1, 0, 0}, {1, 0, 0}}, {2, {1, 1, 0}, {1, 0, 0}},
                              {3, {1, 1, 0}, {1, 0, 1}}};

uint32_t fec_n_tx(const Pattern &p, uint32_t T) {
  uint32_t per = 0, n = 0;
  for (uint32_t i = 0; i < p.period; i++) per += p.a[i] + p.b[i];
  for (uint32_t i = 0; i < T % p.period; i++) n += p.a[i] + p.b[i];
  return T / p.period * per + n;
}

// the persistent grid and the device copy of the position table, shared by both decoders
int fec_grid(mimo_fec *f, hipStream_t s) {
  if (f->grid_blocks) return MIMO_OK;
  int dev = 0, ncu = 0;
  HIPCHK(hipGetDevice(&dev));
  HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  if (ncu <= 0) return fail(MIMO_ERR_HIP, "no CU count");
  uint32_t wpc = kFecWavesPerCu;
  if (const char *e = getenv("RMIMO_FEC_WAVES")) {
    const long v = strtol(e, nullptr, 10);
    if (v >= 4 && v <= 32) wpc = (uint32_t)v;
  }
  const uint32_t wpb = kFecBlock / 64;
  const uint32_t blocks = (uint32_t)ncu * wpc / wpb;
  if (f->d_pos.ensure(f->pos.size()) != hipSuccess) {
    (void)hipGetLastError();
    return fail(MIMO_ERR_NOMEM, "channel code position table");
  }
  HIPCHK(hipMemcpyAsync(f->d_pos.p, f->pos.data(), sizeof(uint32_t) * f->pos.size(),
                        hipMemcpyHostToDevice, s));
  f->grid_blocks = blocks;
  return MIMO_OK;
}

int fec_first_decode(mimo_fec *f, hipStream_t s) {
  const int rc = fec_grid(f, s);
  if (rc) return rc;
  const size_t words = (size_t)f->grid_blocks * (kFecBlock / 64) * f->chunks * kFecChunk;
  if (f->ws.ensure(words) != hipSuccess) {
    (void)hipGetLastError();
    return fail(MIMO_ERR_NOMEM, "Viterbi decision workspace");
  }
  f->max_blocks = f->grid_blocks;
  return MIMO_OK;
}

int fec_first_siso(mimo_fec *f, hipStream_t s) {
  const int rc = fec_grid(f, s);
  if (rc) return rc;
  const size_t words = (size_t)f->grid_blocks * (kFecBlock / 64) * (f->chunks + kFecChunk) *
                       kFecChunk;
  if (f->ws_siso.ensure(words) != hipSuccess) {
    (void)hipGetLastError();
    return fail(MIMO_ERR_NOMEM, "soft-output decoder checkpoint workspace");
  }
  f->siso_blocks = f->grid_blocks;
  return MIMO_OK;
}

// workgroups per CU the encoder's grid is sized for: 6 KiB of LDS and 256 threads each
constexpr uint32_t kFecEncBlocksPerCu = 8;

// the encoder's grid and the inverse position map: row position -> where the kernel parks the
// parity that belongs there
int fec_first_encode(mimo_fec *f, hipStream_t s) {
  int dev = 0, ncu = 0;
  HIPCHK(hipGetDevice(&dev));
  HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  if (ncu <= 0) return fail(MIMO_ERR_HIP, "no CU count");
  const uint32_t nw = (f->T + 31) / 32;
  f->inv.assign(f->n_c, (uint16_t)(64 * nw));
  for (uint32_t t = 0; t < f->T; t++) {
    const uint32_t pa = f->pos[t] & 0xFFFFu, pb = f->pos[t] >> 16;
    if (pa != kFecPunctured) f->inv[pa] = (uint16_t)t;
    if (pb != kFecPunctured) f->inv[pb] = (uint16_t)(32 * nw + t);
  }
  if (f->d_inv.ensure(f->inv.size()) != hipSuccess) {
    (void)hipGetLastError();
    return fail(MIMO_ERR_NOMEM, "encoder position map");
  }
  HIPCHK(hipMemcpyAsync(f->d_inv.p, f->inv.data(), sizeof(uint16_t) * f->inv.size(),
                        hipMemcpyHostToDevice, s));
  f->enc_blocks = (uint32_t)ncu * kFecEncBlocksPerCu;
  return MIMO_OK;
}

}  // namespace

extern "C" {

int mimo_fec_create(const mimo_fec_config *c, mimo_fec **out) {
  if (!c || !out) return fail(MIMO_ERR_ARG, "null argument");
  if (c->rate > MIMO_FEC_R34) return fail(MIMO_ERR_ARG, "rate must be MIMO_FEC_R12, _R23 or _R34");
  if (c->n_c > kFecMaxNc) return fail(MIMO_ERR_ARG, "n_c > 32768");
  const Pattern &p = kPatterns[c->rate];
  uint32_t T = 0;
  while (fec_n_tx(p, T + 1) <= c->n_c) T++;          // n_tx grows with every step
  if (T < kFecTail + 1) return fail(MIMO_ERR_ARG, "row too short: fewer than 7 trellis steps");
  const uint32_t n_tx = fec_n_tx(p, T);
  if (c->perm) {
    std::vector<uint8_t> seen(c->n_c, 0);
    for (uint32_t k = 0; k < n_tx; k++) {
      if (c->perm[k] >= c->n_c) return fail(MIMO_ERR_ARG, "perm entry out of range");
      if (seen[c->perm[k]]++) return fail(MIMO_ERR_ARG, "perm entries are not distinct");
    }
  }
  mimo_fec *f = new (std::nothrow) mimo_fec();
  if (!f) return fail(MIMO_ERR_NOMEM, "mimo_fec");
  f->rate = c->rate; f->n_c = c->n_c; f->T = T; f->n_info = T - kFecTail; f->n_tx = n_tx;
  f->chunks = (T + kFecChunk - 1) / kFecChunk;
  f->pos.assign((size_t)f->chunks * kFecChunk, kFecPunctured | (kFecPunctured << 16));
  uint32_t k = 0;
  for (uint32_t t = 0; t < T; t++) {
    uint32_t pa = kFecPunctured, pb = kFecPunctured;
    if (p.a[t % p.period]) { pa = c->perm ? c->perm[k] : k; k++; }
    if (p.b[t % p.period]) { pb = c->perm ? c->perm[k] : k; k++; }
    f->pos[t] = pa | (pb << 16);
  }
  *out = f;
  return MIMO_OK;
}

int mimo_fec_destroy(mimo_fec *f) {
  delete f;
  return MIMO_OK;
}

int mimo_fec_geometry(const mimo_fec *f, uint32_t *steps, uint32_t *n_info, uint32_t *n_tx) {
  if (!f) return fail(MIMO_ERR_ARG, "null argument");
  if (steps) *steps = f->T;
  if (n_info) *n_info = f->n_info;
  if (n_tx) *n_tx = f->n_tx;
  return MIMO_OK;
}

int mimo_fec_encode(const mimo_fec *f, const uint8_t *info, uint8_t *row) {
  if (!f || !info || !row) return fail(MIMO_ERR_ARG, "null argument");
  memset(row, 0, f->n_c);
  auto u = [&](int64_t t) -> uint32_t {
    return t >= 0 && t < (int64_t)f->n_info ? (info[t] & 1u) : 0u;
  };
  for (int64_t t = 0; t < (int64_t)f->T; t++) {
    const uint32_t A = u(t) ^ u(t - 2) ^ u(t - 3) ^ u(t - 5) ^ u(t - 6);
    const uint32_t B = u(t) ^ u(t - 1) ^ u(t - 2) ^ u(t - 3) ^ u(t - 6);
    const uint32_t pa = f->pos[t] & 0xFFFFu, pb = f->pos[t] >> 16;
    if (pa != kFecPunctured) row[pa] = (uint8_t)A;
    if (pb != kFecPunctured) row[pb] = (uint8_t)B;
  }
  return MIMO_OK;
}

int mimo_fec_decode(mimo_fec *f, const mimo_fec_decode_args *a, void *hip_stream) {
  if (!f || !a || !a->d_llr || !a->d_bits) return fail(MIMO_ERR_ARG, "null argument");
  if (((uintptr_t)a->d_llr & 15u) || ((uintptr_t)a->d_bits & 15u))
    return fail(MIMO_ERR_ARG, "d_llr and d_bits must be 16-byte aligned");
  if ((uintptr_t)a->d_metric & 3u) return fail(MIMO_ERR_ARG, "d_metric must be 4-byte aligned");
  if (a->n_rows == 0) return fail(MIMO_ERR_ARG, "n_rows is 0");
  if ((a->bits_pitch & 3u) || a->bits_pitch < (f->n_info + 7) / 8)
    return fail(MIMO_ERR_ARG, "bits_pitch must be a multiple of 4 and >= ceil(n_info / 8)");
  hipStream_t s = (hipStream_t)hip_stream;
  if (f->max_blocks == 0) {
    const int rc = fec_first_decode(f, s);
    if (rc) return rc;
  }
  FecArgs k{};
  k.llr = reinterpret_cast<const int8_t *>(a->d_llr);
  k.bits = reinterpret_cast<uint8_t *>(a->d_bits);
  k.metric = reinterpret_cast<int32_t *>(a->d_metric);
  k.pos = f->d_pos.p;
  k.ws = f->ws.p;
  k.n_rows = a->n_rows; k.n_c = f->n_c; k.T = f->T; k.chunks = f->chunks;
  k.pitch_dw = a->bits_pitch / 4;
  const uint32_t wpb = kFecBlock / 64;
  launch_fec_viterbi(k, std::min(f->max_blocks, (a->n_rows + wpb - 1) / wpb), s);
  HIPCHK(hipGetLastError());
  return MIMO_OK;
}

int mimo_fec_encode_rows(mimo_fec *f, const mimo_fec_encode_args *a, void *hip_stream) {
  if (!f || !a || !a->d_info || !a->d_out) return fail(MIMO_ERR_ARG, "null argument");
  if (((uintptr_t)a->d_info & 15u) || ((uintptr_t)a->d_out & 15u))
    return fail(MIMO_ERR_ARG, "d_info and d_out must be 16-byte aligned");
  if (a->n_rows == 0) return fail(MIMO_ERR_ARG, "n_rows is 0");
  if ((a->bits_pitch & 3u) || a->bits_pitch < (f->n_info + 7) / 8)
    return fail(MIMO_ERR_ARG, "bits_pitch must be a multiple of 4 and >= ceil(n_info / 8)");
  uint32_t group = 1;
  if (a->form == MIMO_FEC_ENC_BITS) {
    if (a->qam_bits != 0) return fail(MIMO_ERR_ARG, "qam_bits must be 0 with MIMO_FEC_ENC_BITS");
  } else if (a->form == MIMO_FEC_ENC_QAM) {
    if (a->qam_bits < 1 || a->qam_bits > 4)
      return fail(MIMO_ERR_ARG, "qam_bits must be 1..4 with MIMO_FEC_ENC_QAM");
    group = 2 * a->qam_bits;
    if (f->n_c % group) return fail(MIMO_ERR_ARG, "n_c is not a multiple of 2 qam_bits");
  } else {
    return fail(MIMO_ERR_ARG, "form must be MIMO_FEC_ENC_BITS or MIMO_FEC_ENC_QAM");
  }
  const uint32_t n_out = f->n_c / group;
  {
    const uintptr_t i = (uintptr_t)a->d_info, o = (uintptr_t)a->d_out;
    const uintptr_t ib = (uintptr_t)a->n_rows * a->bits_pitch, ob = (uintptr_t)a->n_rows * n_out;
    if (i < o + ob && o < i + ib) return fail(MIMO_ERR_ARG, "d_out overlaps d_info");
  }
  hipStream_t s = (hipStream_t)hip_stream;
  if (f->enc_blocks == 0) {
    const int rc = fec_first_encode(f, s);
    if (rc) return rc;
  }
  FecEncArgs k{};
  k.info = reinterpret_cast<const uint8_t *>(a->d_info);
  k.out = reinterpret_cast<uint8_t *>(a->d_out);
  k.inv = f->d_inv.p;
  k.n_rows = a->n_rows; k.pitch = a->bits_pitch; k.n_info = f->n_info;
  k.nw = (f->T + 31) / 32; k.n_out = n_out;
  if (!launch_fec_encode(k, group, std::min(f->enc_blocks, a->n_rows), s))
    return fail(MIMO_ERR_UNSUPPORTED, "no encoder instance for this row");
  HIPCHK(hipGetLastError());
  return MIMO_OK;
}

int mimo_fec_siso(mimo_fec *f, const mimo_fec_siso_args *a, void *hip_stream) {
  if (!f || !a || !a->d_llr) return fail(MIMO_ERR_ARG, "null argument");
  if (!a->d_out && !a->d_bits && !a->d_info_llr)
    return fail(MIMO_ERR_ARG, "d_out, d_bits and d_info_llr are all null");
  if (((uintptr_t)a->d_llr & 15u) || ((uintptr_t)a->d_out & 15u) ||
      ((uintptr_t)a->d_bits & 15u) || ((uintptr_t)a->d_info_llr & 15u))
    return fail(MIMO_ERR_ARG, "d_llr, d_out, d_bits and d_info_llr must be 16-byte aligned");
  if ((uintptr_t)a->d_metric & 3u) return fail(MIMO_ERR_ARG, "d_metric must be 4-byte aligned");
  if (a->n_rows == 0) return fail(MIMO_ERR_ARG, "n_rows is 0");
  if (a->mode > MIMO_FEC_SISO_EXT)
    return fail(MIMO_ERR_ARG, "mode must be MIMO_FEC_SISO_APP or MIMO_FEC_SISO_EXT");
  if (a->d_bits && ((a->bits_pitch & 3u) || a->bits_pitch < (f->n_info + 7) / 8))
    return fail(MIMO_ERR_ARG, "bits_pitch must be a multiple of 4 and >= ceil(n_info / 8)");
  if (a->d_info_llr && ((a->info_pitch & 3u) || a->info_pitch < f->n_info))
    return fail(MIMO_ERR_ARG, "info_pitch must be a multiple of 4 and >= n_info");
  if (a->d_out) {
    const uintptr_t bytes = (uintptr_t)a->n_rows * f->n_c;
    const uintptr_t l = (uintptr_t)a->d_llr, o = (uintptr_t)a->d_out;
    if (l < o + bytes && o < l + bytes) return fail(MIMO_ERR_ARG, "d_out overlaps d_llr");
  }
  hipStream_t s = (hipStream_t)hip_stream;
  if (f->siso_blocks == 0) {
    const int rc = fec_first_siso(f, s);
    if (rc) return rc;
  }
  FecSisoArgs k{};
  k.llr = reinterpret_cast<const int8_t *>(a->d_llr);
  k.out = reinterpret_cast<int8_t *>(a->d_out);
  k.bits = reinterpret_cast<uint8_t *>(a->d_bits);
  k.info_llr = reinterpret_cast<int8_t *>(a->d_info_llr);
  k.metric = reinterpret_cast<int32_t *>(a->d_metric);
  k.pos = f->d_pos.p;
  k.ws = f->ws_siso.p;
  k.n_rows = a->n_rows; k.n_c = f->n_c; k.T = f->T; k.chunks = f->chunks;
  k.pitch_dw = a->d_bits ? a->bits_pitch / 4 : 0;
  k.info_pitch = a->d_info_llr ? a->info_pitch : 0;
  k.ext = a->mode == MIMO_FEC_SISO_EXT;
  const uint32_t wpb = kFecBlock / 64;
  launch_fec_siso(k, std::min(f->siso_blocks, (a->n_rows + wpb - 1) / wpb), s);
  HIPCHK(hipGetLastError());
  return MIMO_OK;
}

}  // extern "C"
