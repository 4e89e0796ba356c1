// rub_mimo_amd/csrc/engine_diag.cpp -- the engine's RMIMO_* environment switches and the
// diagnostic reports they turn on (device-to-host copies, a stream synchronisation and
// fprintf to stderr: none of it is on the hot path). The stage drivers call each in one line;
// tools/ scripts parse the printed text. (RMIMO_SEARCH_FORM, RMIMO_SEARCH_WAVE and the S&C
// kernels' own RMIMO_SC_DIAG are read in est_kernels.hip and sc_item_kernels.hip.)
#include "engine_internal.hpp"

namespace mimo {

const DiagEnv &diag_env() {
  static const DiagEnv env = [] {
    auto on = [](const char *name) { const char *e = getenv(name); return e && e[0] == '1'; };
    DiagEnv d{};
    const char *e = getenv("RMIMO_SC_DIAG");
    d.sc_diag = e ? atoi(e) : 0;
    d.sc_prof = on("RMIMO_SC_PROF");
    d.sc_one_phase = on("RMIMO_SC_PHASES");
    d.sc_count = on("RMIMO_SC_COUNT");
    d.sc_count_items = d.sc_count && getenv("RMIMO_SC_COUNT")[1] == '+';
    e = getenv("RMIMO_LS_FORM");
    d.ls_terms = e && strcmp(e, "terms") == 0;
    d.dec_prof = on("RMIMO_DEC_PROF");
    d.cfo_debug = on("RMIMO_CFO_DEBUG");
    d.no_graph = on("RMIMO_NO_GRAPH") || d.sc_prof || d.dec_prof;
    return d;
  }();
  return env;
}

int diag_sc_prof_arm(mimo_rx *h, bool screen, hipStream_t s, unsigned long long **prof) {
  if (!diag_env().sc_prof) return MIMO_OK;
  if (!h->sc_prof.p) HIPCHK(h->sc_prof.ensure(32));
  HIPCHK(hipMemsetAsync(h->sc_prof.p, 0, 32 * sizeof(unsigned long long), s));
  HIPCHK(hipMemsetAsync(h->sc_prof.p + 8, 0xFF, sizeof(unsigned long long), s));
  if (screen) HIPCHK(hipMemsetAsync(h->sc_prof.p, 0xFF, sizeof(unsigned long long), s));
  *prof = h->sc_prof.p;
  return MIMO_OK;
}

// S&C work-list size, and with RMIMO_SC_COUNT=1+ per item: frame, chunk, unproven range and
// its iterations
int diag_sc_count(mimo_rx *h, uint32_t F, uint64_t nchunks, bool screen, uint32_t hot_cap,
                  hipStream_t s) {
  if (!diag_env().sc_count) return MIMO_OK;
  hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(s, &cst);
  if (cst != hipStreamCaptureStatusNone) return MIMO_OK;
  uint32_t q[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(q, h->ws.queue.p, sizeof(q), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  fprintf(stderr, "sc_count hot_items %u (screen %d, frames %u, chunks %llu)\n", q[1],
          screen ? 1 : 0, F, (unsigned long long)nchunks);
  if (!diag_env().sc_count_items || !screen) return MIMO_OK;
  const uint32_t n = std::min(q[1], hot_cap);
  std::vector<ScHot> hv(n);
  std::vector<unsigned long long> mn((size_t)F * nchunks), mx((size_t)F * nchunks);
  HIPCHK(hipMemcpyAsync(hv.data(), h->ws.hot.p, sizeof(ScHot) * n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(mn.data(), h->ws.scr_min.p, sizeof(unsigned long long) * mn.size(),
                        hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(mx.data(), h->ws.scr_max.p, sizeof(unsigned long long) * mx.size(),
                        hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (uint32_t i = 0; i < n; i++) {
    const ScHot &it = hv[i];
    const size_t ci = (size_t)it.f * nchunks + it.chunk;
    const long long lo = (long long)mn[ci] - it.w0, hi = (long long)mx[ci] - it.w0;
    const long long a0 = std::max<long long>(0, (lo - (long long)h->cp - 2) / kScIterLen);
    const long long a1 = std::min<long long>(kScSpan / kScIterLen - 1, hi / kScIterLen);
    fprintf(stderr, "sc_item %u f %u chunk %llu w0 %lld c0 %lld unproven [%lld, %lld] (%lld) "
            "iterations %lld-%lld\n", i, it.f, (unsigned long long)it.chunk, (long long)it.w0,
            (long long)it.c0, lo, hi, hi - lo + 1, a0, a1);
  }
  return MIMO_OK;
}

// screened path: the exact kernel's timeline (wall clock, 100 MHz); else the per-item cycle
// split of the S&C item kernel
int diag_sc_prof_report(mimo_rx *h, bool screen, hipStream_t s) {
  if (!diag_env().sc_prof) return MIMO_OK;
  if (screen) {
    unsigned long long v[32];
    HIPCHK(hipMemcpyAsync(v, h->sc_prof.p, sizeof(v), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    fprintf(stderr, "exact_prof passes %llu last_pass_end %.2f us finalize_end %.2f us "
            "avg_pass %.2f us avg_resolve %.2f us finalizes %llu cond %.2f us record %.2f us "
            "(%llu with candidates) slowest pass %.2f us (%llu iterations, resolve %.2f us) "
            "max windows/pass %llu (samples %llu) total samples %llu\n", v[4],
            (double)(v[1] - v[0]) / 100.0, (double)(v[2] - v[0]) / 100.0,
            v[4] ? (double)v[3] / v[4] / 100.0 : 0.0, v[4] ? (double)v[7] / v[4] / 100.0 : 0.0,
            v[6], v[6] ? (double)v[10] / v[6] / 100.0 : 0.0,
            v[12] ? (double)v[11] / v[12] / 100.0 : 0.0, v[12], (double)(v[13] >> 32) / 100.0,
            (v[13] >> 24) & 0xFF, (double)(v[13] & 0xFFFFFF) / 100.0, v[14] >> 32,
            v[14] & 0xFFFFFFFFull, v[15]);
    const double np = v[4] ? (double)v[4] : 1.0;
    fprintf(stderr, "exact_split record %.2f us setup %.2f us iterations %.2f us (%.2f per pass) "
            "start offset avg %.2f max %.2f us | per iteration: ring %.2f scan %.2f walk %.2f us "
            "(first iteration's ring %.2f us per pass; guarded fills %llu)\n",
            v[20] / np / 100.0, v[21] / np / 100.0,
            v[22] / np / 100.0, v[23] / np, (v[26] / np - (double)v[0]) / 100.0,
            (double)(v[25] - v[0]) / 100.0, v[23] ? v[16] / (double)v[23] / 100.0 : 0.0,
            v[23] ? v[17] / (double)v[23] / 100.0 : 0.0, v[23] ? v[18] / (double)v[23] / 100.0 : 0.0,
            v[19] / np / 100.0, v[24]);
    fprintf(stderr, "exact_windows max per iteration %llu, iterations with >= 2 windows %llu "
            "(their passes' max duration %.2f us)\n", v[27], v[28], (double)v[29] / 100.0);
  } else {
    unsigned long long v[20];
    HIPCHK(hipMemcpyAsync(v, h->sc_prof.p, sizeof(v), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const double it = v[0] ? (double)v[0] : 1.0;
    fprintf(stderr, "sc_prof items %llu skipped %llu antenna_passes %llu cycles/item rows %.0f "
            "words %.0f resolve %.0f total %.0f wall_us/item %.2f span_us %.2f max_item_us %.2f "
            "last_start_us %.2f\n", v[0], v[6], v[1],
            v[2] / it, v[3] / it, v[4] / it, v[5] / it, v[7] / it / 100.0,
            (double)(v[9] - v[8]) / 100.0, v[10] / 100.0, (double)(v[11] - v[8]) / 100.0);
    fprintf(stderr, "sc_prof phases/item warm %.0f A %.0f scan %.0f B %.0f run %.0f | resolve "
            "passes %llu chain cycles/pass %.0f samples/pass %.1f\n",
            v[12] / it, v[13] / it, v[14] / it, v[15] / it, v[16] / it, v[17],
            v[17] ? (double)v[18] / v[17] : 0.0, v[17] ? (double)v[19] / v[17] : 0.0);
  }
  return MIMO_OK;
}

int diag_dec_prof_arm(mimo_rx *h, hipStream_t s, unsigned long long **prof) {
  if (!diag_env().dec_prof) return MIMO_OK;
  if (!h->sc_prof.p) HIPCHK(h->sc_prof.ensure(28));
  HIPCHK(hipMemsetAsync(h->sc_prof.p, 0, 8 * sizeof(unsigned long long), s));
  *prof = h->sc_prof.p;
  return MIMO_OK;
}

// per-item cycle split of the decode kernel
int diag_dec_prof_report(mimo_rx *h, hipStream_t s) {
  if (!diag_env().dec_prof) return MIMO_OK;
  unsigned long long v[8];
  HIPCHK(hipMemcpyAsync(v, h->sc_prof.p, sizeof(v), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const double it = v[0] ? (double)v[0] : 1.0;
  fprintf(stderr, "dec_prof items %llu cycles/item load %.0f fft %.0f apply %.0f reduce %.0f "
          "| stream split: pass0 %.0f fetch %.0f subfft %.0f\n",
          v[0], v[1] / it, v[2] / it, v[3] / it, v[4] / it, v[5] / it, v[6] / it, v[7] / it);
  return MIMO_OK;
}

// the per-frame CFO state the decode read
int diag_cfo_frames(mimo_rx *h, uint32_t F, hipStream_t s) {
  if (!diag_env().cfo_debug || !h->cfo) return MIMO_OK;
  std::vector<FrameInfo> fi(F);
  HIPCHK(hipMemcpyAsync(fi.data(), h->ws.info.p, sizeof(FrameInfo) * F, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (uint32_t f = 0; f < F; f++)
    fprintf(stderr, "cfo_dbg f %u status %d base %lld i0 %u eps %.9f E %lld\n", f, (int)fi[f].status,
            (long long)fi[f].base, fi[f].i0, (double)fi[f].cfo_eps, (long long)fi[f].cfo_E);
  return MIMO_OK;
}

}  // namespace mimo
