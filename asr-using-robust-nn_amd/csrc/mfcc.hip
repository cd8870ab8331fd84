// K1: batched waveform -> MFCC on the device (gfx950): the plan, the path selector and the C entry points.
//
// Stages (extract_features, extract_features_construct_dataset.py:24-39) and the kernels of the default path:
//   1. resample_persist_h2_kernel (resample.hip)  resampy 'kaiser_best' to 22 050 Hz on the fp16 matrix instruction
//   2. stft_bdft_kernel (stft_bdft.hip)           reflect-padded Hann frames -> block-DFT on the matrix pipe -> power -> mel -> dB
//   3. dct_kernel (stft_mel.hip)                  top_db floor, DCT-II 128 -> 20, layout, optional StandardScaler affine
// Every other variant (fp32 / VALU resamplers, Stockham and short-window STFTs, the fused resample -> STFT kernel of
// mfcc_fused.hip) is chosen in ONE place, pick_mfcc_path below; plan_run, plan_resample, plan_from_22k, their per-clip-length forms
// and plan_vjp (the one backward chain behind lipasr_mfcc_plan_vjp, _vjp_short and _vjp_ragged) ask it once and hand the kinds to
// the launchers of mfcc_plan.h.  This file holds no stage kernel except add_noise_kernel.
#include "mfcc_plan.h"
#include <memory>

namespace lipasr {

using namespace tables;

long g_k1_launches[K1_KERNELS] = {};
long g_k1_vjp_launches[K1V_KERNELS] = {};

void mfcc_plan_free(MfccPlan* p) {
  if (!p) return;
  void* ptrs[] = {p->d_hbandh, p->d_groups, p->d_dft, p->d_mel_wlo, p->d_mel_whi, p->d_mel_pstart, p->d_mel_plen, p->d_hband, p->d_lo, p->d_h, p->d_noff, p->d_hann, p->d_tw, p->d_mel_start, p->d_mel_len, p->d_mel_off,
                  p->d_mel_w, p->d_dct, p->d_y, p->d_db, p->d_fmax, p->d_gmel, p->d_part, p->d_gy, p->d_dct_rows, p->d_bin_run, p->d_rt_taps, p->d_rt_t0,
                  p->d_dft_t, p->d_melt_off, p->d_melt_len, p->d_melt_m, p->d_melt_w};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  for (hipEvent_t e : p->prof_events) (void)hipEventDestroy(e);
  bdft_tables_free(&p->bd);
  delete p;
}

// ---------------------------------------------------------------------------------------------
// A12 audio-domain noise (attacks.py:73-86, 145-183, 222-245), one workgroup per clip (normal4: common.h)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_noise_kernel(float* __restrict__ y, int n, int mode, float p0, float p1,
                                                         uint64_t seed) {
  __shared__ double red[4];
  const int u = blockIdx.x, tid = threadIdx.x;
  float* yu = y + (size_t)u * n;
  float sigma = p0;
  if (mode == 2) {
    double s = 0.0;
    for (int i = tid; i < n; i += 256) s += (double)yu[i] * (double)yu[i];
    s = wave_sum_d(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    const double watts = ((red[0] + red[1]) + (red[2] + red[3])) / (double)n;
    // noise_avg_watts = 10^((10 log10(P) - snr)/10) = P * 10^(-snr/10)
    sigma = (float)sqrt(watts * pow(10.0, -(double)p0 / 10.0));
  }
  for (int i4 = tid; i4 * 4 < n; i4 += 256) {
    float z[4];
    normal4(seed, (uint64_t)i4, (uint32_t)u, 0u, z);
    float s[4] = {sigma, sigma, sigma, sigma};
    if (mode == 1) {
      float q[4];
      normal4(seed, (uint64_t)i4, (uint32_t)u, 1u, q);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = (fabsf(q[e]) < p0) ? 10.0f * p1 : p1;  // sigma1 = 10 alpha on impulses
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = i4 * 4 + e;
      if (i < n) yu[i] += s[e] * z[e];
    }
  }
}

static int lo_max(const Polyphase& pp) {
  int m = 0;
  for (int r = 0; 32 * r < pp.up; ++r) m = std::max(m, pp.n_off[32 * r]);
  return m;
}
template <typename T>
static int upload(T** dptr, const std::vector<T>& v) {
  LP_HIP(hipMalloc(dptr, v.size() * sizeof(T)));
  LP_HIP(hipMemcpy(*dptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return LIPASR_OK;
}

// ---------------------------------------------------------------------------------------------
// The path selector.  The predicates below are its vocabulary; nothing else decides which kernel runs.
// ---------------------------------------------------------------------------------------------
// the persistent MFMA resamplers: float4-readable rows, one wavefront per phase tile that also fills the window
static bool resample_persist_ok(const MfccPlan* p, const void* wav, int fmt) {
  const int n_waves = p->n_ptiles;
  return p->d_hband && !(p->stage_mask & SM_VALU_RESAMPLER) && rows_vec4(p, wav, fmt) && (p->down & 3) == 0 && n_waves >= 8 &&
         n_waves <= kRpMaxWaves && 32 * ((kRsStride - 1) / 4) <= 5 * 64 * n_waves;
}
// the fp16-plane persistent resampler is the one that takes int16 PCM and per-clip lengths
static bool resample_h2_ok(const MfccPlan* p, const void* wav, int fmt) {
  return !p->identity && p->d_hbandh && !(p->stage_mask & SM_NO_H2) && resample_persist_ok(p, wav, fmt) && p->left == 64 &&
         p->down + 128 + 32 <= kRhRowHalfs;
}
// the 2048/512 kernels that know per-clip lengths (stft_bdft_kernel, stft_mel2_kernel); the profiling switches belong to stft_mel_kernel
static bool stft2_ok(const MfccPlan* p) { return !p->dft && !(p->stage_mask & (SM_ROUND2_STFT | SM_SKIP_FFT | SM_SKIP_MEL)); }
// the plan runs the fused kernel for plain float32 batches too (plan_vjp: the forward then left no resampled signal behind)
static bool prefers_fused(const MfccPlan* p) { return p->fused && p->prefer_fused; }

MfccPath pick_mfcc_path(const MfccPlan* p, const void* wav, int fmt, bool ragged) {
  MfccPath path;
  path.stft = p->dft ? MfccPath::ST_DFT
              : !stft2_ok(p) ? MfccPath::ST_STOCKHAM2
              : (p->bd.cfrag && !(p->stage_mask & SM_STOCKHAM)) ? MfccPath::ST_BDFT : MfccPath::ST_STOCKHAM4;
  if (!wav) return path;  // already at 22 050 Hz
  // three kernels (resample -> y in HBM -> STFT+mel -> DCT) unless the plan prefers the single fused resample+STFT kernel, which
  // moves 2.6x fewer bytes and is slower; the fused kernel also takes over when the three-kernel form cannot read
  // this input (unaligned int16 / ragged rows)
  const bool h2 = resample_h2_ok(p, wav, fmt);
  const bool three_ok = (fmt == 0 && !ragged) || (h2 && stft2_ok(p));
  path.fused = p->fused && !(p->stage_mask & SM_NO_FUSED) && (prefers_fused(p) || !three_ok);
  if (!three_ok) {
    if (!path.fused) {
      set_error("lipasr_mfcc: int16 input and per-clip lengths need the 2048/512 path with a 441/320- or 441/160-style resampler "
                "(16 kHz or 8 kHz input, rows a multiple of 4 samples); this plan is %d Hz, n_fft %d, rows of %d", p->sr_in, p->n_fft, p->n_samp);
      path.rc = LIPASR_EUNSUPPORTED;
    }
    return path;
  }
  const bool mfma = p->d_hband && !(p->stage_mask & SM_VALU_RESAMPLER);
  path.resampler = h2 ? MfccPath::RS_H2
                   : p->identity ? MfccPath::RS_COPY
                   : resample_persist_ok(p, wav, fmt) ? MfccPath::RS_PERSIST_F32
                   : mfma ? MfccPath::RS_MFMA
                   : (p->taps == 128 && p->up <= 448) ? MfccPath::RS_REG128 : MfccPath::RS_GENERIC;
  return path;
}
}  // namespace lipasr

using namespace lipasr;

// opaque plan type of the C ABI
struct lipasr_mfcc : lipasr::MfccPlan {};

namespace lipasr {

static void plan_unregister(MfccPlan* p) {
  if (!p || !p->ctx) return;
  std::vector<MfccPlan*>& v = p->ctx->mfcc_plans;
  for (size_t i = 0; i < v.size(); ++i)
    if (v[i] == p) { v.erase(v.begin() + i); break; }
  if (p->ctx->mfcc == p) p->ctx->mfcc = nullptr;
}

static int plan_build(lipasr_handle_t h, int sr_in, int n_samp, int batch_max, int n_fft, int hop, MfccPlan** out) {
  LP_CHECK_ARG(h != nullptr && out != nullptr, "lipasr_mfcc_plan: null argument");
  const bool dft = !(n_fft == kNFft && hop == kHop);
  if (dft && !(n_fft >= 32 && n_fft <= 32 * kDftMaxTiles * 2 - 2 && hop >= 1 && hop <= n_fft)) {
    set_error("lipasr_mfcc_plan_ex: n_fft=%d hop=%d; supported: 2048/512 (FFT path) or 32 <= n_fft <= %d with "
              "1 <= hop <= n_fft (DFT-contraction path)", n_fft, hop, 32 * kDftMaxTiles * 2 - 2);
    return LIPASR_EUNSUPPORTED;
  }
  LP_CHECK_ARG(sr_in >= 1000 && sr_in <= 384000, "lipasr_mfcc_plan: sr_in=%d outside [1000, 384000]", sr_in);
  LP_CHECK_ARG(n_samp >= 2 && batch_max >= 1, "lipasr_mfcc_plan: n_samp=%d batch_max=%d", n_samp, batch_max);
  DeviceGuard g(h->device);
  std::unique_ptr<MfccPlan, void (*)(MfccPlan*)> guard(new lipasr_mfcc(), mfcc_plan_free);  // every early return frees the plan
  MfccPlan* p = guard.get();
  p->ctx = h;
  p->sr_in = sr_in; p->n_samp = n_samp; p->batch_max = batch_max;
  p->identity = (sr_in == kSr);
  resampled_lengths(n_samp, sr_in, kSr, &p->n_valid, &p->n_y);
  if (p->n_y < 2) { set_error("lipasr_mfcc_plan: clip too short after resampling"); return LIPASR_EINVAL; }
  p->n_fft = n_fft; p->hop = hop; p->dft = dft;
  p->rs_target_wgs = h->rs_target_wgs;
  p->n_frames = 1 + p->n_y / hop;
  // the FFT path reflects repeatedly like np.pad (any clip of >= 2 samples); the short-window path's pad kernel
  // reflects once, which needs the clip to be longer than the padding
  if (dft && p->n_y <= n_fft / 2) { set_error("lipasr_mfcc_plan_ex: clip shorter than the reflect padding"); return LIPASR_EINVAL; }
  int rc = LIPASR_OK;
  if (!p->identity) {
    Polyphase pp = build_polyphase(sr_in, kSr);
    if (pp.up > 4096 || pp.taps > 2048) {
      set_error("lipasr_mfcc_plan: ratio %d/%d needs %d phases x %d taps; unsupported", pp.up, pp.down, pp.up, pp.taps);
      return LIPASR_EUNSUPPORTED;
    }
    p->up = pp.up; p->down = pp.down; p->taps = pp.taps; p->left = pp.left;
    if ((rc = upload(&p->d_h, pp.h)) != LIPASR_OK || (rc = upload(&p->d_noff, pp.n_off)) != LIPASR_OK) return rc;
    {
      std::vector<float> hb;
      std::vector<int> lo;
      if (build_band_tables(pp, &hb, &lo)) {
        p->n_ptiles = (int)lo.size();
        if ((rc = upload(&p->d_hband, hb)) != LIPASR_OK || (rc = upload(&p->d_lo, lo)) != LIPASR_OK) return rc;
        // fp16-plane fragments for resample_persist_h2_kernel: the band of every tile must fit 160 samples from its
        // 8-aligned start and stay inside the 480-sample window
        bool fits = true;
        for (int r = 0; r < (int)lo.size(); ++r) {
          const int first = lo[r] + 1, band0 = first & ~7;
          fits = fits && (first - band0 + kRsBand <= kRhK) && (band0 + kRhK <= kRhRowHalfs);
        }
        if (fits && (rc = upload(&p->d_hbandh, build_band_h2(hb, lo))) != LIPASR_OK) return rc;
      }
    }
    // the fused resample -> STFT kernel: 2048/512 frames, 441 phases (16 kHz and 8 kHz input), rows 2 banks apart
    if (!dft && p->d_hband && pp.up == kFuUp && pp.left == 64 && (pp.down % 32) == 0 && pp.down >= 160 && pp.down <= 320 &&
        (kFuQ - 1) * pp.down + lo_max(pp) + 1 + kRsBand <= kFuQ * pp.down + 160) {
      std::vector<int> groups = build_groups(p->n_y, p->n_frames, pp.up);
      if (!groups.empty()) {
        p->n_groups = (int)groups.size() / 4;
        if ((rc = upload(&p->d_groups, groups)) != LIPASR_OK) return rc;
        p->fused = true;
      }
    }
  }
  MelSparse ms = mel_sparse(n_fft);
  if (dft) {
    p->dft_tiles = (1 + n_fft / 2 + 31) / 32;
    p->dft_krows = ((n_fft / 2 + 1 + 2 * kDftGroup - 1) / (2 * kDftGroup)) * (2 * kDftGroup);  // folded: rows 0..N/2
    p->dft_rpc = (p->n_y + 2 * (n_fft / 2) + hop - 1) / hop;
    if ((rc = upload(&p->d_dft, dft_table(n_fft, p->dft_krows, p->dft_tiles))) != LIPASR_OK) return rc;
  }
  MelPairs mp = dft ? MelPairs() : mel_pairs();
  if (dft) { mp.wlo.assign(1, 0.f); mp.whi.assign(1, 0.f); mp.start.assign(1, 0); mp.len.assign(1, 0); }
  if (!mp.ok) {
    set_error("lipasr_mfcc_plan: mel filter bank is not a two-filters-per-bin bank");
    return LIPASR_EUNSUPPORTED;
  }
  if ((rc = upload(&p->d_mel_wlo, mp.wlo)) != LIPASR_OK || (rc = upload(&p->d_mel_whi, mp.whi)) != LIPASR_OK ||
      (rc = upload(&p->d_mel_pstart, mp.start)) != LIPASR_OK || (rc = upload(&p->d_mel_plen, mp.len)) != LIPASR_OK ||
      (rc = upload(&p->d_hann, hann_periodic())) != LIPASR_OK || (rc = upload(&p->d_tw, twiddles())) != LIPASR_OK ||
      (rc = upload(&p->d_mel_start, ms.start)) != LIPASR_OK || (rc = upload(&p->d_mel_len, ms.len)) != LIPASR_OK ||
      (rc = upload(&p->d_mel_off, ms.off)) != LIPASR_OK || (rc = upload(&p->d_mel_w, ms.w)) != LIPASR_OK ||
      (rc = upload(&p->d_dct, dct_fragments())) != LIPASR_OK)
    return rc;
  if (!dft && (rc = bdft_tables_build(&p->bd)) != LIPASR_OK) return rc;
  const size_t ny = (size_t)batch_max * p->n_y, ndb = (size_t)batch_max * p->n_frames * 128,
               nfm = (size_t)batch_max * p->n_frames;
  if (hipMalloc(&p->d_y, ny * sizeof(float)) != hipSuccess || hipMalloc(&p->d_db, ndb * sizeof(float)) != hipSuccess ||
      hipMalloc(&p->d_fmax, nfm * sizeof(float)) != hipSuccess) {
    set_error("lipasr_mfcc_plan: intermediate allocation failed");
    return LIPASR_ENOMEM;
  }
  h->mfcc_plans.push_back(p);
  *out = guard.release();
  return LIPASR_OK;
}

static int plan_check(const char* fn, const MfccPlan* p, int batch, int L) {
  LP_CHECK_ARG(p != nullptr, "%s: null plan", fn);
  LP_CHECK_ARG(batch >= 1 && batch <= p->batch_max, "%s: batch %d outside [1, %d]", fn, batch, p->batch_max);
  LP_CHECK_ARG(L >= 1, "%s: utterance_length=%d", fn, L);
  return LIPASR_OK;
}

// the five events of one timed extraction (MfccPlan::prof_events)
enum ProfEvent { EV_RESAMPLE_BEGIN, EV_RESAMPLE_END, EV_STFT_BEGIN, EV_STFT_END, EV_DCT_END, kProfEvents };
// the slot of the extraction being timed, or null when profiling is off or full
static hipEvent_t* prof_slot(MfccPlan* p) { return p->prof_n < p->prof_cap ? &p->prof_events[kProfEvents * (size_t)p->prof_n] : nullptr; }

static int plan_resample(MfccPlan* p, const float* wav, int batch, float* y, hipStream_t st) {
  const MfccPath path = pick_mfcc_path(p, wav, 0, false);
  hipEvent_t* ev = prof_slot(p);
  if (ev) LP_HIP(hipEventRecord(ev[EV_RESAMPLE_BEGIN], st));
  int rc = launch_resample(p, path.resampler, wav, 0, nullptr, batch, y, st);
  if (rc != LIPASR_OK) return rc;
  if (ev) {
    LP_HIP(hipEventRecord(ev[EV_RESAMPLE_END], st));
    p->prof_half = true;
  }
  return LIPASR_OK;
}

static int plan_from_22k(MfccPlan* p, const float* y, int batch, int n_y, int L, const double* am, const double* as, float* out,
                         hipStream_t st) {
  LP_CHECK_ARG(n_y == p->n_y, "lipasr_mfcc_from_22k: n_y=%d but the plan was made for %d", n_y, p->n_y);
  LP_CHECK_ARG((am == nullptr) == (as == nullptr), "lipasr_mfcc_from_22k: give both affine arrays or neither");
  const MfccPath path = pick_mfcc_path(p, nullptr, 0, false);
  // timed only as the second half of a split extraction (a resample timing is already in the slot)
  hipEvent_t* ev = p->prof_half ? prof_slot(p) : nullptr;
  if (ev) LP_HIP(hipEventRecord(ev[EV_STFT_BEGIN], st));
  int rc = launch_from_22k(p, path.stft, y, nullptr, batch, L, am, as, out, st, ev ? ev[EV_STFT_END] : nullptr);
  if (rc != LIPASR_OK) return rc;
  if (ev) {
    LP_HIP(hipEventRecord(ev[EV_DCT_END], st));
    p->prof_half = false;
    p->prof_n++;
  }
  return LIPASR_OK;
}

// the whole extraction.  fmt 0: float32 samples, 1: int16 PCM.  n_valid: per-clip sample counts (device) or null.
static int plan_run(MfccPlan* p, const void* wav, int fmt, const int* n_valid, int batch, int L, const double* am, const double* as,
                    float* out, hipStream_t st) {
  LP_CHECK_ARG(wav && out, "lipasr_mfcc: null argument");
  LP_CHECK_ARG(fmt == 0 || fmt == 1, "lipasr_mfcc: sample format %d (0 = float32, 1 = int16 PCM)", fmt);
  LP_CHECK_ARG((am == nullptr) == (as == nullptr), "lipasr_mfcc: give both affine arrays or neither");
  const MfccPath path = pick_mfcc_path(p, wav, fmt, n_valid != nullptr);
  if (path.rc != LIPASR_OK) return path.rc;
  hipEvent_t* ev = p->prof_half ? nullptr : prof_slot(p);
  int rc;
  if (ev) LP_HIP(hipEventRecord(ev[EV_RESAMPLE_BEGIN], st));
  if (path.fused) {
    if (ev) {  // no separate resampling kernel: its slot stays empty, the fused kernel is timed as stft_mel
      LP_HIP(hipEventRecord(ev[EV_RESAMPLE_END], st));
      LP_HIP(hipEventRecord(ev[EV_STFT_BEGIN], st));
    }
    if ((rc = launch_fused(p, wav, fmt, n_valid, batch, st)) != LIPASR_OK) return rc;
    if (ev) LP_HIP(hipEventRecord(ev[EV_STFT_END], st));
    if ((rc = launch_dct(p, batch, L, am, as, out, n_valid, st)) != LIPASR_OK) return rc;
  } else {
    if ((rc = launch_resample(p, path.resampler, wav, fmt, n_valid, batch, p->d_y, st)) != LIPASR_OK) return rc;
    if (ev) {
      LP_HIP(hipEventRecord(ev[EV_RESAMPLE_END], st));
      LP_HIP(hipEventRecord(ev[EV_STFT_BEGIN], st));
    }
    if ((rc = launch_from_22k(p, path.stft, p->d_y, n_valid, batch, L, am, as, out, st, ev ? ev[EV_STFT_END] : nullptr)) != LIPASR_OK) return rc;
  }
  if (ev) {
    LP_HIP(hipEventRecord(ev[EV_DCT_END], st));
    p->prof_n++;
  }
  return LIPASR_OK;
}

// ---- backward pass ----
// what both kinds of plan keep for the backward pass: the plain DCT rows, Gmel, g_y and the partial images of the middle stage
// (n_part floats: [batch_max][vj_groups][kVjSeg] for the 2048/512 kernels, [workgroups][seg] for the short-window one)
static int vjp_workspaces(const char* fn, MfccPlan* p, size_t n_part) {
  int rc;
  if (!p->d_dct_rows && (rc = upload(&p->d_dct_rows, dct_matrix())) != LIPASR_OK) return rc;
  const size_t ngm = (size_t)p->batch_max * p->n_frames * kNMels, ngy = (size_t)p->batch_max * p->n_y;
  if ((!p->d_gmel && hipMalloc(&p->d_gmel, ngm * sizeof(float)) != hipSuccess) ||
      (!p->d_part && hipMalloc(&p->d_part, n_part * sizeof(float)) != hipSuccess) ||
      (!p->d_gy && hipMalloc(&p->d_gy, ngy * sizeof(float)) != hipSuccess)) {
    (void)hipGetLastError();
    set_error("%s: intermediate allocation failed", fn);
    return LIPASR_ENOMEM;
  }
  return LIPASR_OK;
}

// 2048/512 plans, first call: the mel filter of every bin's run, and the workspaces
static int vjp_prepare(const char* fn, MfccPlan* p) {
  if (p->vj_ready) return LIPASR_OK;
  DeviceGuard g(p->ctx->device);
  p->vj_groups = (p->n_frames + kVjFrames - 1) / kVjFrames;
  MelPairs mp = mel_pairs();
  std::vector<int> run(kNBins, 0);
  for (int m = 0; m < kNMels; ++m)
    for (int i = 0; i < mp.len[m]; ++i) run[mp.start[m] + i] = m;
  int rc;
  if (!p->d_bin_run && (rc = upload(&p->d_bin_run, run)) != LIPASR_OK) return rc;
  if ((rc = vjp_workspaces(fn, p, (size_t)p->batch_max * p->vj_groups * kVjSeg)) != LIPASR_OK) return rc;
  p->vj_ready = true;
  return LIPASR_OK;
}

// Tables of R^T in polyphase form: for phase r = j mod down, the run of outputs t (relative to up q') with
// r + left - taps <= pos(t) <= r + left - 1, pos(t) = down floor(t / up) + n_off[t mod up] = floor(t down / up), and their taps.
static int resample_vjp_prepare(MfccPlan* p) {
  if (p->identity || p->d_rt_taps) return LIPASR_OK;
  DeviceGuard g(p->ctx->device);
  const Polyphase pp = build_polyphase(p->sr_in, kSr);
  const long up = pp.up, down = pp.down;
  auto split = [&](long t, long* q, int* ph) {
    long qq = t / up;
    if (t - qq * up < 0) --qq;
    *q = qq; *ph = (int)(t - qq * up);
  };
  auto pos = [&](long t) { long q; int ph; split(t, &q, &ph); return down * q + pp.n_off[ph]; };
  std::vector<int> t0(pp.down), cnt(pp.down);
  int nt = 0;
  for (int r = 0; r < pp.down; ++r) {
    const long A = (long)r + pp.left - pp.taps, B = (long)r + pp.left - 1;
    long num = A * up, t = num / down;
    if (num - t * down < 0) --t;  // floor
    t -= 2;
    while (pos(t) < A) ++t;
    t0[r] = (int)t;
    int c = 0;
    while (pos(t + c) <= B) ++c;
    cnt[r] = c;
    nt = std::max(nt, c);
  }
  std::vector<float> ht((size_t)nt * pp.down, 0.0f);
  for (int r = 0; r < pp.down; ++r)
    for (int i = 0; i < cnt[r]; ++i) {
      long q; int ph;
      split((long)t0[r] + i, &q, &ph);
      const long k = (long)r - (down * q + pp.n_off[ph]) + pp.left - 1;
      if (k >= 0 && k < pp.taps) ht[(size_t)i * pp.down + r] = pp.h[(size_t)ph * pp.taps + k];
    }
  p->rt_nt = nt;
  p->rt_t0min = *std::min_element(t0.begin(), t0.end());
  p->rt_t0max = *std::max_element(t0.begin(), t0.end());
  int rc;
  if ((rc = upload(&p->d_rt_t0, t0)) != LIPASR_OK || (rc = upload(&p->d_rt_taps, ht)) != LIPASR_OK) return rc;
  return LIPASR_OK;
}

static int plan_resample_vjp(MfccPlan* p, const float* gy, int batch, float* gx, hipStream_t st, const int* nv = nullptr) {
  int rc = resample_vjp_prepare(p);
  if (rc != LIPASR_OK) return rc;
  ResampleVjpArgs a;
  a.n_y = p->n_y; a.n_valid = p->n_valid; a.n_samp = p->n_samp; a.up = p->up; a.down = p->down; a.identity = p->identity;
  a.ht = p->d_rt_taps; a.t0 = p->d_rt_t0; a.nt = p->rt_nt; a.t0min = p->rt_t0min; a.t0max = p->rt_t0max;
  a.nv = nv; a.sr_in = p->sr_in;
  return launch_resample_vjp(a, gy, gx, batch, st);
}

// short-window plans (dft_mel_kernel's forward), first call: the folded table with bins and samples exchanged (unit-stride
// B-operand loads of the second contraction), the CSR mel bank by bin, and the workspaces
static int vjp_short_prepare(const char* fn, MfccPlan* p) {
  if (p->vj_ready) return LIPASR_OK;
  DeviceGuard g(p->ctx->device);
  int n_wgs, seg, rc;
  if ((rc = short_vjp_geometry(p->n_fft, p->hop, p->dft_rpc, p->dft_tiles, p->batch_max, &n_wgs, &seg)) != LIPASR_OK) return rc;
  const int nb = p->dft_tiles * 32, ld = p->dft_tiles * 64;
  const std::vector<float> T = dft_table(p->n_fft, p->dft_krows, p->dft_tiles);
  std::vector<float> TT((size_t)nb * ld, 0.0f);
  for (int b = 0; b < nb; ++b)
    for (int n = 0; n < std::min(nb, p->dft_krows); ++n) {
      const size_t src = (size_t)n * ld + (b >> 5) * 64 + (b & 31), dst = (size_t)b * ld + (n >> 5) * 64 + (n & 31);
      TT[dst] = T[src];
      TT[dst + 32] = T[src + 32];
    }
  const MelSparse ms = mel_sparse(p->n_fft);
  std::vector<int> off(nb, 0), len(nb, 0), mm;
  std::vector<float> ww;
  for (int b = 0; b < nb; ++b) {
    off[b] = (int)mm.size();
    for (int m = 0; m < kNMels; ++m) {
      const int j = b - ms.start[m];
      if (j >= 0 && j < ms.len[m] && ms.w[ms.off[m] + j] != 0.0f) { mm.push_back(m); ww.push_back(ms.w[ms.off[m] + j]); }
    }
    len[b] = (int)mm.size() - off[b];
  }
  if (mm.empty()) { mm.push_back(0); ww.push_back(0.0f); }
  if ((rc = upload(&p->d_melt_off, off)) != LIPASR_OK || (rc = upload(&p->d_melt_len, len)) != LIPASR_OK ||
      (rc = upload(&p->d_melt_m, mm)) != LIPASR_OK || (rc = upload(&p->d_melt_w, ww)) != LIPASR_OK ||
      (rc = vjp_workspaces(fn, p, (size_t)n_wgs * seg)) != LIPASR_OK || (rc = upload(&p->d_dft_t, TT)) != LIPASR_OK)
    return rc;
  p->vj_ready = true;
  return LIPASR_OK;
}

// ---- clips of different lengths in one launch: n_valid[] (device) holds each row's samples at the plan's input rate ----
// the plans whose three-kernel forward takes per-clip lengths (pick_mfcc_path): 2048/512 at 16 kHz or 8 kHz, rows of 4 k samples
static int ragged_unsupported(const char* fn, const MfccPlan* p) {
  if (!(resample_h2_ok(p, nullptr, 0) && stft2_ok(p))) {
    set_error("%s: per-clip lengths need a 2048/512 plan at 16 kHz or 8 kHz with rows a multiple of 4 samples; this plan is %d Hz, "
              "n_fft %d, rows of %d", fn, p->sr_in, p->n_fft, p->n_samp);
    return LIPASR_EUNSUPPORTED;
  }
  return LIPASR_OK;
}

static int plan_resample_ragged(MfccPlan* p, const void* wav, int fmt, const int* nv, int batch, float* y, hipStream_t st) {
  LP_CHECK_ARG(wav && nv && y, "lipasr_mfcc_plan_resample_ragged: null argument");
  LP_CHECK_ARG(fmt == 0 || fmt == 1, "lipasr_mfcc_plan_resample_ragged: sample format %d (0 = float32, 1 = int16 PCM)", fmt);
  const MfccPath path = pick_mfcc_path(p, wav, fmt, true);
  if (path.rc != LIPASR_OK) return path.rc;
  if (path.fused) {
    set_error("lipasr_mfcc_plan_resample_ragged: this plan runs the fused resample -> STFT kernel for this input (rows of %d samples, "
              "alignment, or plan key 2): it has no resampled signal to return", p->n_samp);
    return LIPASR_EUNSUPPORTED;
  }
  int rc = launch_resample(p, path.resampler, wav, fmt, nv, batch, y, st);
  if (rc != LIPASR_OK) return rc;
  return launch_clear_tail(p, nv, batch, y, st);
}

static int plan_from_22k_ragged(MfccPlan* p, const float* y, const int* nv, int batch, int L, const double* am, const double* as,
                                float* out, hipStream_t st) {
  LP_CHECK_ARG(y && nv && out, "lipasr_mfcc_plan_from_22k_ragged: null argument");
  LP_CHECK_ARG((am == nullptr) == (as == nullptr), "lipasr_mfcc_plan_from_22k_ragged: give both affine arrays or neither");
  const MfccPath path = pick_mfcc_path(p, nullptr, 0, true);
  if (!stft2_ok(p)) {
    set_error("lipasr_mfcc_plan_from_22k_ragged: per-clip lengths need the 2048/512 kernels (n_fft %d, hop %d, stage mask %d)", p->n_fft,
              p->hop, p->stage_mask);
    return LIPASR_EUNSUPPORTED;
  }
  return launch_from_22k(p, path.stft, y, nv, batch, L, am, as, out, st);
}

// ---- the backward chain.  The three entry points (lipasr_mfcc_plan_vjp, _vjp_short, _vjp_ragged) describe their call; what
// differs between them is the named conditions of plan_vjp and nothing else ----
enum VjpEntry { VJ_ONE_LENGTH, VJ_SHORT, VJ_RAGGED };
struct VjpCall {
  const char* fn;
  VjpEntry entry;
  const void* sig;     // rows at the plan's input rate (domain 0) or at 22 050 Hz (domain 1)
  int fmt;             // 0: float32 samples, 1: int16 PCM
  const int* n_valid;  // per-clip sample counts at the plan's input rate (device), VJ_RAGGED only
  int domain, batch, L;
  const double* scale;
  const float* g_feat;
  float* g_sig;
  int flags;
};

static int plan_vjp(MfccPlan* p, const VjpCall& c, hipStream_t st) {
  const char* fn = c.fn;
  const int* nv = c.n_valid;
  const int domain = c.domain, batch = c.batch, L = c.L;
  int rc = plan_check(fn, p, batch, L);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(c.sig && c.g_feat && c.g_sig && (nv || c.entry != VJ_RAGGED), "%s: null argument", fn);
  LP_CHECK_ARG(c.fmt == 0 || c.fmt == 1, "%s: sample format %d (0 = float32, 1 = int16 PCM)", fn, c.fmt);
  LP_CHECK_ARG(domain == 0 || domain == 1, "%s: domain %d (0 = the plan's input rate, 1 = 22 050 Hz)", fn, domain);
  // allowed flag bits: 1 = reuse the caller's forward; the one-length entry also knows 2 and 4 by name, to refuse them
  LP_CHECK_ARG((c.flags & ~(c.entry == VJ_ONE_LENGTH ? 7 : 1)) == 0, "%s: unknown flag bits %d", fn, c.flags);
  if (c.flags & 6) {
    set_error("%s: int16 input and per-clip lengths have no backward pass (float32 rows of one length only)", fn);
    return LIPASR_EUNSUPPORTED;
  }
  // which plans the entry refuses
  if (c.entry == VJ_SHORT && !p->dft) {
    set_error("%s: the short-window backward pass covers the plans made with n_fft, hop other than 2048, 512; this plan is 2048/512 "
              "(lipasr_mfcc_plan_vjp)", fn);
    return LIPASR_EUNSUPPORTED;
  }
  if (c.entry != VJ_SHORT && p->dft) {
    set_error("%s: the backward pass covers the 2048/512 plans; this plan has n_fft %d, hop %d%s", fn, p->n_fft, p->hop,
              c.entry == VJ_ONE_LENGTH ? " (short-window plans: lipasr_mfcc_plan_vjp_short)" : "");
    return LIPASR_EUNSUPPORTED;
  }
  if (c.entry == VJ_ONE_LENGTH && p->n_y <= kNFft) {
    set_error("%s: the backward pass needs clips longer than the reflect padding (n_y %d <= %d)", fn, p->n_y, kNFft);
    return LIPASR_EUNSUPPORTED;
  }
  if (c.entry == VJ_RAGGED) {
    if (c.fmt == 1 && domain == 1) {
      set_error("%s: int16 PCM rows are rows at the plan's input rate (domain 0); the 22 050 Hz signal is float32", fn);
      return LIPASR_EUNSUPPORTED;
    }
    if ((rc = ragged_unsupported(fn, p)) != LIPASR_OK) return rc;
  }
  const MfccPath path = pick_mfcc_path(p, domain == 0 ? c.sig : nullptr, c.fmt, nv != nullptr);
  // whether path.rc is checked: the one-length entry does not (float32 rows of one length always have a three-kernel form)
  if (c.entry != VJ_ONE_LENGTH && path.rc != LIPASR_OK) return path.rc;
  if (c.entry == VJ_RAGGED && domain == 0 && path.fused) {
    set_error("%s: this plan runs the fused resample -> STFT kernel for this input (row alignment, or plan key 2), which leaves no "
              "resampled signal behind for the backward pass", fn);
    return LIPASR_EUNSUPPORTED;
  }
  if ((rc = c.entry == VJ_SHORT ? vjp_short_prepare(fn, p) : vjp_prepare(fn, p)) != LIPASR_OK) return rc;
  // What of the caller's forward is reused (flags bit 0).
  // d_y, the resampled signal: whenever the forward left one -- the one-length entry's fused resample -> STFT kernel leaves none
  // (the ragged entry has refused that case above).  It does not depend on the STFT kernel.
  // d_db / d_fmax, the tile: only where stft_mel2_kernel (or, on short-window plans, dft_mel_kernel) made it, which is also the
  // kernel the backward pass runs for itself.  The other 2048/512 kernels lose, on a quiet frame next to a loud one, digits that the
  // features never see (tolerance 2e-2) but that Gmel = Gdb (10 / ln 10) / mel magnifies: stft_bdft_kernel applies the Hann window
  // in the frequency domain, 0.5 X[k] - 0.25 (X[k-1] + X[k+1]) of the rectangular-window spectrum, and a burst under the tail of a
  // window cancels a large spectrum down to a small one that keeps the large one's 2^-22 (measured: mel powers 49 and 86 x further
  // from float64 than a float32 evaluation, 3 .. 4 x on other frames); stft_mel_kernel sends two frames of any loudness through one
  // transform.  stft_mel2_kernel windows in the time domain and scales every frame by itself.  Same bits either way.
  const MfccPath::Stft stft = p->dft ? MfccPath::ST_DFT : MfccPath::ST_STOCKHAM4;
  const bool reuse_y = (c.flags & 1) && !(c.entry == VJ_ONE_LENGTH && prefers_fused(p));
  const bool reuse_tile = (c.flags & 1) && path.stft == stft && (domain == 1 || reuse_y);
  const float* y = static_cast<const float*>(c.sig);
  if (domain == 0) {
    if (!reuse_y && (rc = launch_resample(p, path.resampler, c.sig, c.fmt, nv, batch, p->d_y, st)) != LIPASR_OK) return rc;
    y = p->d_y;
  }
  if (!reuse_tile && (rc = launch_from_22k(p, stft, y, nv, batch, L, nullptr, nullptr, nullptr, st, nullptr, true)) != LIPASR_OK) return rc;
  MfccVjpArgs a;
  a.y = y; a.n_y = p->n_y; a.n_frames = p->n_frames; a.batch = batch; a.L = L;
  a.db = p->d_db; a.fmax = p->d_fmax; a.g_feat = c.g_feat; a.aff_scale = c.scale; a.dct_rows = p->d_dct_rows;
  a.hann = p->d_hann; a.tw = reinterpret_cast<const float2*>(p->d_tw);
  a.mel_wlo = p->d_mel_wlo; a.mel_whi = p->d_mel_whi; a.bin_run = p->d_bin_run;
  a.gmel = p->d_gmel; a.part = p->d_part; a.n_groups = p->vj_groups;
  a.gy = domain == 0 ? p->d_gy : c.g_sig;
  // the middle stage: dB step, then dft_vjp_kernel (short window) or the Stockham adjoint, which takes the lengths
  if (c.entry == VJ_SHORT) {
    if ((rc = launch_mfcc_vjp_db(a, st)) != LIPASR_OK) return rc;
    ShortVjpArgs s;
    s.y = y; s.table = p->d_dft; s.table_t = p->d_dft_t; s.gmel = p->d_gmel;
    s.melt_off = p->d_melt_off; s.melt_len = p->d_melt_len; s.melt_m = p->d_melt_m; s.melt_w = p->d_melt_w;
    s.n_y = p->n_y; s.batch = batch; s.hop = p->hop; s.n_fft = p->n_fft; s.k_rows = p->dft_krows; s.n_tiles = p->dft_tiles;
    s.rpc = p->dft_rpc; s.n_frames = p->n_frames; s.total_rows = batch * p->dft_rpc; s.seg = 0;
    s.part = p->d_part; s.gy = a.gy;
    rc = launch_short_vjp(s, st);
  } else {
    rc = nv ? launch_mfcc_vjp(a, st, nv, p->sr_in, p->n_samp) : launch_mfcc_vjp(a, st);
  }
  if (rc != LIPASR_OK) return rc;
  if (domain == 0) return plan_resample_vjp(p, p->d_gy, batch, c.g_sig, st, nv);
  return LIPASR_OK;
}

static int plan_profile_begin(MfccPlan* p, int max_calls) {
  LP_CHECK_ARG(p != nullptr && max_calls >= 1 && max_calls <= 100000, "lipasr_mfcc_profile_begin: bad argument");
  DeviceGuard g(p->ctx->device);
  while ((int)p->prof_events.size() < kProfEvents * max_calls) {
    hipEvent_t e;
    LP_HIP(hipEventCreate(&e));
    p->prof_events.push_back(e);
  }
  p->prof_cap = max_calls;
  p->prof_n = 0;
  p->prof_half = false;
  return LIPASR_OK;
}

static int plan_profile_end(MfccPlan* p, float* avg_ms3, int* n_calls) {
  LP_CHECK_ARG(p && avg_ms3 && n_calls, "lipasr_mfcc_profile_end: null argument");
  double acc[3] = {0, 0, 0};
  static const int kFrom[3] = {EV_RESAMPLE_BEGIN, EV_STFT_BEGIN, EV_STFT_END}, kTo[3] = {EV_RESAMPLE_END, EV_STFT_END, EV_DCT_END};
  for (int i = 0; i < p->prof_n; ++i) {
    hipEvent_t* ev = &p->prof_events[kProfEvents * (size_t)i];
    LP_HIP(hipEventSynchronize(ev[EV_DCT_END]));
    for (int k = 0; k < 3; ++k) {
      float ms = 0.0f;
      LP_HIP(hipEventElapsedTime(&ms, ev[kFrom[k]], ev[kTo[k]]));
      acc[k] += ms;
    }
  }
  *n_calls = p->prof_n;
  for (int k = 0; k < 3; ++k) avg_ms3[k] = p->prof_n ? (float)(acc[k] / p->prof_n) : 0.0f;
  p->prof_cap = 0;
  p->prof_n = 0;
  p->prof_half = false;
  return LIPASR_OK;
}

static int plan_set(MfccPlan* p, int key, int value) {
  LP_CHECK_ARG(p != nullptr, "lipasr_mfcc_set: null plan");
  LP_CHECK_ARG(key >= 0 && key <= 4, "lipasr_mfcc_set: unknown key %d", key);
  if (key == 3) LP_CHECK_ARG(value >= 4 && value <= 4096 && (value & 3) == 0, "lipasr_mfcc_set: frames per workgroup %d (a multiple of 4)", value);
  if (key == 1) LP_CHECK_ARG(value >= 1 && value <= 4096, "lipasr_mfcc_set: resampler workgroup target %d", value);
  switch (key) {
    case 0: p->stage_mask = value; break;
    case 1: p->rs_target_wgs = value; break;
    case 2: p->prefer_fused = value != 0; break;
    case 3: p->bd_seg = value; break;
    default: p->bd_fuse_dct = value != 0; break;
  }
  return LIPASR_OK;
}

}  // namespace lipasr

extern "C" {

// ---------------------------------------------------------------- plan objects
int lipasr_mfcc_create(lipasr_handle_t h, int sr_in, int n_samp_max, int batch_max, int n_fft, int hop, lipasr_mfcc_t* out) {
  LP_CHECK_ARG(out != nullptr, "lipasr_mfcc_create: out is null");
  MfccPlan* p = nullptr;
  int rc = plan_build(h, sr_in, n_samp_max, batch_max, n_fft, hop, &p);
  if (rc != LIPASR_OK) return rc;
  *out = static_cast<lipasr_mfcc*>(p);
  return LIPASR_OK;
}

int lipasr_mfcc_destroy(lipasr_mfcc_t p) {
  LP_CHECK_ARG(p != nullptr, "lipasr_mfcc_destroy: null plan");
  DeviceGuard g(p->ctx->device);
  plan_unregister(p);
  mfcc_plan_free(p);
  return LIPASR_OK;
}

int lipasr_mfcc_plan_dims(lipasr_mfcc_t p, int* n_y, int* n_frames, int* fused) {
  LP_CHECK_ARG(p && n_y && n_frames, "lipasr_mfcc_plan_dims: null argument");
  *n_y = p->n_y;
  *n_frames = p->n_frames;
  if (fused) *fused = p->fused ? 1 : 0;
  return LIPASR_OK;
}

int lipasr_mfcc_extract(lipasr_mfcc_t p, const void* wav, int sample_format, const int* n_valid, int batch, int utterance_length,
                        const double* affine_mean, const double* affine_scale, float* out, lipasr_stream_t stream) {
  int rc = plan_check("lipasr_mfcc_extract", p, batch, utterance_length);
  if (rc != LIPASR_OK) return rc;
  return plan_run(p, wav, sample_format, n_valid, batch, utterance_length, affine_mean, affine_scale, out, S(stream));
}

int lipasr_mfcc_plan_resample(lipasr_mfcc_t p, const float* wav, int batch, float* y, lipasr_stream_t stream) {
  int rc = plan_check("lipasr_mfcc_plan_resample", p, batch, 1);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(wav && y, "lipasr_mfcc_plan_resample: null argument");
  return plan_resample(p, wav, batch, y, S(stream));
}

int lipasr_mfcc_plan_from_22k(lipasr_mfcc_t p, const float* y, int batch, int n_y, int utterance_length, const double* affine_mean,
                              const double* affine_scale, float* out, lipasr_stream_t stream) {
  int rc = plan_check("lipasr_mfcc_plan_from_22k", p, batch, utterance_length);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(y && out, "lipasr_mfcc_plan_from_22k: null argument");
  return plan_from_22k(p, y, batch, n_y, utterance_length, affine_mean, affine_scale, out, S(stream));
}

int lipasr_mfcc_plan_vjp(lipasr_mfcc_t p, const float* sig, int domain, int batch, int utterance_length, const double* affine_scale,
                         const float* g_feat, float* g_sig, int flags, lipasr_stream_t stream) {
  return plan_vjp(p, {"lipasr_mfcc_plan_vjp", VJ_ONE_LENGTH, sig, 0, nullptr, domain, batch, utterance_length, affine_scale, g_feat, g_sig, flags},
                  S(stream));
}

int lipasr_mfcc_plan_vjp_short(lipasr_mfcc_t p, const float* sig, int domain, int batch, int utterance_length, const double* affine_scale,
                               const float* g_feat, float* g_sig, int flags, lipasr_stream_t stream) {
  return plan_vjp(p, {"lipasr_mfcc_plan_vjp_short", VJ_SHORT, sig, 0, nullptr, domain, batch, utterance_length, affine_scale, g_feat, g_sig, flags},
                  S(stream));
}

int lipasr_mfcc_plan_vjp_ragged(lipasr_mfcc_t p, const void* sig, int sample_format, const int* n_valid, int domain, int batch,
                                int utterance_length, const double* affine_scale, const float* g_feat, float* g_sig, int flags,
                                lipasr_stream_t stream) {
  return plan_vjp(p, {"lipasr_mfcc_plan_vjp_ragged", VJ_RAGGED, sig, sample_format, n_valid, domain, batch, utterance_length, affine_scale,
                      g_feat, g_sig, flags},
                  S(stream));
}

int lipasr_mfcc_plan_resample_ragged(lipasr_mfcc_t p, const void* wav, int sample_format, const int* n_valid, int batch, float* y,
                                     lipasr_stream_t stream) {
  int rc = plan_check("lipasr_mfcc_plan_resample_ragged", p, batch, 1);
  if (rc != LIPASR_OK) return rc;
  return plan_resample_ragged(p, wav, sample_format, n_valid, batch, y, S(stream));
}

int lipasr_mfcc_plan_from_22k_ragged(lipasr_mfcc_t p, const float* y, const int* n_valid, int batch, int utterance_length,
                                     const double* affine_mean, const double* affine_scale, float* out, lipasr_stream_t stream) {
  int rc = plan_check("lipasr_mfcc_plan_from_22k_ragged", p, batch, utterance_length);
  if (rc != LIPASR_OK) return rc;
  return plan_from_22k_ragged(p, y, n_valid, batch, utterance_length, affine_mean, affine_scale, out, S(stream));
}

int lipasr_mfcc_plan_resample_vjp(lipasr_mfcc_t p, const float* g_y, int batch, float* g_wav, lipasr_stream_t stream) {
  int rc = plan_check("lipasr_mfcc_plan_resample_vjp", p, batch, 1);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(g_y && g_wav, "lipasr_mfcc_plan_resample_vjp: null argument");
  return plan_resample_vjp(p, g_y, batch, g_wav, S(stream));
}

int lipasr_mfcc_plan_profile_begin(lipasr_mfcc_t p, int max_calls) { return plan_profile_begin(p, max_calls); }
int lipasr_mfcc_plan_profile_end(lipasr_mfcc_t p, float* avg_ms3, int* n_calls) { return plan_profile_end(p, avg_ms3, n_calls); }
int lipasr_mfcc_plan_set(lipasr_mfcc_t p, int key, int value) { return plan_set(p, key, value); }

// ---------------------------------------------------------------- test hooks of the forward pass
long lipasr_debug_k1_launches(int kernel) { return (kernel >= 0 && kernel < K1_KERNELS) ? g_k1_launches[kernel] : -1; }

int lipasr_debug_mfcc_stage(lipasr_mfcc_t p, int which, int batch, float* out, lipasr_stream_t stream) {
  LP_CHECK_ARG(p != nullptr && out != nullptr, "lipasr_debug_mfcc_stage: null argument");
  LP_CHECK_ARG(batch >= 1 && batch <= p->batch_max, "lipasr_debug_mfcc_stage: batch %d outside [1, %d]", batch, p->batch_max);
  LP_CHECK_ARG(which >= 0 && which <= 2, "lipasr_debug_mfcc_stage: unknown stage %d (0 dB tile, 1 frame maxima, 2 resampled signal)", which);
  const float* src = which == 0 ? p->d_db : which == 1 ? p->d_fmax : p->d_y;
  const size_t row = which == 0 ? (size_t)p->n_frames * 128 : which == 1 ? (size_t)p->n_frames : (size_t)p->n_y;
  DeviceGuard g(p->ctx->device);
  LP_HIP(hipMemcpyAsync(out, src, (size_t)batch * row * sizeof(float), hipMemcpyDeviceToDevice, S(stream)));
  return LIPASR_OK;
}

// ---------------------------------------------------------------- test hooks of the backward pass
long lipasr_debug_k1_vjp_launches(int kernel) { return (kernel >= 0 && kernel < K1V_KERNELS) ? g_k1_vjp_launches[kernel] : -1; }

int lipasr_debug_mfcc_vjp_stage(lipasr_mfcc_t p, int which, int batch, float* out, lipasr_stream_t stream) {
  LP_CHECK_ARG(p != nullptr && out != nullptr, "lipasr_debug_mfcc_vjp_stage: null argument");
  LP_CHECK_ARG(batch >= 1 && batch <= p->batch_max, "lipasr_debug_mfcc_vjp_stage: batch %d outside [1, %d]", batch, p->batch_max);
  LP_CHECK_ARG(which >= 0 && which <= 1, "lipasr_debug_mfcc_vjp_stage: unknown stage %d (0 Gmel, 1 g_y of a domain-0 call)", which);
  LP_CHECK_ARG(p->vj_ready && p->d_gmel && p->d_gy, "lipasr_debug_mfcc_vjp_stage: the plan has run no backward pass yet (no workspaces)");
  const float* src = which == 0 ? p->d_gmel : p->d_gy;
  const size_t row = which == 0 ? (size_t)p->n_frames * 128 : (size_t)p->n_y;
  DeviceGuard g(p->ctx->device);
  LP_HIP(hipMemcpyAsync(out, src, (size_t)batch * row * sizeof(float), hipMemcpyDeviceToDevice, S(stream)));
  return LIPASR_OK;
}

int lipasr_debug_mfcc_stage_put(lipasr_mfcc_t p, int which, int batch, const float* in, lipasr_stream_t stream) {
  LP_CHECK_ARG(p != nullptr && in != nullptr, "lipasr_debug_mfcc_stage_put: null argument");
  LP_CHECK_ARG(batch >= 1 && batch <= p->batch_max, "lipasr_debug_mfcc_stage_put: batch %d outside [1, %d]", batch, p->batch_max);
  LP_CHECK_ARG(which >= 0 && which <= 1, "lipasr_debug_mfcc_stage_put: unknown stage %d (0 dB tile, 1 frame maxima)", which);
  float* dst = which == 0 ? p->d_db : p->d_fmax;
  const size_t row = which == 0 ? (size_t)p->n_frames * 128 : (size_t)p->n_frames;
  DeviceGuard g(p->ctx->device);
  LP_HIP(hipMemcpyAsync(dst, in, (size_t)batch * row * sizeof(float), hipMemcpyDeviceToDevice, S(stream)));
  return LIPASR_OK;
}

// ---------------------------------------------------------------- the handle's default plan (round-1/2 entry points)
int lipasr_mfcc_plan(lipasr_handle_t h, int sr_in, int n_samp, int batch_max) {
  return lipasr_mfcc_plan_ex(h, sr_in, n_samp, batch_max, kNFft, kHop);
}

int lipasr_mfcc_plan_ex(lipasr_handle_t h, int sr_in, int n_samp, int batch_max, int n_fft, int hop) {
  LP_CHECK_ARG(h != nullptr, "lipasr_mfcc_plan: null handle");
  MfccPlan* p = nullptr;
  int rc = plan_build(h, sr_in, n_samp, batch_max, n_fft, hop, &p);
  if (rc != LIPASR_OK) return rc;
  if (h->mfcc) {
    DeviceGuard g(h->device);
    MfccPlan* old = h->mfcc;
    plan_unregister(old);
    mfcc_plan_free(old);
  }
  h->mfcc = p;
  return LIPASR_OK;
}

int lipasr_mfcc_dims(lipasr_handle_t h, int* n_y, int* n_frames) {
  LP_CHECK_ARG(h && n_y && n_frames, "lipasr_mfcc_dims: null argument");
  if (!h->mfcc) { set_error("lipasr_mfcc_dims: call lipasr_mfcc_plan first"); return LIPASR_ESTATE; }
  *n_y = h->mfcc->n_y;
  *n_frames = h->mfcc->n_frames;
  return LIPASR_OK;
}

static int mfcc_check(const char* fn, lipasr_handle_t h, int batch, int L) {
  LP_CHECK_ARG(h != nullptr, "%s: null handle", fn);
  if (!h->mfcc) { set_error("%s: call lipasr_mfcc_plan first", fn); return LIPASR_ESTATE; }
  return plan_check(fn, h->mfcc, batch, L);
}

int lipasr_resample_f32(lipasr_handle_t h, const float* wav, int batch, float* y, lipasr_stream_t stream) {
  int rc = mfcc_check("lipasr_resample_f32", h, batch, 1);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(wav && y, "lipasr_resample_f32: null argument");
  return plan_resample(h->mfcc, wav, batch, y, S(stream));
}

int lipasr_mfcc_from_22k(lipasr_handle_t h, const float* y, int batch, int n_y, int utterance_length,
                         const double* affine_mean, const double* affine_scale, float* out, lipasr_stream_t stream) {
  int rc = mfcc_check("lipasr_mfcc_from_22k", h, batch, utterance_length);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(y && out, "lipasr_mfcc_from_22k: null argument");
  return plan_from_22k(h->mfcc, y, batch, n_y, utterance_length, affine_mean, affine_scale, out, S(stream));
}

int lipasr_mfcc_f32(lipasr_handle_t h, const float* wav, int batch, int utterance_length, const double* affine_mean,
                    const double* affine_scale, float* out, lipasr_stream_t stream) {
  int rc = mfcc_check("lipasr_mfcc_f32", h, batch, utterance_length);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(wav && out, "lipasr_mfcc_f32: null argument");
  LP_CHECK_ARG((affine_mean == nullptr) == (affine_scale == nullptr), "lipasr_mfcc_f32: give both affine arrays or neither");
  return plan_run(h->mfcc, wav, 0, nullptr, batch, utterance_length, affine_mean, affine_scale, out, S(stream));
}

int lipasr_mfcc_i16(lipasr_handle_t h, const int16_t* pcm, const int* n_valid, int batch, int utterance_length,
                    const double* affine_mean, const double* affine_scale, float* out, lipasr_stream_t stream) {
  int rc = mfcc_check("lipasr_mfcc_i16", h, batch, utterance_length);
  if (rc != LIPASR_OK) return rc;
  return plan_run(h->mfcc, pcm, 1, n_valid, batch, utterance_length, affine_mean, affine_scale, out, S(stream));
}

int lipasr_mfcc_profile_begin(lipasr_handle_t h, int max_calls) {
  LP_CHECK_ARG(h != nullptr, "lipasr_mfcc_profile_begin: bad argument");
  if (!h->mfcc) { set_error("lipasr_mfcc_profile_begin: call lipasr_mfcc_plan first"); return LIPASR_ESTATE; }
  return plan_profile_begin(h->mfcc, max_calls);
}

int lipasr_mfcc_profile_end(lipasr_handle_t h, float* avg_ms3, int* n_calls) {
  LP_CHECK_ARG(h && avg_ms3 && n_calls, "lipasr_mfcc_profile_end: null argument");
  if (!h->mfcc) { set_error("lipasr_mfcc_profile_end: call lipasr_mfcc_plan first"); return LIPASR_ESTATE; }
  return plan_profile_end(h->mfcc, avg_ms3, n_calls);
}

int lipasr_add_noise_f32(lipasr_handle_t h, float* y, int batch, int n, int mode, float p0, float p1, uint64_t seed,
                         lipasr_stream_t stream) {
  LP_CHECK_ARG(h && y, "lipasr_add_noise_f32: null argument");
  LP_CHECK_ARG(batch >= 1 && n >= 1, "lipasr_add_noise_f32: bad shape %dx%d", batch, n);
  LP_CHECK_ARG(mode >= 0 && mode <= 2, "lipasr_add_noise_f32: mode %d", mode);
  hipLaunchKernelGGL(add_noise_kernel, dim3(batch), dim3(256), 0, S(stream), y, n, mode, p0, p1, seed);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

/* Knobs of the handle's default plan (lipasr_mfcc_plan_set is the per-plan form; the stage-mask bits of key 0 are listed
 * there in include/lipasr.h).  key 1: workgroups the persistent resampler of the three-kernel path aims for. */
int lipasr_debug_set(lipasr_handle_t h, int key, int value) {
  LP_CHECK_ARG(h != nullptr, "lipasr_debug_set: null handle");
  LP_CHECK_ARG(key >= 0 && key <= 2, "lipasr_debug_set: unknown key %d", key);
  if (!h->mfcc) { set_error("lipasr_debug_set: call lipasr_mfcc_plan first"); return LIPASR_ESTATE; }
  int rc = plan_set(h->mfcc, key, value);
  if (rc == LIPASR_OK && key == 1) h->rs_target_wgs = value;  // kept in the handle: a later lipasr_mfcc_plan inherits it
  return rc;
}

/* Host-only: copies one constant table (as the kernels see it) into `out`; returns the element count
 * (or a negative error).  which: 0 hann[2048], 1 dct[20*128], 2 dense mel[128*1025], 3 polyphase taps
 * [up*taps] for sr_in, 4 polyphase meta {up, down, taps, left} as floats, 5 phase offsets as floats. */
int lipasr_debug_table(int which, int sr_in, float* out, int cap) {
  std::vector<float> v;
  switch (which) {
    case 0: v = hann_periodic(); break;
    case 1: v = dct_matrix(); break;
    case 2: v = mel_dense(); break;
    case 3: case 4: case 5: case 6: case 7: {
      LP_CHECK_ARG(sr_in >= 1000 && sr_in != kSr, "lipasr_debug_table: sr_in=%d", sr_in);
      Polyphase pp = build_polyphase(sr_in, kSr);
      if (which == 3) v = pp.h;
      else if (which == 4) v = {(float)pp.up, (float)pp.down, (float)pp.taps, (float)pp.left};
      else if (which == 5) v.assign(pp.n_off.begin(), pp.n_off.end());
      else {
        std::vector<float> hb;
        std::vector<int> lo;
        if (!build_band_tables(pp, &hb, &lo)) { set_error("lipasr_debug_table: no banded form for sr_in=%d", sr_in); return LIPASR_EUNSUPPORTED; }
        if (which == 6) v = hb;
        else v.assign(lo.begin(), lo.end());
      }
      break;
    }
    case 8: {  // the mel bank as the kernel applies it (pair form), expanded to dense [128*1025]
      MelPairs mp = mel_pairs();
      LP_CHECK_ARG(mp.ok, "lipasr_debug_table: mel bank has no pair form");
      v.assign((size_t)kNMels * kNBins, 0.0f);
      for (int m = 0; m < kNMels; ++m)
        for (int i = 0; i < mp.len[m]; ++i) {
          const int b = mp.start[m] + i;
          v[(size_t)m * kNBins + b] += mp.wlo[b];
          if (m + 1 < kNMels) v[(size_t)(m + 1) * kNBins + b] += mp.whi[b];
        }
      break;
    }
    default: set_error("lipasr_debug_table: unknown table %d", which); return LIPASR_EINVAL;
  }
  if (out) {
    LP_CHECK_ARG((size_t)cap >= v.size(), "lipasr_debug_table: capacity %d < %zu", cap, v.size());
    memcpy(out, v.data(), v.size() * sizeof(float));
  }
  return (int)v.size();
}

}  // extern "C"
