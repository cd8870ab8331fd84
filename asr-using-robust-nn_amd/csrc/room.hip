// The over-the-air channel: a bank of room impulse responses in front of the MFCC stage (lipasr/room.py, OverTheAirClassifier).
//
//   lipasr_room_apply   out[b * R + j][t] = sum_{k <= min(t, taps - 1)} rirs[j][k] * x[b][t - k]           (t < nv_b, else 0)
//   lipasr_room_vjp     gx[b][s] = scale * sum_j sum_{k < taps, s + k < nv_b} rirs[j][k] * g[b * R + j][s + k]   (s < nv_b, else 0)
//
// Both are one launch of room_kernel, the resampler's contraction (resample_mfma_kernel) with the taps themselves as the banded
// operand.  For one room j a tile of 32 clips x 32 output times is
//       Y[clip i][col] = sum_kk  X[i][p0 + kk] * Toeplitz(h_j)[kk][col]
// on v_mfma_f32_32x32x2_f32 (an exact fp32 fma chain per output element; the zero entries of the band add exact zeros to a
// finite signal).  A workgroup is 4 wavefronts = 32 clips x 128 output times of one room (apply) or of the sum over all rooms
// (vjp, the loop over j feeds the same accumulator).  The room's taps sit in LDS between two pads of 96 zeros, so the B operand
// is the plain read h[k] with k = t - p (apply) or k = p - s (vjp) and no branch; the signal goes through LDS in chunks of 64
// positions x 32 rows (row stride 65 = 1 mod 32: the A-operand read `lane i -> row i` is conflict-free), the next chunk's 8
// loads per thread in flight while the current one feeds 32 MFMAs per wavefront.  A wavefront skips a chunk none of whose 64 x 32
// (position, time) pairs has a tap; which chunks it takes depends on the tile's position alone, so that a row's sum runs in one
// fixed order: by room, then by position upwards.  Loads and stores are single floats (coalesced along time): any alignment.
// Nothing here allocates, synchronises or waits on another workgroup.
#include "common.h"
#include "row.h"

namespace lipasr {

typedef float room_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kRoomWaves = 4;                // wavefronts of a workgroup, one 32 x 32 tile each
constexpr int kRoomTimes = 32 * kRoomWaves;  // output times of a workgroup
constexpr int kRoomChunk = 64;               // signal positions staged per step
constexpr int kRoomStride = kRoomChunk + 1;
constexpr int kRoomPad = 96;                 // zeros on either side of the taps: a chunk a wavefront takes has k in [-94, taps + 93]
constexpr int kRoomRegs = 32 * kRoomChunk / (64 * kRoomWaves);
constexpr int kRoomMaxTaps = 8192;
constexpr int kRoomMaxN = 1 << 30;

static size_t room_lds_bytes(int taps) { return ((size_t)taps + 2 * kRoomPad + 32 * kRoomStride + 32) * sizeof(float); }

// ADJ = false: src = x [clips][n], dst = out [clips * R][n], one room per workgroup.
// ADJ = true:  src = g [clips * R][n], dst = gx [clips][n], every room in turn.
template <bool ADJ>
__global__ __launch_bounds__(64 * kRoomWaves) void room_kernel(const float* __restrict__ src, const int* __restrict__ n_valid,
                                                               const float* __restrict__ rirs, int taps, int R, int clips, int n,
                                                               int ttiles, int ctiles, float scale, float* __restrict__ dst) {
  extern __shared__ __attribute__((aligned(16))) float room_lds[];
  float* hs = room_lds;                      // [kRoomPad + taps + kRoomPad]; hs[kRoomPad + k] = h_j[k]
  float* xs = hs + taps + 2 * kRoomPad;      // [32][kRoomStride]; xs[i][c] = row i at position p0 + c
  int* nvs = reinterpret_cast<int*>(xs + 32 * kRoomStride);  // [32] clamped n_valid of the tile's clips, 0 past the batch
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, h = lane >> 5;
  const int L = blockIdx.x;
  const int tt = L % ttiles, rest = L / ttiles;
  const int ct = rest % ctiles, j0 = rest / ctiles;
  const int c0 = ct * 32, t0 = tt * kRoomTimes;
  if (tid < 32) {
    const int c = c0 + tid;
    int v = 0;
    if (c < clips) v = row_valid(n_valid, c, n);
    nvs[tid] = v;
  }
  __syncthreads();
  int nvmax = 0;
#pragma unroll
  for (int i = 0; i < 32; ++i) nvmax = max(nvmax, nvs[i]);
  room_f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
  const int tw = t0 + 32 * wave;  // first output time of this wavefront's tile
  if (t0 < nvmax) {
    // positions the workgroup's outputs read: [t0 - taps + 1, t0 + 127] (apply), [t0, t0 + 127 + taps - 1] (vjp), below nvmax
    const int pstart = ADJ ? t0 : t0 - (taps - 1);
    const int plast = ADJ ? min(t0 + kRoomTimes - 1 + taps - 1, nvmax - 1) : min(t0 + kRoomTimes - 1, nvmax - 1);
    const int cbeg = pstart < 0 ? (-pstart) / kRoomChunk : 0;
    const int cend = (plast - pstart) / kRoomChunk + 1;
    const int frow = tid >> 6, fcol = tid & 63;  // this thread fills rows frow + 4 r at column fcol
    int nvr[kRoomRegs];
#pragma unroll
    for (int r = 0; r < kRoomRegs; ++r) nvr[r] = nvs[frow + 4 * r];
    const int jbeg = ADJ ? 0 : j0, jend = ADJ ? R : j0 + 1;
    for (int j = jbeg; j < jend; ++j) {
      __syncthreads();  // the previous room's taps and last chunk are read
      const float* hj = rirs + (size_t)j * taps;
      for (int idx = tid; idx < taps + 2 * kRoomPad; idx += 64 * kRoomWaves) {
        const int k = idx - kRoomPad;
        hs[idx] = (k >= 0 && k < taps) ? hj[k] : 0.0f;
      }
      float pre[kRoomRegs];
      auto fetch = [&](int p0) {
        const int p = p0 + fcol;
#pragma unroll
        for (int r = 0; r < kRoomRegs; ++r) {
          const int c = c0 + frow + 4 * r;
          const size_t row = ADJ ? (size_t)c * R + j : (size_t)c;
          pre[r] = (p >= 0 && p < nvr[r]) ? src[row * (size_t)n + p] : 0.0f;
        }
      };
      fetch(pstart + cbeg * kRoomChunk);
      for (int c = cbeg; c < cend; ++c) {
        const int p0 = pstart + c * kRoomChunk;
        __syncthreads();  // the previous chunk is read
#pragma unroll
        for (int r = 0; r < kRoomRegs; ++r) xs[(frow + 4 * r) * kRoomStride + fcol] = pre[r];
        __syncthreads();
        if (c + 1 < cend) fetch(p0 + kRoomChunk);
        // k over this wavefront's 64 positions x 32 times
        const int kmin = ADJ ? p0 - (tw + 31) : tw - (p0 + kRoomChunk - 1);
        const int kmax = ADJ ? p0 + kRoomChunk - 1 - tw : tw + 31 - p0;
        if (kmax < 0 || kmin >= taps) continue;
        const float* xa = xs + li * kRoomStride + h;
        if (ADJ) {
          const float* hb = hs + kRoomPad + (p0 + h - (tw + li));
#pragma unroll
          for (int s = 0; s < kRoomChunk / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[2 * s], hb[2 * s], acc, 0, 0, 0);
        } else {
          const float* hb = hs + kRoomPad + (tw + li - p0 - h);
#pragma unroll
          for (int s = 0; s < kRoomChunk / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[2 * s], hb[-2 * s], acc, 0, 0, 0);
        }
      }
    }
  }
  const int t = tw + li;
  if (t < n) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int i = (e & 3) + 8 * (e >> 2) + 4 * h;
      const int c = c0 + i;
      if (c < clips) {
        const size_t row = ADJ ? (size_t)c : (size_t)c * R + j0;
        const float v = ADJ ? acc[e] * scale : acc[e];
        dst[row * (size_t)n + t] = t < nvs[i] ? v : 0.0f;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------ checks
// sig: the [clips][n] side (x or gx); rows: the [clips * R][n] side (out or g); dst: the one of the two that is written
static int room_check(const char* fn, const float* sig, const float* rows, const float* rirs, int taps, int R, int clips, int n,
                      const float* dst, float scale) {
  LP_CHECK_ARG(clips >= 0 && R >= 0 && n >= 0, "%s: bad shape %d x %d x %d", fn, clips, R, n);
  LP_CHECK_ARG(taps >= 1 && taps <= kRoomMaxTaps, "%s: %d taps; 1 to %d are supported", fn, taps, kRoomMaxTaps);
  LP_CHECK_ARG(n <= kRoomMaxN, "%s: rows of %d elements; at most 2^30", fn, n);
  LP_CHECK_ARG((long long)clips * R <= 0x7fffffffLL, "%s: %d x %d rows", fn, clips, R);
  LP_CHECK_ARG(scale == scale && std::fabs(scale) < INFINITY, "%s: scale %g", fn, (double)scale);
  if (clips == 0 || R == 0 || n == 0) return LIPASR_OK;
  LP_CHECK_ARG(sig != nullptr && rows != nullptr && rirs != nullptr, "%s: a null pointer", fn);
  const size_t sb = (size_t)clips * n * 4, rb = (size_t)clips * R * n * 4, hb = (size_t)R * taps * 4;
  const void* other = dst == sig ? (const void*)rows : (const void*)sig;
  const size_t db = dst == sig ? sb : rb, ob = dst == sig ? rb : sb;
  LP_CHECK_ARG(!spans_overlap(dst, db, other, ob) && !spans_overlap(dst, db, rirs, hb), "%s: the output overlaps an input", fn);
  return LIPASR_OK;
}

template <bool ADJ>
static int room_launch(const char* fn, const float* src, const int* n_valid, const float* rirs, int taps, int R, int clips, int n,
                       float scale, float* dst, lipasr_stream_t stream) {
  const long long ttiles = ((long long)n + kRoomTimes - 1) / kRoomTimes, ctiles = ((long long)clips + 31) / 32;
  const long long wgs = ttiles * ctiles * (ADJ ? 1 : R);
  LP_CHECK_ARG(wgs <= 0x7fffffffLL, "%s: %lld workgroups; split the batch", fn, wgs);
  const size_t lds = room_lds_bytes(taps);  // 42 kB at 8 192 taps: below the 48 kB a kernel takes without asking
  hipLaunchKernelGGL(room_kernel<ADJ>, dim3((unsigned)wgs), dim3(64 * kRoomWaves), lds, S(stream), src, n_valid, rirs, taps, R, clips,
                     n, (int)ttiles, (int)ctiles, scale, dst);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

// one tap of the host twins: the exact product added to the fp32 accumulator, rounded to fp32 (through float64, which holds the
// product of two floats exactly: what tests/room_ref.py restates in NumPy)
static inline float room_tap(float acc, float h, float v) { return (float)((double)acc + (double)h * (double)v); }

}  // namespace lipasr

using namespace lipasr;

extern "C" {

int lipasr_room_apply(const float* x, const int* n_valid, const float* rirs, int taps, int rir_count, int clips, int n, float* out,
                      lipasr_stream_t stream) {
  const char* fn = "lipasr_room_apply";
  if (int rc = room_check(fn, x, out, rirs, taps, rir_count, clips, n, out, 1.0f)) return rc;
  if (clips == 0 || rir_count == 0 || n == 0) return LIPASR_OK;
  return room_launch<false>(fn, x, n_valid, rirs, taps, rir_count, clips, n, 1.0f, out, stream);
}

int lipasr_room_vjp(const float* g, const int* n_valid, const float* rirs, int taps, int rir_count, int clips, int n, float scale,
                    float* gx, lipasr_stream_t stream) {
  const char* fn = "lipasr_room_vjp";
  if (int rc = room_check(fn, gx, g, rirs, taps, rir_count, clips, n, gx, scale)) return rc;
  if (clips == 0 || rir_count == 0 || n == 0) return LIPASR_OK;
  return room_launch<true>(fn, g, n_valid, rirs, taps, rir_count, clips, n, scale, gx, stream);
}

int lipasr_room_apply_host(const float* x, const int* n_valid, const float* rirs, int taps, int rir_count, int clips, int n,
                           float* out) {
  const char* fn = "lipasr_room_apply_host";
  if (int rc = room_check(fn, x, out, rirs, taps, rir_count, clips, n, out, 1.0f)) return rc;
  for (int b = 0; b < clips; ++b) {
    const int nv = row_valid(n_valid, b, n);
    const float* xr = x + (size_t)b * n;
    for (int j = 0; j < rir_count; ++j) {
      const float* hj = rirs + (size_t)j * taps;
      float* o = out + ((size_t)b * rir_count + j) * n;
      // o[t] takes its taps in the order k = 0, 1, ...; the loop over t is the inner one only so that it vectorises
      for (int t = 0; t < n; ++t) o[t] = 0.0f;
      for (int k = 0; k < std::min(taps, nv); ++k)
        for (int t = k; t < nv; ++t) o[t] = room_tap(o[t], hj[k], xr[t - k]);
    }
  }
  return LIPASR_OK;
}

int lipasr_room_vjp_host(const float* g, const int* n_valid, const float* rirs, int taps, int rir_count, int clips, int n,
                         float scale, float* gx) {
  const char* fn = "lipasr_room_vjp_host";
  if (int rc = room_check(fn, gx, g, rirs, taps, rir_count, clips, n, gx, scale)) return rc;
  for (int b = 0; b < clips; ++b) {
    const int nv = row_valid(n_valid, b, n);
    float* o = gx + (size_t)b * n;
    // o[s] takes its taps in (j, k) order; the loop over s is the inner one only so that it vectorises
    for (int s = 0; s < n; ++s) o[s] = 0.0f;
    for (int j = 0; j < rir_count; ++j) {
      const float* hj = rirs + (size_t)j * taps;
      const float* gr = g + ((size_t)b * rir_count + j) * n;
      for (int k = 0; k < std::min(taps, nv); ++k)
        for (int s = 0; s + k < nv; ++s) o[s] = room_tap(o[s], hj[k], gr[s + k]);
    }
    for (int s = 0; s < nv; ++s) o[s] = scale * o[s];
  }
  return LIPASR_OK;
}

}  // extern "C"
