// Randomized smoothing (Cohen, Rosenfeld, Kolter 2019): the two kernels around the classifier in CERTIFY / PREDICT, and the host
// table of the noise they draw.  (include/lipasr.h, lipasr_smooth_expand / lipasr_smooth_vote, fixes the conventions.)
//
// smooth_expand_kernel: ONE workgroup of 256 threads per OUTPUT row b * draws + j, one launch per call, no workspace, no atomics.
//   A lane takes the quads k >> 2 = tid, tid + 256, ... of its row: one Philox block keyed (seed; quad, clip0 + b, draw0 + j), one
//   normal4, out = clamp(fmaf(sigma, z, x)) on the elements below the clip's valid length, the bits of x on the others.  A quad
//   that lies wholly in the padding is copied without a draw.  The counter holds the clip and the draw, never the row's position
//   in the call, so a chunk of any size at any start draws what one big call would.
//   The quads move as row.h says, `whole` judged per array: x and out are told apart, so an aligned x with an odd out still
//   loads float4.
//   The kernel is bound by vector-instruction issue, not by HBM: ten Philox rounds (20 v_mul_hi/lo pairs) plus two logf, two
//   sqrtf and two sincosf per 32 bytes moved.  Nothing here chases the memory roofline.
//
// smooth_vote_kernel: ONE workgroup of 256 threads per clip.  A lane takes rows j = tid, tid + 256, ... of its clip's draws and
//   finds the row's bin: argmax (lowest index on a tie, +inf a maximum like any other), or bin `classes` if any entry is NaN.
//   Per wave the bins are counted by ballot and popcount (lane c keeps bin c), the four waves are summed through LDS in a fixed
//   order, and thread c adds the sum to counts[b][c], which no other workgroup touches: no global atomics, the same bits on
//   every run, and calls accumulate.
#include "common.h"
#include "row.h"

namespace lipasr {

constexpr int kSmThreads = 256;
constexpr int kSmWaves = kSmThreads / 64;
constexpr int kSmMaxC = 32;
extern long g_smooth_launches[2];  // smooth_train.hip (lipasr_debug_smooth_loss_launches): id 1 counts smooth_expand_kernel

__global__ __launch_bounds__(kSmThreads) void smooth_expand_kernel(const float* __restrict__ x, const int* __restrict__ n_valid,
                                                                    int n, int draws, uint32_t clip0, uint32_t draw0, float sigma,
                                                                    uint64_t seed, float lo, float hi, float* __restrict__ out) {
  const size_t row = blockIdx.x;
  const int b = (int)(row / (size_t)draws), j = (int)(row % (size_t)draws);
  const int tid = threadIdx.x;
  const float* __restrict__ xr = x + (size_t)b * n;
  float* __restrict__ orow = out + row * (size_t)n;
  const int nv = row_valid(n_valid, b, n);
  const bool xvec = (reinterpret_cast<uintptr_t>(xr) & 15) == 0, ovec = (reinterpret_cast<uintptr_t>(orow) & 15) == 0;  // uniform
  const uint32_t clip = clip0 + (uint32_t)b, draw = draw0 + (uint32_t)j;
  const int quads = (n + 3) >> 2;
  for (int q = tid; q < quads; q += kSmThreads) {
    const int k0 = q * 4;
    const bool full = k0 + 4 <= n;
    float v[4];
    ld4(xr, k0, n, full && xvec, v);
    if (k0 < nv) {
      float z[4];
      normal4(seed, (uint64_t)q, clip, draw, z);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (k0 + e < nv) v[e] = clampf(fmaf(sigma, z[e], v[e]), lo, hi);
      }
    }
    st4(orow, k0, n, full && ovec, v);
  }
}

__global__ __launch_bounds__(kSmThreads) void smooth_vote_kernel(const float* __restrict__ logits, int draws, int C,
                                                                  int* __restrict__ counts) {
  __shared__ int part[kSmWaves][kSmMaxC + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t b = blockIdx.x;
  const float* __restrict__ L = logits + b * (size_t)draws * (size_t)C;
  int cnt = 0;  // lane c: this wave's rows in bin c
  for (int j0 = wave * 64; j0 < draws; j0 += kSmThreads) {  // uniform per wave
    const int j = j0 + lane;
    int bin = -1;
    if (j < draws) {
      const float* __restrict__ r = L + (size_t)j * C;
      float top = r[0];
      bool nan = top != top;
      bin = 0;
      for (int c = 1; c < C; ++c) {
        const float v = r[c];
        nan |= v != v;
        if (v > top) { top = v; bin = c; }
      }
      if (nan) bin = C;
    }
    for (int c = 0; c <= C; ++c) {
      const int votes = __popcll(__ballot(bin == c));
      if (lane == c) cnt += votes;
    }
  }
  if (lane <= C) part[wave][lane] = cnt;
  __syncthreads();
  if (tid <= C) counts[b * (size_t)(C + 1) + tid] += ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

int lipasr_smooth_expand(lipasr_handle_t h, const float* x, const int* n_valid, int batch, int n, int draws, uint32_t clip0,
                         uint32_t draw0, float sigma, uint64_t seed, float clip_lo, float clip_hi, float* out,
                         lipasr_stream_t stream) {
  LP_CHECK_ARG(batch >= 0 && n >= 0 && draws >= 0, "lipasr_smooth_expand: bad shape %d x %d x %d", batch, draws, n);
  LP_CHECK_ARG(sigma >= 0.0f && sigma < INFINITY, "lipasr_smooth_expand: sigma %g", (double)sigma);
  LP_CHECK_ARG(clip_lo <= clip_hi, "lipasr_smooth_expand: clip range [%g, %g]", (double)clip_lo, (double)clip_hi);
  LP_CHECK_ARG(h != nullptr, "lipasr_smooth_expand: null handle");
  if (batch == 0 || draws == 0 || n == 0) return LIPASR_OK;
  LP_CHECK_ARG(x != nullptr && out != nullptr, "lipasr_smooth_expand: x or out is null");
  LP_CHECK_ARG((long long)batch * draws <= 0x7fffffffLL, "lipasr_smooth_expand: %d x %d rows in one call", batch, draws);
  hipLaunchKernelGGL(smooth_expand_kernel, dim3((unsigned)(batch * draws)), dim3(kSmThreads), 0, S(stream), x, n_valid, n, draws,
                     clip0, draw0, sigma, seed, clip_lo, clip_hi, out);
  LP_LAUNCH_CHECK();
  ++g_smooth_launches[1];
  return LIPASR_OK;
}

int lipasr_smooth_vote(lipasr_handle_t h, const float* logits, int batch, int draws, int classes, int* counts,
                       lipasr_stream_t stream) {
  LP_CHECK_ARG(classes >= 1 && classes <= kSmMaxC, "lipasr_smooth_vote: %d classes; 1 to %d are supported", classes, kSmMaxC);
  LP_CHECK_ARG(batch >= 0 && draws >= 0, "lipasr_smooth_vote: bad shape %d x %d", batch, draws);
  LP_CHECK_ARG(h != nullptr, "lipasr_smooth_vote: null handle");
  if (batch == 0 || draws == 0) return LIPASR_OK;
  LP_CHECK_ARG(logits != nullptr && counts != nullptr, "lipasr_smooth_vote: logits or counts is null");
  hipLaunchKernelGGL(smooth_vote_kernel, dim3((unsigned)batch), dim3(kSmThreads), 0, S(stream), logits, draws, classes, counts);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_smooth_noise_host(uint64_t seed, uint32_t clip, uint32_t draw, int n, float* z_out) {
  LP_CHECK_ARG(n >= 0, "lipasr_smooth_noise_host: n %d", n);
  LP_CHECK_ARG(n == 0 || z_out != nullptr, "lipasr_smooth_noise_host: z_out is null");
  for (int q = 0; q * 4 < n; ++q) {
    float z[4];
    normal4(seed, (uint64_t)q, clip, draw, z);
    for (int e = 0; e < 4 && q * 4 + e < n; ++e) z_out[q * 4 + e] = z[e];
  }
  return LIPASR_OK;
}

}  // extern "C"
