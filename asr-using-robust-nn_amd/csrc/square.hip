// Square Attack (Andriushchenko, Croce, Flammarion, Hein 2020), the L-inf random search that queries scores only: the two kernels
// around the classifier, and their host restatements.  (include/lipasr.h, lipasr_square_init / lipasr_square_step, fixes the
// conventions.)
//
// A row is height x width, element (r, c) at r * width + c; every perturbed element is clamp(x0 + s eps), s = +-1, so a point of the
// search is a sign pattern.  x_best holds the best pattern found, x_cand the pattern the classifier is asked about next: x_best with
// one window overwritten by one sign.  win[b] = (r, c, h, w) names that window, so a step knows what to keep or to take back.
//
// square_init_kernel: ONE workgroup of 256 threads per row.  A lane takes the columns c = tid, tid + 256, ...: one bit of the Philox
//   block of column block c >> 7 is the sign of the whole column (the paper's vertical stripes), written to x_best and x_cand.
//
// square_step_kernel: ONE workgroup of 256 threads per row, one launch per query, no workspace, no atomics.
//   1. the margin of the row's logits (every thread computes it from the <= 32 logits: no exchange), the row's loss_best, done and
//      win into registers; a barrier, so that no wave reads what thread 0 then writes;
//   2. the window of proposal `it` is copied x_cand -> x_best (accepted) or x_best -> x_cand (rejected): O(window) bytes;
//   3. a barrier (the next window may overlap this one, and another thread may own the shared element), then proposal it + 1 from
//      one Philox block: corner, sign; the window is written into x_cand from x0 alone.
//   Everything is integer arithmetic, one fp32 add, two clamps and one fp32 subtract, in functions the host twins share: the same
//   bits on both sides.  The row's other n - h w elements are never touched, whatever the alignment.
#include "common.h"
#include "row.h"

namespace lipasr {

constexpr int kSqThreads = 256;
constexpr int kSqMaxC = 32;

// min(max(fl(x + s eps), lo), hi); se = +-eps.  A NaN compares false twice and stays.
__host__ __device__ __forceinline__ float square_value(float x, float se, float lo, float hi) {
  return clampf(x + se, lo, hi);
}

// the sign bit of column c at the stripe start: 1 = minus
__host__ __device__ __forceinline__ uint32_t square_stripe_bit(const uint32_t (&o)[4], int c) { return (o[(c >> 5) & 3] >> (c & 31)) & 1u; }

__host__ __device__ __forceinline__ void square_stripe_block(uint64_t seed, int c, uint32_t clip, uint32_t restart, uint32_t (&o)[4]) {
  Philox::gen(seed, (uint64_t)(c >> 7) | (1ull << 62), clip, restart << 24, o);
}

// z_y - max_{c != y} z_c in fp32 (targeted: its negative).  One class: +inf.  A NaN anywhere in the row: NaN.  A label outside
// [0, classes): +inf -- such a row never improves and is never done.
__host__ __device__ __forceinline__ float square_margin(const float* __restrict__ z, int classes, int y, int targeted) {
  if (classes == 1 || y < 0 || y >= classes) return INFINITY;
  const float zy = z[y];
  float other = -INFINITY;
  bool nan = zy != zy;
  for (int c = 0; c < classes; ++c) {
    const float v = z[c];
    nan |= v != v;
    if (c != y && v > other) other = v;
  }
  if (nan) return NAN;
  const float m = zy - other;
  return targeted ? -m : m;
}

// proposal it1 = it + 1 of clip `clip`: the window (r, c, h, w) and the sign bit (1 = minus).  nv < 0: no n_valid.
__host__ __device__ __forceinline__ uint32_t square_draw(uint64_t seed, uint32_t clip, uint32_t restart, uint32_t it1, int height,
                                                          int width, int nv, int win_h, int win_w, uint32_t p_q, int (&w)[4]) {
  uint32_t o[4];
  Philox::gen(seed, 0ull, clip, (restart << 24) | it1, o);
  int h = win_h, ww = win_w, rows = height, cols = width;
  if (nv >= 0) {  // a strip: the segment is a share of the clip's own samples
    const int64_t s = ((int64_t)nv * (int64_t)p_q + (1ll << 23)) >> 24;
    h = 1;
    ww = (int)(s < 1 ? 1 : (s > nv ? nv : s));
    rows = 1;
    cols = nv;
  }
  w[0] = (int)(((uint64_t)o[0] * (uint64_t)(rows - h + 1)) >> 32);
  w[1] = (int)(((uint64_t)o[1] * (uint64_t)(cols - ww + 1)) >> 32);
  w[2] = h;
  w[3] = ww;
  return o[2] & 1u;
}

// what one step decides for a row, from what it found: shared by the kernel and the host twin
struct SquareRow {
  bool accept, revert, propose;
  float loss_best;
  int done;
};

__host__ __device__ __forceinline__ SquareRow square_decide(float loss, float loss_best, int done, uint32_t it, int nv, int flags) {
  SquareRow r;
  r.accept = r.revert = false;
  r.loss_best = loss_best;
  r.done = done;
  if (it == 0) {
    r.loss_best = loss != loss ? INFINITY : loss;
  } else if (done == 0 && loss < loss_best) {
    r.accept = true;
    r.loss_best = loss;
  } else {
    r.revert = true;
  }
  if (done == 0 && r.loss_best < 0.0f) r.done = (int)it + 1;
  r.propose = r.done == 0 && nv != 0 && !(flags & LIPASR_SQUARE_LAST);
  return r;
}

__global__ __launch_bounds__(kSqThreads) void square_init_kernel(const float* __restrict__ x0, const int* __restrict__ n_valid,
                                                                  int height, int width, uint32_t clip0, uint32_t restart,
                                                                  uint64_t seed, float eps, float lo, float hi,
                                                                  float* __restrict__ x_best, float* __restrict__ x_cand,
                                                                  int* __restrict__ win) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)b * height * width;
  const int nv = row_valid(n_valid, b, width);  // n_valid comes with height == 1 only
  if (tid < 4) win[(size_t)b * 4 + tid] = 0;
  for (int c = tid; c < width; c += kSqThreads) {
    uint32_t o[4];
    square_stripe_block(seed, c, clip0 + (uint32_t)b, restart, o);
    const float se = square_stripe_bit(o, c) ? -eps : eps;
    for (int r = 0; r < height; ++r) {
      const size_t k = base + (size_t)r * width + c;
      const float x = x0[k];
      const float v = c < nv ? square_value(x, se, lo, hi) : x;
      x_best[k] = v;
      x_cand[k] = v;
    }
  }
}

__global__ __launch_bounds__(kSqThreads) void square_step_kernel(const float* __restrict__ logits, const int* __restrict__ labels,
                                                                  const float* __restrict__ x0, const int* __restrict__ n_valid,
                                                                  int classes, int height, int width, int win_h, int win_w,
                                                                  uint32_t p_q, int targeted, uint32_t clip0, uint32_t restart,
                                                                  uint32_t it, int flags, uint64_t seed, float eps, float lo,
                                                                  float hi, float* __restrict__ x_best, float* __restrict__ x_cand,
                                                                  float* __restrict__ loss_best, int* __restrict__ done,
                                                                  int* __restrict__ win) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)b * height * width;
  int* __restrict__ wb = win + (size_t)b * 4;
  const int pr = wb[0], pc = wb[1], ph = wb[2], pw = wb[3];
  const int nvr = n_valid ? row_valid(n_valid, b, width) : -1;
  const float loss = square_margin(logits + (size_t)b * classes, classes, labels[b], targeted);
  const SquareRow d = square_decide(loss, loss_best[b], done[b], it, nvr, flags);  // uniform
  __syncthreads();  // every wave has read the row's state
  if (tid == 0) {
    loss_best[b] = d.loss_best;
    done[b] = d.done;
  }
  if (d.accept | d.revert) {
    // the window the previous step wrote lies inside the row: (pr, pc, ph, pw) are this kernel's own output, clamped all the same
    const int r0 = min(max(pr, 0), height), c0 = min(max(pc, 0), width);
    const int h = min(max(ph, 0), height - r0), w = min(max(pw, 0), width - c0);
    const float* __restrict__ src = (d.accept ? x_cand : x_best) + base;
    float* __restrict__ dst = (d.accept ? x_best : x_cand) + base;
    const int cells = h * w;
    for (int i = tid; i < cells; i += kSqThreads) {
      const size_t k = (size_t)(r0 + i / w) * width + (c0 + i % w);
      dst[k] = src[k];
    }
  }
  int nw[4] = {0, 0, 0, 0};
  if (d.propose) {
    __syncthreads();  // the new window may overlap the old one: its copies are in before it is overwritten
    const uint32_t minus = square_draw(seed, clip0 + (uint32_t)b, restart, it + 1u, height, width, nvr, win_h, win_w, p_q, nw);
    const float se = minus ? -eps : eps;
    const int w = nw[3], cells = nw[2] * w;
    for (int i = tid; i < cells; i += kSqThreads) {
      const size_t k = base + (size_t)(nw[0] + i / w) * width + (nw[1] + i % w);
      x_cand[k] = square_value(x0[k], se, lo, hi);
    }
  }
  if (tid < 4) wb[tid] = nw[tid];
}

// the checks the device entry points and their host twins share
static int square_check(const char* fn, const int* n_valid, int B, int height, int width, uint32_t restart, float eps, float lo,
                        float hi) {
  LP_CHECK_ARG(B >= 0 && height >= 0 && width >= 0, "%s: bad shape %d x %d x %d", fn, B, height, width);
  LP_CHECK_ARG((long long)height * width <= 0x7fffffffLL, "%s: rows of %d x %d elements", fn, height, width);
  LP_CHECK_ARG(n_valid == nullptr || height <= 1, "%s: n_valid with height %d; lengths go with a 1 x n strip", fn, height);
  LP_CHECK_ARG(restart < 256u, "%s: restart %u; below 256 is required", fn, restart);
  LP_CHECK_ARG(eps >= 0.0f && eps < INFINITY, "%s: eps %g", fn, (double)eps);
  LP_CHECK_ARG(lo <= hi, "%s: clip range [%g, %g]", fn, (double)lo, (double)hi);
  return LIPASR_OK;
}

static int square_step_check(const char* fn, const int* n_valid, int B, int classes, int height, int width, int win_h, int win_w,
                             uint32_t p_q, uint32_t restart, uint32_t it, int flags, float eps, float lo, float hi) {
  if (int rc = square_check(fn, n_valid, B, height, width, restart, eps, lo, hi)) return rc;
  LP_CHECK_ARG(it < (1u << 24), "%s: it %u; below 2^24 is required", fn, it);
  LP_CHECK_ARG(classes >= 1 && classes <= kSqMaxC, "%s: %d classes; 1 to %d are supported", fn, classes, kSqMaxC);
  LP_CHECK_ARG(p_q <= (1u << 24), "%s: p_q %u; at most 2^24", fn, p_q);
  LP_CHECK_ARG((flags & ~LIPASR_SQUARE_LAST) == 0, "%s: flags %d", fn, flags);
  LP_CHECK_ARG(height == 0 || width == 0 || (win_h >= 1 && win_h <= height && win_w >= 1 && win_w <= width),
               "%s: window %d x %d in a row of %d x %d", fn, win_h, win_w, height, width);
  return LIPASR_OK;
}

static int square_pointers(const char* fn, const float* x0, const float* x_best, const float* x_cand, const int* win, int B, int n) {
  LP_CHECK_ARG(x0 != nullptr && x_best != nullptr && x_cand != nullptr && win != nullptr, "%s: a null pointer", fn);
  const size_t bytes = (size_t)B * n * sizeof(float);
  LP_CHECK_ARG(!spans_overlap(x_best, bytes, x_cand, bytes), "%s: x_best overlaps x_cand", fn);
  LP_CHECK_ARG(!spans_overlap(x_best, bytes, x0, bytes), "%s: x_best overlaps x0", fn);
  LP_CHECK_ARG(!spans_overlap(x_cand, bytes, x0, bytes), "%s: x_cand overlaps x0", fn);
  return LIPASR_OK;
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

int lipasr_square_init(lipasr_handle_t h, const float* x0, const int* n_valid, int batch, int height, int width, uint32_t clip0,
                       uint32_t restart, uint64_t seed, float eps, float clip_lo, float clip_hi, float* x_best, float* x_cand, int* win,
                       lipasr_stream_t stream) {
  const char* fn = "lipasr_square_init";
  if (int rc = square_check(fn, n_valid, batch, height, width, restart, eps, clip_lo, clip_hi)) return rc;
  LP_CHECK_ARG(h != nullptr, "%s: null handle", fn);
  if (batch == 0 || height == 0 || width == 0) return LIPASR_OK;
  if (int rc = square_pointers(fn, x0, x_best, x_cand, win, batch, height * width)) return rc;
  hipLaunchKernelGGL(square_init_kernel, dim3((unsigned)batch), dim3(kSqThreads), 0, S(stream), x0, n_valid, height, width, clip0,
                     restart, seed, eps, clip_lo, clip_hi, x_best, x_cand, win);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_square_init_host(const float* x0, const int* n_valid, int batch, int height, int width, uint32_t clip0, uint32_t restart,
                            uint64_t seed, float eps, float clip_lo, float clip_hi, float* x_best, float* x_cand, int* win) {
  const char* fn = "lipasr_square_init_host";
  if (int rc = square_check(fn, n_valid, batch, height, width, restart, eps, clip_lo, clip_hi)) return rc;
  if (batch == 0 || height == 0 || width == 0) return LIPASR_OK;
  if (int rc = square_pointers(fn, x0, x_best, x_cand, win, batch, height * width)) return rc;
  for (int b = 0; b < batch; ++b) {
    const size_t base = (size_t)b * height * width;
    const int nv = row_valid(n_valid, b, width);
    for (int e = 0; e < 4; ++e) win[(size_t)b * 4 + e] = 0;
    for (int c = 0; c < width; ++c) {
      uint32_t o[4];
      square_stripe_block(seed, c, clip0 + (uint32_t)b, restart, o);
      const float se = square_stripe_bit(o, c) ? -eps : eps;
      for (int r = 0; r < height; ++r) {
        const size_t k = base + (size_t)r * width + c;
        const float v = c < nv ? square_value(x0[k], se, clip_lo, clip_hi) : x0[k];
        x_best[k] = v;
        x_cand[k] = v;
      }
    }
  }
  return LIPASR_OK;
}

int lipasr_square_step(lipasr_handle_t h, const float* logits, const int* labels, const float* x0, const int* n_valid, int batch,
                       int classes, int height, int width, int win_h, int win_w, uint32_t p_q, int targeted, uint32_t clip0,
                       uint32_t restart, uint32_t it, int flags, uint64_t seed, float eps, float clip_lo, float clip_hi, float* x_best,
                       float* x_cand, float* loss_best, int* done, int* win, lipasr_stream_t stream) {
  const char* fn = "lipasr_square_step";
  if (int rc = square_step_check(fn, n_valid, batch, classes, height, width, win_h, win_w, p_q, restart, it, flags, eps, clip_lo, clip_hi))
    return rc;
  LP_CHECK_ARG(h != nullptr, "%s: null handle", fn);
  if (batch == 0 || height == 0 || width == 0) return LIPASR_OK;
  LP_CHECK_ARG(logits != nullptr && labels != nullptr && loss_best != nullptr && done != nullptr, "%s: a null pointer", fn);
  if (int rc = square_pointers(fn, x0, x_best, x_cand, win, batch, height * width)) return rc;
  hipLaunchKernelGGL(square_step_kernel, dim3((unsigned)batch), dim3(kSqThreads), 0, S(stream), logits, labels, x0, n_valid, classes,
                     height, width, win_h, win_w, p_q, targeted ? 1 : 0, clip0, restart, it, flags, seed, eps, clip_lo, clip_hi, x_best,
                     x_cand, loss_best, done, win);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_square_step_host(const float* logits, const int* labels, const float* x0, const int* n_valid, int batch, int classes,
                            int height, int width, int win_h, int win_w, uint32_t p_q, int targeted, uint32_t clip0, uint32_t restart,
                            uint32_t it, int flags, uint64_t seed, float eps, float clip_lo, float clip_hi, float* x_best, float* x_cand,
                            float* loss_best, int* done, int* win) {
  const char* fn = "lipasr_square_step_host";
  if (int rc = square_step_check(fn, n_valid, batch, classes, height, width, win_h, win_w, p_q, restart, it, flags, eps, clip_lo, clip_hi))
    return rc;
  if (batch == 0 || height == 0 || width == 0) return LIPASR_OK;
  LP_CHECK_ARG(logits != nullptr && labels != nullptr && loss_best != nullptr && done != nullptr, "%s: a null pointer", fn);
  if (int rc = square_pointers(fn, x0, x_best, x_cand, win, batch, height * width)) return rc;
  for (int b = 0; b < batch; ++b) {
    const size_t base = (size_t)b * height * width;
    int* wb = win + (size_t)b * 4;
    const int nvr = n_valid ? row_valid(n_valid, b, width) : -1;
    const float loss = square_margin(logits + (size_t)b * classes, classes, labels[b], targeted ? 1 : 0);
    const SquareRow d = square_decide(loss, loss_best[b], done[b], it, nvr, flags);
    loss_best[b] = d.loss_best;
    done[b] = d.done;
    if (d.accept || d.revert) {
      const int r0 = std::min(std::max(wb[0], 0), height), c0 = std::min(std::max(wb[1], 0), width);
      const int hh = std::min(std::max(wb[2], 0), height - r0), ww = std::min(std::max(wb[3], 0), width - c0);
      const float* src = (d.accept ? x_cand : x_best) + base;
      float* dst = (d.accept ? x_best : x_cand) + base;
      for (int r = r0; r < r0 + hh; ++r)
        for (int c = c0; c < c0 + ww; ++c) dst[(size_t)r * width + c] = src[(size_t)r * width + c];
    }
    int nw[4] = {0, 0, 0, 0};
    if (d.propose) {
      const uint32_t minus = square_draw(seed, clip0 + (uint32_t)b, restart, it + 1u, height, width, nvr, win_h, win_w, p_q, nw);
      const float se = minus ? -eps : eps;
      for (int r = nw[0]; r < nw[0] + nw[2]; ++r)
        for (int c = nw[1]; c < nw[1] + nw[3]; ++c) {
          const size_t k = base + (size_t)r * width + c;
          x_cand[k] = square_value(x0[k], se, clip_lo, clip_hi);
        }
    }
    for (int e = 0; e < 4; ++e) wb[e] = nw[e];
  }
  return LIPASR_OK;
}

}  // extern "C"
