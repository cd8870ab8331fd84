// The genetic black-box attack (Alzantot, Balaji, Srivastava 2018): the two kernels around the classifier in one generation, and the
// host restatement of the first.  (include/lipasr.h, lipasr_genetic_breed / lipasr_genetic_select, fixes the conventions.)
//
// genetic_breed_kernel: ONE workgroup of 256 threads per OUTPUT row b * P + p, one launch per call, no workspace, no atomics.
//   A lane takes the quads k >> 2 = tid, tid + 256, ... of its row: it loads x0 and the two parents' quads, and genetic_quad --
//   the ONE __host__ __device__ function that holds the arithmetic -- draws one Philox block keyed (seed; quad, clip0 + b,
//   generation * 256 + p) for the crossover and the mutation decisions, a second one (quad | 1 << 63) for the amplitudes only
//   where an element of the quad mutates, and clamps to the eps ball and to the clip range.  A quad that lies wholly in the
//   padding is a copy of x0 without a draw or a parent load; a child with parents (a, -1) is a copy of member a.
//   The counter holds the clip, the generation and the member, never the row's position in the call, so a chunk of any size at
//   any start draws what one big call would.  The quads move as row.h says, `whole` judged per array (x0, either parent, the
//   child): the row starts on 16 bytes and the quad is not the partial last one.
//   16 bytes move per element (two parents, x0, the child) against ten Philox rounds per four elements.  Measured on the
//   MI355X at 1024 rows x 22 050 (profiles/genetic_timing.txt): 75 us with two parents, 4.8 TB/s of those nominal bytes (x0 and
//   the parents are shared between children, so part of the reads are cache hits), and 59 us for the initial population, which
//   reads 5.6 MB and writes the same 90 MB with the same arithmetic.  So the floor is vector-instruction issue, as in
//   smooth_expand_kernel (51 us at that shape), and the parents' reads add a fifth on top.  Nothing here chases either roofline.
//
// genetic_select_kernel: ONE wavefront per clip, lane p owns member p (P <= 64).  Fitness from the member's row of logits in
//   fp64 (the difference of two fp32 numbers is then exact), argmax by a butterfly of (value, index) that prefers the lower index,
//   the softmax weights expf((fit - max) / T), their inclusive sum by a Hillis-Steele scan in fp64 (fixed order: the same bits on
//   every run), and per child two inverse-CDF draws from one Philox block against the sums in LDS.  No global atomics; no other
//   workgroup touches the clip's outputs.
#include "common.h"
#include "row.h"

namespace lipasr {

constexpr int kGaThreads = 256;
constexpr int kGaMaxP = 64;
constexpr int kGaMaxC = 32;

// The four children of quad q.  a, c: the parents' elements, x: the clean row's; nvq: how many of the four lie inside the clip
// (the others get the bits of x).  No libm, one explicit fmaf: host and device produce the same bits.
__host__ __device__ __forceinline__ void genetic_quad(uint64_t seed, uint64_t q, uint32_t clip, uint32_t key, uint32_t thresh,
                                                      float step, float eps, float lo, float hi, int nvq, const float (&a)[4],
                                                      const float (&c)[4], const float (&x)[4], float (&out)[4]) {
  uint32_t o[4], m[4] = {0u, 0u, 0u, 0u};
  Philox::gen(seed, q, clip, key, o);
  const bool any = ((o[0] >> 8) < thresh) | ((o[1] >> 8) < thresh) | ((o[2] >> 8) < thresh) | ((o[3] >> 8) < thresh);
  if (any) Philox::gen(seed, q | (1ull << 63), clip, key, m);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float t = (o[e] & 1u) ? c[e] : a[e];
    if ((o[e] >> 8) < thresh) {
      const float v = 2.0f * Philox::u01(m[e]) - 1.0f;  // exact: (k - 2^23) / 2^23, k = 1 .. 2^24
      t = fmaf(step, v, t);
    }
    const float l = x[e] - eps, h = x[e] + eps;
    t = clampf(clampf(t, l, h), lo, hi);
    out[e] = e < nvq ? t : x[e];
  }
}

__host__ __device__ __forceinline__ int genetic_index(int i, int P) { return i < 0 ? 0 : (i >= P ? P - 1 : i); }

__global__ __launch_bounds__(kGaThreads) void genetic_breed_kernel(const float* __restrict__ x0, const int* __restrict__ n_valid,
                                                                    const float* __restrict__ pop_in, const int* __restrict__ parents,
                                                                    int P, int n, uint32_t clip0, uint32_t gen256, uint64_t seed,
                                                                    uint32_t thresh, float step, float eps, float lo, float hi,
                                                                    float* __restrict__ pop_out) {
  const size_t row = blockIdx.x;
  const int b = (int)(row / (size_t)P), p = (int)(row % (size_t)P);
  const int tid = threadIdx.x;
  const float* __restrict__ xr = x0 + (size_t)b * n;
  float* __restrict__ orow = pop_out + row * (size_t)n;
  const float* __restrict__ ar = xr;
  const float* __restrict__ cr = xr;
  bool copy = false;
  if (pop_in) {  // uniform
    const int ia = parents[row * 2], ic = parents[row * 2 + 1];
    ar = pop_in + ((size_t)b * P + genetic_index(ia, P)) * (size_t)n;
    copy = ic < 0;
    cr = copy ? ar : pop_in + ((size_t)b * P + genetic_index(ic, P)) * (size_t)n;
  }
  const int nv = row_valid(n_valid, b, n);
  const bool xvec = (reinterpret_cast<uintptr_t>(xr) & 15) == 0, avec = (reinterpret_cast<uintptr_t>(ar) & 15) == 0,
             cvec = (reinterpret_cast<uintptr_t>(cr) & 15) == 0, ovec = (reinterpret_cast<uintptr_t>(orow) & 15) == 0;
  const bool same = ar == cr;
  const uint32_t clip = clip0 + (uint32_t)b, key = gen256 + (uint32_t)p;
  const int quads = (n + 3) >> 2;
  for (int q = tid; q < quads; q += kGaThreads) {
    const int k0 = q * 4;
    const bool full = k0 + 4 <= n;
    float x[4], v[4];
    ld4(xr, k0, n, xvec && full, x);
    if (k0 >= nv) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = x[e];
    } else {
      const int nvq = min(nv - k0, 4);
      float a[4];
      ld4(ar, k0, n, avec && full, a);
      if (copy) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = e < nvq ? a[e] : x[e];
      } else if (same) {
        genetic_quad(seed, (uint64_t)q, clip, key, thresh, step, eps, lo, hi, nvq, a, a, x, v);
      } else {
        float c[4];
        ld4(cr, k0, n, cvec && full, c);
        genetic_quad(seed, (uint64_t)q, clip, key, thresh, step, eps, lo, hi, nvq, a, c, x, v);
      }
    }
    st4(orow, k0, n, ovec && full, v);
  }
}

__global__ __launch_bounds__(64) void genetic_select_kernel(const float* __restrict__ logits, const int* __restrict__ labels, int P,
                                                             int C, int targeted, float temperature, uint32_t clip0,
                                                             uint32_t generation, uint64_t seed, float* __restrict__ fitness,
                                                             int* __restrict__ best, int* __restrict__ done,
                                                             int* __restrict__ parents) {
  __shared__ double cum[64];
  const size_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const int y = labels[b];
  double fd = -INFINITY;
  if (lane < P && y >= 0 && y < C) {
    const float* __restrict__ r = logits + (b * (size_t)P + lane) * (size_t)C;
    const float zy = r[y];
    bool nan = zy != zy;
    float other = -INFINITY;
    for (int c = 0; c < C; ++c) {
      const float v = r[c];
      nan |= v != v;
      if (c != y && v > other) other = v;
    }
    fd = targeted ? (double)zy - (double)other : (double)other - (double)zy;
    if (nan || fd != fd) fd = -INFINITY;
  }
  if (lane < P) fitness[b * (size_t)P + lane] = (float)fd;
  // argmax, the lowest index on a tie; lanes >= P hold -inf at an index above every member's
  double bv = fd;
  int bi = lane;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  bool frozen = done[b] != 0;  // uniform
  if (!frozen) {
    frozen = bv > 0.0;
    if (lane == 0) {
      best[b] = bi;
      if (frozen) done[b] = (int)generation + 1;
    }
  }
  int* __restrict__ pr = parents + (b * (size_t)P + lane) * 2;
  if (frozen || !(bv > -INFINITY)) {
    if (lane < P) { pr[0] = lane; pr[1] = -1; }
    return;
  }
  // here the largest fitness is finite
  float w = 0.0f;
  if (lane < P && fd > -INFINITY) w = expf((float)((fd - bv) / (double)temperature));
  double s = (double)w;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(s, o, 64);
    if (lane >= o) s += t;
  }
  cum[lane] = s;
  __syncthreads();
  const double total = cum[63];
  if (lane >= P) return;
  if (lane == 0) { pr[0] = bi; pr[1] = -1; return; }
  uint32_t o[4];
  Philox::gen(seed, (uint64_t)lane | (1ull << 62), clip0 + (uint32_t)b, generation * 256u, o);
  const double ta = (double)Philox::u01(o[0]) * total, tc = (double)Philox::u01(o[1]) * total;
  int ia = 0, ic = 0;
  for (int k = 0; k < P; ++k) {
    const double ck = cum[k];
    ia += ck < ta;
    ic += ck < tc;
  }
  pr[0] = min(ia, P - 1);
  pr[1] = min(ic, P - 1);
}

// the checks lipasr_genetic_breed and lipasr_genetic_breed_host share
static int genetic_breed_check(const char* fn, int B, int P, int n, uint32_t generation, uint32_t thresh, float step, float eps,
                               float lo, float hi) {
  LP_CHECK_ARG(B >= 0 && n >= 0, "%s: bad shape %d x %d x %d", fn, B, P, n);
  LP_CHECK_ARG(P >= 2 && P <= kGaMaxP, "%s: population %d; 2 to %d are supported", fn, P, kGaMaxP);
  LP_CHECK_ARG(generation < (1u << 24), "%s: generation %u; below 2^24 is required", fn, generation);
  LP_CHECK_ARG(thresh <= (1u << 24), "%s: mutate_thresh %u; at most 2^24", fn, thresh);
  LP_CHECK_ARG(step >= 0.0f && step < INFINITY, "%s: step %g", fn, (double)step);
  LP_CHECK_ARG(eps >= 0.0f && eps < INFINITY, "%s: eps %g", fn, (double)eps);
  LP_CHECK_ARG(lo <= hi, "%s: clip range [%g, %g]", fn, (double)lo, (double)hi);
  return LIPASR_OK;
}

static int genetic_breed_pointers(const char* fn, const float* x0, const float* pop_in, const int* parents, int B, int P, int n,
                                  const float* pop_out) {
  LP_CHECK_ARG(x0 != nullptr && pop_out != nullptr, "%s: x0 or pop_out is null", fn);
  LP_CHECK_ARG((pop_in == nullptr) == (parents == nullptr), "%s: pop_in and parents go together (both or neither)", fn);
  LP_CHECK_ARG((long long)B * P <= 0x7fffffffLL, "%s: %d x %d rows in one call", fn, B, P);
  const size_t bytes = (size_t)B * P * n * sizeof(float);
  LP_CHECK_ARG(pop_in == nullptr || !spans_overlap(pop_out, bytes, pop_in, bytes), "%s: pop_out overlaps pop_in", fn);
  LP_CHECK_ARG(!spans_overlap(pop_out, bytes, x0, (size_t)B * n * sizeof(float)), "%s: pop_out overlaps x0", fn);
  return LIPASR_OK;
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

int lipasr_genetic_breed(lipasr_handle_t h, const float* x0, const int* n_valid, const float* pop_in, const int* parents, int batch,
                         int pop, int n, uint32_t clip0, uint32_t generation, uint64_t seed, uint32_t mutate_thresh, float step,
                         float eps, float clip_lo, float clip_hi, float* pop_out, lipasr_stream_t stream) {
  const char* fn = "lipasr_genetic_breed";
  if (int rc = genetic_breed_check(fn, batch, pop, n, generation, mutate_thresh, step, eps, clip_lo, clip_hi)) return rc;
  LP_CHECK_ARG(h != nullptr, "%s: null handle", fn);
  if (batch == 0 || n == 0) return LIPASR_OK;
  if (int rc = genetic_breed_pointers(fn, x0, pop_in, parents, batch, pop, n, pop_out)) return rc;
  hipLaunchKernelGGL(genetic_breed_kernel, dim3((unsigned)(batch * pop)), dim3(kGaThreads), 0, S(stream), x0, n_valid, pop_in,
                     parents, pop, n, clip0, generation * 256u, seed, mutate_thresh, step, eps, clip_lo, clip_hi, pop_out);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_genetic_breed_host(const float* x0, const int* n_valid, const float* pop_in, const int* parents, int batch, int pop,
                              int n, uint32_t clip0, uint32_t generation, uint64_t seed, uint32_t mutate_thresh, float step,
                              float eps, float clip_lo, float clip_hi, float* pop_out) {
  const char* fn = "lipasr_genetic_breed_host";
  if (int rc = genetic_breed_check(fn, batch, pop, n, generation, mutate_thresh, step, eps, clip_lo, clip_hi)) return rc;
  if (batch == 0 || n == 0) return LIPASR_OK;
  if (int rc = genetic_breed_pointers(fn, x0, pop_in, parents, batch, pop, n, pop_out)) return rc;
  for (int b = 0; b < batch; ++b) {
    const float* xr = x0 + (size_t)b * n;
    const int nv = row_valid(n_valid, b, n);
    for (int p = 0; p < pop; ++p) {
      const size_t row = (size_t)b * pop + p;
      float* orow = pop_out + row * (size_t)n;
      const float* ar = xr;
      const float* cr = xr;
      bool copy = false;
      if (pop_in) {
        ar = pop_in + ((size_t)b * pop + genetic_index(parents[row * 2], pop)) * (size_t)n;
        copy = parents[row * 2 + 1] < 0;
        cr = copy ? ar : pop_in + ((size_t)b * pop + genetic_index(parents[row * 2 + 1], pop)) * (size_t)n;
      }
      for (int k0 = 0; k0 < n; k0 += 4) {
        float x[4], a[4], c[4], v[4];
        for (int e = 0; e < 4; ++e) {
          const bool in = k0 + e < n;
          x[e] = in ? xr[k0 + e] : 0.0f;
          a[e] = in ? ar[k0 + e] : 0.0f;
          c[e] = in ? cr[k0 + e] : 0.0f;
        }
        const int nvq = std::min(std::max(nv - k0, 0), 4);
        if (nvq == 0) {
          for (int e = 0; e < 4; ++e) v[e] = x[e];
        } else if (copy) {
          for (int e = 0; e < 4; ++e) v[e] = e < nvq ? a[e] : x[e];
        } else {
          genetic_quad(seed, (uint64_t)(k0 >> 2), clip0 + (uint32_t)b, generation * 256u + (uint32_t)p, mutate_thresh, step, eps,
                       clip_lo, clip_hi, nvq, a, c, x, v);
        }
        for (int e = 0; e < 4 && k0 + e < n; ++e) orow[k0 + e] = v[e];
      }
    }
  }
  return LIPASR_OK;
}

int lipasr_genetic_select(lipasr_handle_t h, const float* logits, const int* labels, int batch, int pop, int classes, int targeted,
                          float temperature, uint32_t clip0, uint32_t generation, uint64_t seed, float* fitness, int* best,
                          int* done, int* parents, lipasr_stream_t stream) {
  const char* fn = "lipasr_genetic_select";
  LP_CHECK_ARG(classes >= 1 && classes <= kGaMaxC, "%s: %d classes; 1 to %d are supported", fn, classes, kGaMaxC);
  LP_CHECK_ARG(pop >= 2 && pop <= kGaMaxP, "%s: population %d; 2 to %d are supported", fn, pop, kGaMaxP);
  LP_CHECK_ARG(batch >= 0, "%s: batch %d", fn, batch);
  LP_CHECK_ARG(temperature > 0.0f && temperature < INFINITY, "%s: temperature %g", fn, (double)temperature);
  LP_CHECK_ARG(generation < (1u << 24), "%s: generation %u; below 2^24 is required", fn, generation);
  LP_CHECK_ARG(h != nullptr, "%s: null handle", fn);
  if (batch == 0) return LIPASR_OK;
  LP_CHECK_ARG(logits != nullptr && labels != nullptr && fitness != nullptr && best != nullptr && done != nullptr && parents != nullptr,
               "%s: a null pointer", fn);
  hipLaunchKernelGGL(genetic_select_kernel, dim3((unsigned)batch), dim3(64), 0, S(stream), logits, labels, pop, classes,
                     targeted ? 1 : 0, temperature, clip0, generation, seed, fitness, best, done, parents);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

}  // extern "C"
