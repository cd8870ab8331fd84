// The row contract of the attack kernels (apgd, hsj, genetic, square, smoothing, room, deepfool, lp_attack, jacobian, universal, bounds), stated once.
//
// A row of n floats is owned quad by quad: quad q is the elements 4q .. 4q + 3, whichever thread takes it.  A quad moves as one
// float4 where it is whole and its base sits on 16 bytes (the caller says so: `whole`), as four guarded scalars otherwise; the
// element-to-thread map is the same in both, so the alignment never changes a value.  n_valid[b] is clamped to [0, n]; the padding
// keeps the bits of x0.  clip_lo / clip_hi are applied as v < lo ? lo : (v > hi ? hi : v), so that a NaN stays.  A sum over a row is a
// butterfly per wavefront, one double per wavefront in LDS, then index order.  No written span overlaps any other.
//
// Nothing here holds an a * b + c: hsj.hip turns contraction off only after its includes, and its host and device twins must round
// alike, so whatever multiplies and adds stays in the file that owns it.
// The margin / "is adversarial" functions (square_margin, hsj_adv, the fitness of genetic_select_kernel, apgd_loss_kernel, the
// head of deepfool_step_kernel, smooth_vote_kernel) are deliberately NOT shared: they differ in what a NaN gives (NaN, -inf, false,
// bin C), in what one class gives and in whether the difference is fp32 or fp64, each pinned by its own tests and its paragraph
// of include/lipasr.h.
#pragma once
#include "common.h"

namespace lipasr {

// the valid length of row b: n without lengths, else n_valid[b] clamped to [0, n]
__host__ __device__ __forceinline__ int row_valid(const int* n_valid, int b, int n) {
  return n_valid ? std::min(std::max(n_valid[b], 0), n) : n;
}

__host__ __device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
__host__ __device__ __forceinline__ double clampf(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// quad k0 / 4 of a row of n floats at p; whole: the quad has four elements and p + k0 sits on 16 bytes.  A load pads with 0.
__device__ __forceinline__ void ld4(const float* __restrict__ p, int k0, int n, bool whole, float (&v)[4]) {
  if (whole) {
    const float4 t = *reinterpret_cast<const float4*>(p + k0);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (k0 + e < n) ? p[k0 + e] : 0.0f;
  }
}
__device__ __forceinline__ void st4(float* __restrict__ p, int k0, int n, bool whole, const float (&v)[4]) {
  if (whole) {
    *reinterpret_cast<float4*>(p + k0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (k0 + e < n) p[k0 + e] = v[e];
  }
}

// vector i of a row whose width and base the caller has found to be multiples of VEC floats (VEC = 4 or 1)
template <int VEC>
__device__ __forceinline__ void ldv(const float* __restrict__ p, size_t i, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 t = reinterpret_cast<const float4*>(p)[i];
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = p[i];
  }
}
template <int VEC>
__device__ __forceinline__ void stv(float* __restrict__ p, size_t i, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    reinterpret_cast<float4*>(p)[i] = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    p[i] = v[0];
  }
}

// the sum of v over the T threads of a row, the same bits in every thread: xor butterfly per wavefront, then (T > 64) one double
// per wavefront in LDS, added by every thread in index order.  Two barriers: the LDS slots may be used again at once.
template <int T>
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  if constexpr (T > 64) {
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = 0.0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) v += red[w];
    __syncthreads();
  }
  return v;
}

// do [a, a + bytes_a) and [b, b + bytes_b) share a byte?  An empty span overlaps nothing.
inline bool spans_overlap(const void* a, size_t bytes_a, const void* b, size_t bytes_b) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
  return bytes_a != 0 && bytes_b != 0 && !(p + bytes_a <= q || q + bytes_b <= p);
}

}  // namespace lipasr
