// What bounds.hip (the interval and CROWN-IBP bounds) and bounds_grad.hip (the backward pass of the interval bounds) share: the
// classifier's shape in the flat layout of lipasr_mlp_create, the inference-mode BatchNorm affine, the workspace alignment.
#pragma once
#include "common.h"
#include "row.h"
#include "mlp.h"

namespace lipasr {

typedef float bd_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBdMaxWidth = 4096;                  // (width + 2) 2^-53 <= kBdD / 2 and gamma_{width + 1} << 1
constexpr int kBdThreads = 256;

#define BD_HD __host__ __device__ __forceinline__

// h = s relu(z) + t in inference mode; tm bounds the magnitudes t was made of
struct BdAff { double s, t, tm; };
BD_HD BdAff bd_aff(const float* gamma, const float* beta, const float* mmean, const float* mvar, int j) {
  if (!gamma) return BdAff{1.0, 0.0, 0.0};
  const double s = (double)gamma[j] / sqrt((double)mvar[j] + (double)kBnEps);
  const double sm = s * (double)mmean[j];
  return BdAff{s, (double)beta[j] - sm, fabs((double)beta[j]) + fabs(sm)};
}

struct BdShape {
  int L = 0;
  int n[LIPASR_MAX_LAYERS + 1] = {};
  bool bn[LIPASR_MAX_LAYERS] = {};
  size_t offW[LIPASR_MAX_LAYERS] = {}, offb[LIPASR_MAX_LAYERS] = {}, offg[LIPASR_MAX_LAYERS] = {}, offbe[LIPASR_MAX_LAYERS] = {};
  size_t offmm[LIPASR_MAX_LAYERS] = {}, offmv[LIPASR_MAX_LAYERS] = {};
  size_t n_params = 0, n_state = 0;
};

// the boxes the forward pass keeps, as layer_lo / layer_hi hold them: one span [ input box [B][n_0] | z_1 | h_1 | z_2 | h_2 | ... ]
// of fam floats; z[l] / h[l]: where the pre- and post-activation box [B][n_{l+1}] of hidden layer l starts
struct BdBoxes {
  size_t z[LIPASR_MAX_LAYERS] = {}, h[LIPASR_MAX_LAYERS] = {}, fam = 0;
};
inline BdBoxes bd_boxes(const BdShape& sh, int batch) {
  BdBoxes x;
  const size_t B = batch;
  size_t f = B * sh.n[0];
  for (int l = 0; l + 1 < sh.L; ++l) {
    x.z[l] = f; f += B * sh.n[l + 1];
    x.h[l] = f; f += B * sh.n[l + 1];
  }
  x.fam = f;
  return x;
}

inline size_t bd_align4(size_t v) { return (v + 3) & ~(size_t)3; }
inline float* bd_base(float* ws) { return reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(ws) + 15) & ~(uintptr_t)15); }

// the shape from widths and BatchNorm flags (the host twins) / from a classifier plan; both refuse what the kernels do not take
int bd_shape_from(const char* fn, int n_layers, const int* widths, const int* bn, BdShape* sh);
int bd_shape_of(const char* fn, lipasr_mlp_t m, BdShape* sh);

}  // namespace lipasr
