// What bounds.hip (the interval and CROWN-IBP bounds), bounds_grad.hip (the backward pass of the interval bounds) and
// bounds_crown_grad.hip (the backward pass of the relaxation) share: the classifier's shape in the flat layout of lipasr_mlp_create,
// the inference-mode BatchNorm affine, the slope of a ReLU line, the workspace alignment, the checks every entry point makes, and
// the two launch sequences that bounds_crown_grad.hip borrows.  bounds_tile.h holds the MFMA tile of the six product kernels.
#pragma once
#include "common.h"
#include "row.h"
#include "mlp.h"

namespace lipasr {

typedef float bd_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBdMaxWidth = 4096;                  // (width + 2) 2^-53 <= kBdD / 2 and gamma_{width + 1} << 1
constexpr int kBdThreads = 256;

constexpr double kBdU = 5.9604644775390625e-08;    // 2^-24, the unit roundoff of fp32
constexpr double kBdTiny = 1.401298464324817e-45;  // 2^-149, the smallest fp32 subnormal
constexpr double kBdD = 9.094947017729282e-13;     // 2^-40: covers every fp64 rounding of a sum of <= 4096 + 2 terms

#define BD_HD __host__ __device__ __forceinline__

BD_HD double bd_max(double a, double b) { return a < b ? b : a; }

// the slope of the line that relaxes relu on [zlo, zhi] for a coefficient p on its output; upper: the line is the upper one of an
// unstable neuron (p < 0), the only one whose slope moves with the box and that has an intercept
BD_HD double bd_slope(double p, float zlo, float zhi, bool& upper) {
  upper = false;
  if (zhi <= 0.0f) return 0.0;
  if (zlo >= 0.0f) return 1.0;
  if (p < 0.0) {
    // any slope >= hi / (hi - lo) lies above relu on [lo, hi]
    upper = true;
    return (double)zhi / ((double)zhi - (double)zlo) * (1.0 + kBdD);
  }
  return zhi >= -zlo ? 1.0 : 0.0;
}

// h = s relu(z) + t in inference mode; tm bounds the magnitudes t was made of
struct BdAff { double s, t, tm; };
// the BatchNorm of one layer: four nulls where the layer has none
struct BdBn { const float *gamma, *beta, *mmean, *mvar; };
BD_HD BdAff bd_aff(const BdBn& bn, int j) {
  if (!bn.gamma) return BdAff{1.0, 0.0, 0.0};
  const double s = (double)bn.gamma[j] / sqrt((double)bn.mvar[j] + (double)kBnEps);
  const double sm = s * (double)bn.mmean[j];
  return BdAff{s, (double)bn.beta[j] - sm, fabs((double)bn.beta[j]) + fabs(sm)};
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

inline BdBn bd_bn(const BdShape& sh, const float* params, const float* bnstate, int l) {
  if (!sh.bn[l]) return BdBn{nullptr, nullptr, nullptr, nullptr};
  return BdBn{params + sh.offg[l], params + sh.offbe[l], bnstate + sh.offmm[l], bnstate + sh.offmv[l]};
}

inline size_t bd_align4(size_t v) { return (v + 3) & ~(size_t)3; }
inline float* bd_base(float* ws) { return reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(ws) + 15) & ~(uintptr_t)15); }

// the shape from widths and BatchNorm flags (the host twins) / from a classifier plan; both refuse what the kernels do not take
int bd_shape_from(const char* fn, int n_layers, const int* widths, const int* bn, BdShape* sh);
int bd_shape_of(const char* fn, lipasr_mlp_t m, BdShape* sh);

// batch >= 1 and batch x classes <= 2^24 / no written span (an output, the workspace) overlaps another one; null spans are skipped
struct BdSpan { const void* p; size_t bytes; bool written; };
int bd_batch_check(const char* fn, const BdShape& sh, int batch);
int bd_check_spans(const char* fn, const BdSpan* sp, int n);

// every *_workspace entry point: the shape's verdict, the checks, then the total of the family's plan
template <class Plan>
int bd_workspace(const char* fn, int shape_rc, const BdShape& sh, int batch, size_t* floats, Plan plan) {
  if (shape_rc) return shape_rc;
  LP_CHECK_ARG(floats != nullptr, "%s: null argument", fn);
  if (int rc = bd_batch_check(fn, sh, batch)) return rc;
  *floats = plan(sh, batch).total;
  return LIPASR_OK;
}

// bounds.hip: out[m][i] = sum_j A[m][j] W[i][j] on the tile of bounds_back_kernel, without its relaxation epilogue
int bd_launch_product(hipStream_t st, const float* A, const float* W, int M, int K, int N, int C, float* out);

// bounds_grad.hip: the sweep of lipasr_mlp_bounds_grad and of its host twin.  mix = null: exactly that call.  Otherwise the margins
// are (1 - beta) margin + beta margin2, the head's cotangent is weighted by 1 - beta, and inj_lo / inj_hi (laid out as layer_lo /
// layer_hi are; only the z boxes are read) are added to the gradient on every pre-activation box before it goes down.
struct BgMixIn {
  const float* margin2;
  float beta;
  const float* inj_lo;
  const float* inj_hi;
};
size_t bg_workspace_floats(const BdShape& sh, int batch);
int bg_run_device(const BdShape& sh, hipStream_t st, const float* params, const float* bnstate, const float* margin, const float* layer_lo,
                  const float* layer_hi, const int* y, int batch, float* ws, float scale_old, float scale_new, float* grads, float* loss_rows,
                  const BgMixIn* mix);
void bg_run_host(const BdShape& sh, const float* params, const float* bnstate, const float* margin, const float* layer_lo,
                 const float* layer_hi, const int* y, int batch, float* ws, float scale_old, float scale_new, float* grads, float* loss_rows,
                 const BgMixIn* mix);

}  // namespace lipasr
