// K3 host side: what the units of the Lipschitz projections share -- the limits, the kernel arguments that cross a unit, the launch
// counters, the ONE map of the handle's scratch, and the launchers (spectral_chain.hip, spectral_sigma.hip, spectral_pi.hip,
// spectral_clip.hip).  spectral.hip holds the C entry points: they check arguments and call these.
#pragma once
#include "common.h"

namespace lipasr {

constexpr double kEps = 2.220446049250313e-16;  // np.spacing(1), Constraints.py:25,167
constexpr int kMaxR = 32;
constexpr int kMaxOrder = 64;
#ifndef LIPASR_SQUARINGS
#define LIPASR_SQUARINGS 40
#endif
constexpr int kSquarings = LIPASR_SQUARINGS;
static_assert(kSquarings <= 64, "sigma_scale_layers_kernel gives the logarithm of squaring j to lane j of one wavefront");

struct OrderArgs {
  int n_layers;
  int n_order;
  int order[kMaxOrder];
};

struct LayerPtrs {
  int n_layers;
  float* W[LIPASR_MAX_LAYERS];
  int rows[LIPASR_MAX_LAYERS];
  int cols[LIPASR_MAX_LAYERS];
  int wg_start[LIPASR_MAX_LAYERS + 1];  // sigma_scale_layers_kernel only: workgroups wg_start[l] .. wg_start[l + 1] - 1 scale layer l
};
inline void fill_layer_ptrs(LayerPtrs* lp, float* const* Ws, const int* rows, const int* cols, int n_layers) {
  lp->n_layers = n_layers;
  for (int l = 0; l < n_layers; ++l) { lp->W[l] = Ws[l]; lp->rows[l] = rows[l]; lp->cols[l] = cols[l]; }
}

// Test hook (lipasr_debug_k3_launches): launches since load per K3 kernel, counted on the host where the launch happens.
enum K3Kernel { K3_CHAIN_STEP_12 = 0, K3_CHAIN_STEP_20, K3_CHAIN_STEP_32, K3_CHAIN_HEAD, K3_PRODUCT_SIGMA, K3_SCALE_LAYERS, K3_SIGMA_SCALE_LAYERS,
                K3_PI_U, K3_PI_V, K3_PI_FINISH, K3_SV_CLIP, K3_FROBENIUS, K3_BN_CORRECTION, K3_KERNELS };
extern __attribute__((visibility("hidden"))) long g_k3_launches[K3_KERNELS];  // spectral.hip
inline void k3_count(K3Kernel k) { ++g_k3_launches[k]; }

// ---------------------------------------------------------------------------------------------
// The handle's scratch (h->scratch, h->scratch_floats floats) as K3 uses it:
//   [0, 32)    scale factor per layer          (product_sigma_kernel / sigma_scale_layers_kernel -> scale_layers_kernel)
//   [32, 64)   sigma of the product
//   [64, ...)  the work area, one use at a time on a stream: the chain's two ping-pong P buffers and the fp64 Gram partials
//              behind them | the power iteration's left vectors | the Frobenius pair's fp64 partial sums
// One function per use carves the work area and checks its capacity (message set, null / LIPASR_EUNSUPPORTED when it is short).
// ---------------------------------------------------------------------------------------------
struct K3Scratch {
  static constexpr size_t kScales = 0, kSigma = 32, kWork = 64;
  static constexpr size_t kChainGramMin = 1024;  // floats the chain leaves for Gram partials at the least
  float* scales;
  float* sigma;
  float* work;
  size_t work_floats;
  explicit K3Scratch(const lipasr_ctx* h)
      : scales(h->scratch + kScales), sigma(h->scratch + kSigma), work(h->scratch + kWork),
        work_floats(h->scratch_floats > kWork ? h->scratch_floats - kWork : 0) {}
};

struct ChainScratch {
  float* scales;
  float* sigma;
  float* P[2];
  double* gram;
  size_t gram_cap_doubles;
};
inline int carve_chain_scratch(const lipasr_ctx* h, int R, int max_width, ChainScratch* cs) {
  const K3Scratch k(h);
  const size_t pbuf = ((size_t)R * max_width + 63) & ~size_t(63);
  if (2 * pbuf + K3Scratch::kChainGramMin > k.work_floats) {
    set_error("product chain: %d classes x width %d exceeds the handle's scratch", R, max_width);
    return LIPASR_EUNSUPPORTED;
  }
  cs->scales = k.scales;
  cs->sigma = k.sigma;
  cs->P[0] = k.work;
  cs->P[1] = k.work + pbuf;
  cs->gram = reinterpret_cast<double*>(k.work + 2 * pbuf);
  cs->gram_cap_doubles = (k.work_floats - 2 * pbuf) / 2;
  return LIPASR_OK;
}
// the power iteration's left vectors, `floats` in all
inline float* carve_pi_left(const lipasr_ctx* h, size_t floats) {
  const K3Scratch k(h);
  if (floats > k.work_floats) {
    set_error("power iteration: left vectors exceed scratch");
    return nullptr;
  }
  return k.work;
}
// one fp64 partial sum per workgroup of sumsq_clamped_kernel
inline double* carve_frobenius_partials(const lipasr_ctx* h, int n_part) {
  const K3Scratch k(h);
  if (2 * (size_t)n_part > k.work_floats) {
    set_error("Frobenius projection: %d partial sums exceed scratch", n_part);
    return nullptr;
  }
  return reinterpret_cast<double*>(k.work);
}

// spectral.hip: lipasr_project_product with an optional device counter bumped by its single-workgroup kernel (optim.hip: the fused
// Adam + projection step)
int project_product_bump(lipasr_handle_t h, float* const* Ws, const int* rows, const int* cols, int n_layers, float rho,
                         const int* order, int n_order, float* norms_out, int* bump, lipasr_stream_t stream);

// What the K3 units share among themselves (g_k3_launches above too) stays out of the library's exported symbols.
#pragma GCC visibility push(hidden)
// spectral.hip
int check_layers(const char* fn, const float* const* Ws, const int* rows, const int* cols, int n_layers, bool need_chain);

// spectral_chain.hip.  Launches the chain; on return the Gram partials are in cs.gram (n_part blocks).
// want_gram = false: the caller takes the finished product itself (*p_final, R x rows[0]) and the last step emits nothing else.
int launch_chain(lipasr_ctx* h, const float* const* Ws, const int* rows, const int* cols, int m, ChainScratch* cs, int* n_part_out,
                 hipStream_t st, bool want_gram = true, const float** p_final = nullptr);

// spectral_sigma.hip.  sigma_fused_fits: the ONE rule for the update step's path -- chain without Gram partials, then
// launch_sigma_scale_layers (true), or chain with them, launch_product_sigma and, when n_order > 0, launch_scale_layers (false).
bool sigma_fused_fits(int R, int n0, int n_order);
int launch_sigma_scale_layers(const float* P, int n0, int R, double rho, const OrderArgs& oa, LayerPtrs lp, float* scales,
                              float* norms_out, float* sigma_out, int* bump, hipStream_t st);
int launch_product_sigma(const double* gram_part, int n_part, int R, double rho, const OrderArgs& oa, float* scales, float* norms_out,
                         float* sigma_out, int* bump, hipStream_t st);
int launch_scale_layers(const LayerPtrs& lp, const float* scales, hipStream_t st);

// spectral_pi.hip: `iters` rounds of the batched power iteration (warm: from v_state, else from the fixed start vector), then
// sigmas_out[l] = ||W_l v_l||; do_scale: also W_l <- max(W_l, 0) * c / (sigma_l + eps)
int launch_power_iteration(lipasr_ctx* h, const float* const* Ws, const int* rows, const int* cols, int n_layers, float* v_state,
                           int clamp, int warm, int iters, double c, int do_scale, float* sigmas_out, hipStream_t st);

// spectral_clip.hip
int launch_sv_clip(const float* X, int R, int n, double hi, float* out, float* svals_out, hipStream_t st);
int launch_frobenius(lipasr_ctx* h, float* W, size_t n, double rho, hipStream_t st);
int launch_bn_correction(const float* gamma, const float* var, int n, float* out, hipStream_t st);
#pragma GCC visibility pop

}  // namespace lipasr
