// K3: Lipschitz projections on the device (gfx950).  This unit holds the C entry points: they check their arguments and call the
// launchers of spectral.h; the kernels live in spectral_chain.hip, spectral_sigma.hip, spectral_pi.hip and spectral_clip.hip.
//
//   product variant  (simple_norm_constraint, Constraints.py:135-189; get_lipschitz_constrained,
//                     extract_features_construct_dataset.py:169-196)
//     cst = W_m^T ... W_1^T is R x n_0 with R = number of classes (<= 32).  It is formed by m-1
//     skinny chain steps  P <- P * W_k^T  (each output element is a dot product along a contiguous
//     row of W_k: one wavefront per row, 64-lane DPP/shuffle reduction, W read exactly once), the
//     last step also emits per-workgroup partial Gram matrices P P^T in fp64.  One small kernel
//     sums the partials in a fixed order, takes lambda_max by repeated squaring
//     (lambda_max <= tr(G^(2^J))^(1/2^J) <= R^(1/2^J) lambda_max, J = 40), derives every scale factor
//     of the sequential pass in closed form and writes them to scratch; a last multi-tensor kernel
//     applies them.  No host round trip, bitwise reproducible (no float atomics), so data-parallel
//     replicas stay identical.
//
//   per-layer variant (norm_constraint, Constraints.py:9-33; get_norms,
//                      extract_features_construct_dataset.py:154-161)
//     power iteration on W^T W, all layers batched in each launch, warm-started from the previous
//     step's right singular vector.  u = W v: one wavefront per row; v = W^T u: 32 columns x 8 row
//     lanes per workgroup with an LDS tree, fixed summation order.
#include "spectral.h"

namespace lipasr {

long g_k3_launches[K3_KERNELS] = {};

int check_layers(const char* fn, const float* const* Ws, const int* rows, const int* cols, int n_layers, bool need_chain) {
  LP_CHECK_ARG(Ws && rows && cols, "%s: null layer arrays", fn);
  LP_CHECK_ARG(n_layers >= 1 && n_layers <= LIPASR_MAX_LAYERS, "%s: n_layers=%d outside [1,%d]", fn, n_layers,
               LIPASR_MAX_LAYERS);
  for (int l = 0; l < n_layers; ++l) {
    LP_CHECK_ARG(Ws[l] != nullptr, "%s: kernel %d is null", fn, l);
    LP_CHECK_ARG(rows[l] >= 1 && cols[l] >= 1, "%s: kernel %d has shape %dx%d", fn, l, rows[l], cols[l]);
    if (need_chain && l > 0)
      LP_CHECK_ARG(rows[l] == cols[l - 1], "%s: kernel %d has %d inputs but kernel %d has %d outputs", fn, l, rows[l],
                   l - 1, cols[l - 1]);
  }
  return LIPASR_OK;
}

// bump: optional device int incremented by the (single-workgroup) eigenvalue kernel -- lets the fused
// Adam + projection entry point drop its one-thread step-counter launch
int project_product_bump(lipasr_handle_t h, float* const* Ws, const int* rows, const int* cols, int n_layers, float rho,
                         const int* order, int n_order, float* norms_out, int* bump, lipasr_stream_t stream) {
  LP_CHECK_ARG(h && norms_out, "lipasr_project_product: null argument");
  int rc = check_layers("lipasr_project_product", Ws, rows, cols, n_layers, true);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(n_order >= 0 && n_order <= kMaxOrder, "lipasr_project_product: n_order=%d outside [0,%d]", n_order,
               kMaxOrder);
  LP_CHECK_ARG(n_order == 0 || order != nullptr, "lipasr_project_product: order is null");
  LP_CHECK_ARG(rho > 0.0f, "lipasr_project_product: rho=%g must be positive", (double)rho);
  OrderArgs oa;
  oa.n_layers = n_layers;
  oa.n_order = n_order;
  for (int v = 0; v < n_order; ++v) {
    LP_CHECK_ARG(order[v] >= 0 && order[v] < n_layers, "lipasr_project_product: order[%d]=%d out of range", v, order[v]);
    oa.order[v] = order[v];
  }
  LayerPtrs lp;
  fill_layer_ptrs(&lp, Ws, rows, cols, n_layers);
  ChainScratch cs;
  int n_part = 0;
  const int R = cols[n_layers - 1], n0 = rows[0];
  if (sigma_fused_fits(R, n0, n_order)) {
    const float* p_final = nullptr;
    rc = launch_chain(h, Ws, rows, cols, n_layers, &cs, &n_part, S(stream), false, &p_final);
    if (rc != LIPASR_OK) return rc;
    return launch_sigma_scale_layers(p_final, n0, R, (double)rho, oa, lp, cs.scales, norms_out, cs.sigma, bump, S(stream));
  }
  rc = launch_chain(h, Ws, rows, cols, n_layers, &cs, &n_part, S(stream));
  if (rc != LIPASR_OK) return rc;
  rc = launch_product_sigma(cs.gram, n_part, R, (double)rho, oa, cs.scales, norms_out, cs.sigma, bump, S(stream));
  if (rc != LIPASR_OK || n_order == 0) return rc;
  return launch_scale_layers(lp, cs.scales, S(stream));
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

long lipasr_debug_k3_launches(int kernel) { return (kernel >= 0 && kernel < K3_KERNELS) ? g_k3_launches[kernel] : -1; }

int lipasr_sigma_max(lipasr_handle_t h, const float* W, int rows, int cols, float* v_state, int warm, int iters,
                     int clamp_nonneg, float* sigma_out, lipasr_stream_t stream) {
  LP_CHECK_ARG(h && W && v_state && sigma_out, "lipasr_sigma_max: null argument");
  LP_CHECK_ARG(rows >= 1 && cols >= 1 && iters >= 0, "lipasr_sigma_max: bad shape %dx%d or iters %d", rows, cols, iters);
  return launch_power_iteration(h, &W, &rows, &cols, 1, v_state, clamp_nonneg, warm, iters, 0.0, 0, sigma_out, S(stream));
}

int lipasr_project_per_layer(lipasr_handle_t h, float* const* Ws, const int* rows, const int* cols, int n_layers,
                             float rho, float* v_state, int warm, int iters, float* sigmas_out,
                             lipasr_stream_t stream) {
  LP_CHECK_ARG(h && v_state && sigmas_out, "lipasr_project_per_layer: null argument");
  int rc = check_layers("lipasr_project_per_layer", Ws, rows, cols, n_layers, false);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(iters >= 0, "lipasr_project_per_layer: iters=%d", iters);
  LP_CHECK_ARG(rho > 0.0f, "lipasr_project_per_layer: rho=%g must be positive", (double)rho);
  const double c = pow((double)rho, 1.0 / (double)n_layers);  // np.power(rho, 1/self.m), Constraints.py:25
  return launch_power_iteration(h, Ws, rows, cols, n_layers, v_state, 1, warm, iters, c, 1, sigmas_out, S(stream));
}

int lipasr_project_product(lipasr_handle_t h, float* const* Ws, const int* rows, const int* cols, int n_layers,
                           float rho, const int* order, int n_order, float* norms_out, lipasr_stream_t stream) {
  return project_product_bump(h, Ws, rows, cols, n_layers, rho, order, n_order, norms_out, nullptr, stream);
}

int lipasr_product_norm(lipasr_handle_t h, const float* const* Ws, const int* rows, const int* cols, int n_layers,
                        float* sigma_out, lipasr_stream_t stream) {
  LP_CHECK_ARG(h && sigma_out, "lipasr_product_norm: null argument");
  int rc = check_layers("lipasr_product_norm", Ws, rows, cols, n_layers, true);
  if (rc != LIPASR_OK) return rc;
  ChainScratch cs;
  int n_part = 0;
  rc = launch_chain(h, Ws, rows, cols, n_layers, &cs, &n_part, S(stream));
  if (rc != LIPASR_OK) return rc;
  OrderArgs oa;
  oa.n_layers = n_layers;
  oa.n_order = 0;
  return launch_product_sigma(cs.gram, n_part, cols[n_layers - 1], 1.0, oa, nullptr, nullptr, sigma_out, nullptr, S(stream));
}

int lipasr_frobenius_project(lipasr_handle_t h, float* W, size_t n, float rho, lipasr_stream_t stream) {
  LP_CHECK_ARG(h && W && n > 0, "lipasr_frobenius_project: null or empty kernel");
  return launch_frobenius(h, W, n, (double)rho, S(stream));
}

int lipasr_bn_correction(lipasr_handle_t h, const float* gamma, const float* var, int n, float* out,
                         lipasr_stream_t stream) {
  LP_CHECK_ARG(h && gamma && var && out && n > 0, "lipasr_bn_correction: bad argument");
  return launch_bn_correction(gamma, var, n, out, S(stream));
}

int lipasr_sv_clip(lipasr_handle_t h, const float* X, int R, int n, float hi, float* out, float* svals_out,
                   lipasr_stream_t stream) {
  LP_CHECK_ARG(h && X, "lipasr_sv_clip: null argument");
  LP_CHECK_ARG(out || svals_out, "lipasr_sv_clip: nothing to compute (out and svals_out both null)");
  LP_CHECK_ARG(R >= 1 && R <= kMaxR && n >= 1, "lipasr_sv_clip: needs 1 <= R <= 32 rows and n >= 1 columns");
  LP_CHECK_ARG(hi >= 0.0f, "lipasr_sv_clip: negative clipping level");
  return launch_sv_clip(X, R, n, (double)hi, out, svals_out, S(stream));
}

}  // extern "C"
