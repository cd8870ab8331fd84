// The dense classifier in inference mode: the three softmax kernels, the forward and the backward-to-the-input GEMM sequences, and
// the entry points on them -- predict, own labels, input gradient, the FGM / PGD steps, output VJP and the whole Jacobian.  Every
// GEMM goes through the launchers of gemm.hip (gemm.h); the plan is mlp.hip's.
#include "gemm.h"

namespace lipasr {

// One row of softmax_vjp_kernel / softmax_vjp_onehot_kernel: upstream vector at the network output -> dz at the logits.
// on_logits: dz = v;  else out = softmax(z): dz = p * (v - sum_c p_c v_c).  v(c) is the upstream value of class c: the two kernels
// differ in nothing else, so for the vector e_cls they give the same dz, bit for bit.
template <class Upstream>
__device__ __forceinline__ void softmax_vjp_row(const float* __restrict__ z, int b, int C, int on_logits, float* __restrict__ prob,
                                                float* __restrict__ dz, Upstream v) {
  const float* zr = z + (size_t)b * C;
  float mx = zr[0];
  for (int c = 1; c < C; ++c) mx = fmaxf(mx, zr[c]);
  float se = 0.0f;
  for (int c = 0; c < C; ++c) se += expf(zr[c] - mx);
  const float inv = 1.0f / se;
  float dot = 0.0f;
  for (int c = 0; c < C; ++c) dot = fmaf(expf(zr[c] - mx) * inv, v(c), dot);
  for (int c = 0; c < C; ++c) {
    const float pc = expf(zr[c] - mx) * inv;
    if (prob) prob[(size_t)b * C + c] = pc;
    const float vc = v(c);
    dz[(size_t)b * C + c] = on_logits ? vc : pc * (vc - dot);
  }
}

// one thread per row, the upstream vector read from v (class_gradient and the optimisation-based attacks)
__global__ __launch_bounds__(256) void softmax_vjp_kernel(const float* __restrict__ z, const float* __restrict__ v, int B,
                                                           int C, int on_logits, float* __restrict__ prob,
                                                           float* __restrict__ dz) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const float* vr = v + (size_t)b * C;
  softmax_vjp_row(z, b, C, on_logits, prob, dz, [vr](int c) { return vr[c]; });
}

// the one-hot upstream vector e_cls, made in registers instead of read (lipasr_mlp_jacobian: one launch per class, no [B][C]
// vector to upload)
__global__ __launch_bounds__(256) void softmax_vjp_onehot_kernel(const float* __restrict__ z, int cls, int B, int C, int on_logits,
                                                                  float* __restrict__ prob, float* __restrict__ dz) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  softmax_vjp_row(z, b, C, on_logits, prob, dz, [cls](int c) { return c == cls ? 1.0f : 0.0f; });
}

// softmax from logits, one thread per row: prob (optional) and onehot_out = one-hot FIRST argmax z (optional).  (The loss and the
// gradient at the logits are the last GEMM's epilogue, EPI_BIAS_SOFTMAX_CE.)
__global__ __launch_bounds__(256) void softmax_ce_kernel(const float* __restrict__ z, int B, int C, float* __restrict__ prob,
                                                          float* __restrict__ onehot_out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const float* zr = z + (size_t)b * C;
  float mx = zr[0];
  int am = 0;
  for (int c = 1; c < C; ++c)
    if (zr[c] > mx) { mx = zr[c]; am = c; }
  float se = 0.0f;
  for (int c = 0; c < C; ++c) se += expf(zr[c] - mx);
  const float inv = 1.0f / se;
  for (int c = 0; c < C; ++c) {
    const float zs = zr[c] - mx;
    const float pc = expf(zs) * inv;
    if (prob) prob[(size_t)b * C + c] = pc;
    if (onehot_out) onehot_out[(size_t)b * C + c] = (c == am) ? 1.0f : 0.0f;
  }
}

static int launch_softmax_ce(const lipasr_mlp* m, const float* logits, int batch, float* prob, float* onehot_out, hipStream_t st) {
  const int C = m->L[m->n_layers - 1].n_out;
  hipLaunchKernelGGL(softmax_ce_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, logits, batch, C, prob, onehot_out);
  LP_LAUNCH_CHECK();
  ++g_k2_launches[K2_SOFTMAX_CE];
  return LIPASR_OK;
}

// inference-mode forward: fills A_l (post-ReLU, if keep_a) and H_l, logits into logits_out.
// ce_y != nullptr: the last GEMM's epilogue also produces softmax (m->ws + offProb) and (p - y) / batch at m->ws + offDzLast.
static int forward_infer(lipasr_mlp* m, const float* params, const float* bnstate, const float* x, int batch,
                         bool keep_a, float* logits_out, hipStream_t st, const float* ce_y = nullptr) {
  const float* hin = x;
  for (int l = 0; l < m->n_layers; ++l) {
    const MlpLayer& L = m->L[l];
    const bool last = (l == m->n_layers - 1);
    float* outp = last ? logits_out : (m->ws + L.offH);
    const bool fuse = last && ce_y;
    GemmArgs g = gemm_args(hin, L.n_in, params + L.offW, L.n_out, outp, L.n_out, batch, L.n_out, L.n_in,
                           last ? (fuse ? EPI_BIAS_SOFTMAX_CE : EPI_BIAS) : EPI_BIAS_RELU_BN);
    g.bias = params + L.offb;
    if (fuse) {
      g.y = ce_y;
      g.inv_batch = 1.0f / (float)batch;
      g.prob = m->ws + m->offProb;
      g.dz = m->ws + m->offDzLast;
    }
    if (!last) {
      if (L.bn) {
        g.gamma = params + L.offg;
        g.beta = params + L.offbe;
        g.mmean = bnstate + L.offmm;
        g.mvar = bnstate + L.offmv;
      }
      // when H aliases A (no BN, no dropout) the ReLU output lands in H == A directly
      g.aux = (keep_a && L.offH != L.offA) ? (m->ws + L.offA) : nullptr;
    }
    set_arith(g, m, OP_ACT, OP_WEIGHT, 1.0f, false);
    int rc = launch_gemm(0, 1, g, st);
    if (rc != LIPASR_OK) return rc;
    hin = outp;
  }
  return LIPASR_OK;
}

// inference-mode backward to the input from dz at the logits (in m->ws + offDzLast).
// final_mode 0: store dx; 1: fused sign step on x_adv.  ld_dx: floats between the rows of dx (0: the input width, rows packed).
static int backward_infer(lipasr_mlp* m, const float* params, const float* bnstate, int batch, float* dx, float* x_adv,
                          const float* x0, float alpha, float eps, hipStream_t st, float g0 = 1.0f, int ld_dx = 0) {
  const float* gin = m->ws + m->offDzLast;
  float* pp[2] = {m->ws + m->offG0, m->ws + m->offG1};
  int cur = 0;
  for (int l = m->n_layers - 1; l >= 0; --l) {
    const MlpLayer& L = m->L[l];
    // dprev[B][n_in] = gin[B][n_out] * W^T ; W stored [n_in][n_out] -> K (= n_out) contiguous
    if (l > 0) {
      const MlpLayer& P = m->L[l - 1];
      GemmArgs g = gemm_args(gin, L.n_out, params + L.offW, L.n_out, pp[cur], L.n_in, batch, L.n_in, L.n_out,
                             EPI_DZ_INFER);
      if (P.bn) {
        g.gamma = params + P.offg;
        g.mvar = bnstate + P.offmv;
      }
      g.aux = m->ws + P.offA;
      set_arith(g, m, OP_GRAD, OP_WEIGHT, g0, false);
      int rc = launch_gemm(0, 0, g, st);
      if (rc != LIPASR_OK) return rc;
      gin = pp[cur];
      cur ^= 1;
    } else {
      GemmArgs g = gemm_args(gin, L.n_out, params + L.offW, L.n_out, dx, ld_dx ? ld_dx : L.n_in, batch, L.n_in, L.n_out,
                             x_adv ? EPI_SIGNSTEP : EPI_STORE);
      g.x_adv = x_adv;
      g.x0 = x0;
      g.alpha = alpha;
      g.eps = eps;
      set_arith(g, m, OP_GRAD, OP_WEIGHT, g0, false);
      int rc = launch_gemm(0, 0, g, st);
      if (rc != LIPASR_OK) return rc;
    }
  }
  return LIPASR_OK;
}

// forward with the loss gradient (p - y) / batch from the last GEMM's epilogue, then backward to the input
static int attack_common(lipasr_mlp_t m, const float* params, const float* bnstate, const float* x_eval,
                         const float* y_onehot, int batch, float* dx, float* x_adv, const float* x0, float alpha,
                         float eps, hipStream_t st) {
  int rc = forward_infer(m, params, bnstate, x_eval, batch, true, m->ws + m->offLogits, st, y_onehot);
  if (rc != LIPASR_OK) return rc;
  return backward_infer(m, params, bnstate, batch, dx, x_adv, x0, alpha, eps, st, 1.0f / (float)batch);
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

int lipasr_mlp_predict(lipasr_mlp_t m, const float* params, const float* bnstate, const float* x, int batch,
                       float* probs, float* logits, lipasr_stream_t stream) {
  int rc = check_call("lipasr_mlp_predict", m, batch, bnstate);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(params && x && (probs || logits), "lipasr_mlp_predict: null argument");
  float* lg = logits ? logits : (m->ws + m->offLogits);
  rc = forward_infer(m, params, bnstate, x, batch, false, lg, S(stream));
  if (rc != LIPASR_OK || !probs) return rc;
  return launch_softmax_ce(m, lg, batch, probs, nullptr, S(stream));
}

int lipasr_mlp_own_labels(lipasr_mlp_t m, const float* params, const float* bnstate, const float* x, int batch,
                          float* y_onehot_out, lipasr_stream_t stream) {
  int rc = check_call("lipasr_mlp_own_labels", m, batch, bnstate);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(params && x && y_onehot_out, "lipasr_mlp_own_labels: null argument");
  float* lg = m->ws + m->offLogits;
  rc = forward_infer(m, params, bnstate, x, batch, false, lg, S(stream));
  if (rc != LIPASR_OK) return rc;
  return launch_softmax_ce(m, lg, batch, nullptr, y_onehot_out, S(stream));
}

int lipasr_mlp_input_grad(lipasr_mlp_t m, const float* params, const float* bnstate, const float* x,
                          const float* y_onehot, int batch, float* dx, lipasr_stream_t stream) {
  int rc = check_call("lipasr_mlp_input_grad", m, batch, bnstate);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(params && x && y_onehot && dx, "lipasr_mlp_input_grad: null argument");
  return attack_common(m, params, bnstate, x, y_onehot, batch, dx, nullptr, nullptr, 0.0f, 0.0f, S(stream));
}

int lipasr_mlp_attack_step(lipasr_mlp_t m, const float* params, const float* bnstate, float* x_adv, const float* x0,
                           const float* y_onehot, int batch, float alpha, float eps, lipasr_stream_t stream) {
  int rc = check_call("lipasr_mlp_attack_step", m, batch, bnstate);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(params && x_adv && x0 && y_onehot, "lipasr_mlp_attack_step: null argument");
  LP_CHECK_ARG(eps >= 0.0f && !(alpha != alpha), "lipasr_mlp_attack_step: eps=%g alpha=%g", (double)eps, (double)alpha);
  return attack_common(m, params, bnstate, x_adv, y_onehot, batch, nullptr, x_adv, x0, alpha, eps, S(stream));
}

// Lp FGM / PGD iteration: norm inf is lipasr_mlp_attack_step (the fused K4 epilogue).  L1 / L2: the dX GEMM of layer 0 stores g
// into the ping-pong gradient buffer that backward_infer does not read at layer 0 (both are max_batch x max(widths) wide, the
// input width included), then the row-wise step kernel of lp_attack.hip -- two launches, no allocation, capturable.
int lipasr_mlp_attack_step_lp(lipasr_mlp_t m, const float* params, const float* bnstate, float* x_adv, const float* x0,
                              const float* y_onehot, int batch, float norm, float alpha, float eps, lipasr_stream_t stream) {
  int code = 0;
  int rc = lp_norm_code("lipasr_mlp_attack_step_lp", norm, &code);
  if (rc != LIPASR_OK) return rc;
  if (code == 0) return lipasr_mlp_attack_step(m, params, bnstate, x_adv, x0, y_onehot, batch, alpha, eps, stream);
  rc = check_call("lipasr_mlp_attack_step_lp", m, batch, bnstate);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(params && x_adv && x0 && y_onehot, "lipasr_mlp_attack_step_lp: null argument");
  LP_CHECK_ARG(eps >= 0.0f && !(alpha != alpha), "lipasr_mlp_attack_step_lp: eps=%g alpha=%g", (double)eps, (double)alpha);
  // backward_infer writes layer n-1's input gradient into G0, then alternates: at layer 0 it reads G[(n-2) % 2]
  float* g = m->ws + (((m->n_layers - 1) & 1) ? m->offG1 : m->offG0);
  rc = attack_common(m, params, bnstate, x_adv, y_onehot, batch, g, nullptr, nullptr, 0.0f, 0.0f, S(stream));
  if (rc != LIPASR_OK) return rc;
  return lp_step_launch(x_adv, x0, g, batch, m->L[0].n_in, code, alpha, eps, S(stream));
}

int lipasr_mlp_output_vjp(lipasr_mlp_t m, const float* params, const float* bnstate, const float* x, const float* v,
                          int on_logits, int batch, float* probs_out, float* dx, lipasr_stream_t stream) {
  int rc = check_call("lipasr_mlp_output_vjp", m, batch, bnstate);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(params && x && v && dx, "lipasr_mlp_output_vjp: null argument");
  hipStream_t st = S(stream);
  float* lg = m->ws + m->offLogits;
  rc = forward_infer(m, params, bnstate, x, batch, true, lg, st);
  if (rc != LIPASR_OK) return rc;
  const int C = m->L[m->n_layers - 1].n_out;
  hipLaunchKernelGGL(softmax_vjp_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, lg, v, batch, C, on_logits ? 1 : 0,
                     probs_out, m->ws + m->offDzLast);
  LP_LAUNCH_CHECK();
  ++g_k2_launches[K2_SOFTMAX_VJP];
  return backward_infer(m, params, bnstate, batch, dx, nullptr, nullptr, 0.0f, 0.0f, st);
}

// The whole Jacobian from ONE forward: backward_infer only reads what forward_infer(keep_a) left (the post-ReLU activations) and
// writes the two ping-pong gradient buffers and dx, so the C backward chains follow one another on the same saved state.  The last
// dX GEMM stores class c's rows straight into the caller's layout (ldc = stride_b): n_layers (1 + C) GEMM launches and C small ones.
int lipasr_mlp_jacobian(lipasr_mlp_t m, const float* params, const float* bnstate, const float* x, int on_logits, int batch,
                        float* probs_out, float* jac, long stride_b, long stride_c, lipasr_stream_t stream) {
  int rc = check_call("lipasr_mlp_jacobian", m, batch, bnstate);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(params && x && jac, "lipasr_mlp_jacobian: null argument");
  const int C = m->L[m->n_layers - 1].n_out;
  const long n = m->L[0].n_in;
  LP_CHECK_ARG(C <= 32, "lipasr_mlp_jacobian: %d classes; at most 32 are supported", C);
  // [B][C][n] (rows of a sample together) or class-major [C][B][n], padded or not; nothing else is known not to overlap
  LP_CHECK_ARG((stride_c >= n && stride_b >= (long)C * stride_c) || (stride_b >= n && stride_c >= (long)batch * stride_b),
               "lipasr_mlp_jacobian: strides (%ld, %ld) are neither [batch][classes][%ld] nor [classes][batch][%ld]", stride_b, stride_c,
               n, n);
  LP_CHECK_ARG(stride_b <= 0x7fffffffL, "lipasr_mlp_jacobian: stride_b %ld does not fit a leading dimension", stride_b);
  hipStream_t st = S(stream);
  float* lg = m->ws + m->offLogits;
  rc = forward_infer(m, params, bnstate, x, batch, true, lg, st);
  if (rc != LIPASR_OK) return rc;
  for (int c = 0; c < C; ++c) {
    hipLaunchKernelGGL(softmax_vjp_onehot_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, lg, c, batch, C, on_logits ? 1 : 0,
                       c == 0 ? probs_out : (float*)nullptr, m->ws + m->offDzLast);
    LP_LAUNCH_CHECK();
    ++g_k2_launches[K2_SOFTMAX_VJP_ONEHOT];
    rc = backward_infer(m, params, bnstate, batch, jac + (size_t)c * stride_c, nullptr, nullptr, 0.0f, 0.0f, st, 1.0f, (int)stride_b);
    if (rc != LIPASR_OK) return rc;
  }
  return LIPASR_OK;
}

}  // extern "C"
