// The dense classifier's plan: layout of the parameters, the BatchNorm state and the workspace, the plan's settings, the test
// hooks, and what the two passes share (mlp.h).  The training step is mlp_train.hip, inference / attacks / class gradients are
// mlp_infer.hip; this unit holds no kernel.
#include "gemm.h"

namespace lipasr {

long g_k2_launches[K2_KERNELS] = {};

// arithmetic mode of a plan's GEMM + the fp16 range scales of mode 2 by operand kind.  Powers of two (exact): activations and
// features unscaled (|x| < 65504; BatchNorm outputs are O(1): their low plane is a normal fp16 number down to |x| = 0.12 and loses
// bits gradually below, on values that weigh little in a sum), kernels x 2^12 (|w| < 16), gradients x 2^8 / 2^floor(log2 g0) where g0 is the
// size of the gradient at the network's output (the loss gradient is <= 1 / batch: a batch of 1024 gives 2^18, and room for the
// gradient to grow 256-fold on its way down).  A value outside its range becomes inf in the fp16 conversion and the loss NaN --
// loud, not silently wrong.  The low plane keeps its full 11 bits while |x| scale >= 2^-3 and degrades gradually below (fp16
// subnormals): with the first gradient scale tried, a fixed 2^14, the bias gradients of a 1024-row batch (sums of 1024 terms of
// 1e-6 that cancel to 5e-7) came out 9e-5 off; scaled by the batch they are inside the exact mode's 5e-5.
static float grad_scale_for(float g0) {  // g0: bound of the gradient at the logits (inv_batch, or 1 for a caller-given upstream vector)
  int e = 0;
  (void)frexpf(g0 > 0.0f ? g0 : 1.0f, &e);  // g0 = f 2^e, f in [0.5, 1)
  return ldexpf(1.0f, 8 - e);               // 2^8 / 2^e >= 2^8 / (2 g0)
}
int plan_cus(const lipasr_mlp* m) { return m->cu_budget > 0 ? std::min(m->cu_budget, m->n_cus) : m->n_cus; }
void set_arith(GemmArgs& g, const lipasr_mlp* m, int kind_a, int kind_b, float g0, bool training) {
  // Mode 2 is a TRAINING arithmetic: there the activations are BatchNorm outputs (bounded by construction) and the gradients carry
  // their own measured scale.  Inference-mode activations have no such bound (BatchNorm with moving statistics that have not
  // adapted yet passes 1e4-sized values: the fp16 conversion overflowed in the first suite run) -- predict / attacks / class
  // gradients stay on the exact fp32 chains, so every logit-parity statement is about exact fp32 whatever the training mode.
  g.bf16 = (m->compute_bf16 == 2 && !training) ? 0 : m->compute_bf16;
  g.zeros = reinterpret_cast<const float*>(m->xc_ctrl + 4);  // words 4 .. 7 of the control block: never written
  g.cus = plan_cus(m);
  const float sc[3] = {1.0f, 4096.0f, grad_scale_for(g0)};
  g.sa = sc[kind_a];
  g.sb = sc[kind_b];
}

int check_batch(const char* fn, const lipasr_mlp* m, int batch) {
  LP_CHECK_ARG(m != nullptr, "%s: null plan", fn);
  LP_CHECK_ARG(batch >= 1 && batch <= m->max_batch, "%s: batch %d outside [1, %d]", fn, batch, m->max_batch);
  return LIPASR_OK;
}
int check_call(const char* fn, const lipasr_mlp* m, int batch, const float* bnstate) {
  int rc = check_batch(fn, m, batch);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(m->n_state == 0 || bnstate, "%s: bnstate is null", fn);
  return LIPASR_OK;
}

static inline size_t align4(size_t x) { return (x + 3) & ~size_t(3); }

void mlp_plan_free(lipasr_mlp* m) {
  if (!m) return;
  if (m->ws) (void)hipFree(m->ws);
  if (m->xc_gran) (void)hipFree(m->xc_gran);
  if (m->xc_ctrl) (void)hipFree(m->xc_ctrl);
  delete m;
}

}  // namespace lipasr

using namespace lipasr;

// ------------------------------------------------------------------------------------------------
// plan
// ------------------------------------------------------------------------------------------------
extern "C" {
int lipasr_mlp_create(lipasr_handle_t h, int n_layers, const int* widths, const int* bn, const float* dropout,
                      const int* nonneg, int max_batch, lipasr_mlp_t* out) {
  LP_CHECK_ARG(h && widths && out, "lipasr_mlp_create: null argument");
  LP_CHECK_ARG(n_layers >= 1 && n_layers <= LIPASR_MAX_LAYERS, "lipasr_mlp_create: n_layers=%d outside [1,%d]", n_layers,
               LIPASR_MAX_LAYERS);
  LP_CHECK_ARG(max_batch >= 1, "lipasr_mlp_create: max_batch=%d", max_batch);
  for (int l = 0; l <= n_layers; ++l) LP_CHECK_ARG(widths[l] >= 1, "lipasr_mlp_create: widths[%d]=%d", l, widths[l]);
  LP_CHECK_ARG(widths[n_layers] <= 32, "lipasr_mlp_create: %d classes; at most 32 are supported", widths[n_layers]);
  lipasr_mlp* m = new lipasr_mlp();
  m->ctx = h;
  m->n_layers = n_layers;
  m->max_batch = max_batch;
  size_t po = 0, so = 0, wo = 0;
  int maxw = widths[0];
  for (int l = 0; l < n_layers; ++l) {
    MlpLayer& L = m->L[l];
    L.n_in = widths[l];
    L.n_out = widths[l + 1];
    const bool last = (l == n_layers - 1);
    L.bn = !last && bn && bn[l];
    L.dropout = (!last && dropout) ? dropout[l] : 0.0f;
    L.nonneg = nonneg && nonneg[l];
    if (L.dropout < 0.0f || L.dropout >= 1.0f) {
      delete m;
      set_error("lipasr_mlp_create: dropout[%d]=%g outside [0,1)", l, (double)L.dropout);
      return LIPASR_EINVAL;
    }
    maxw = L.n_out > maxw ? L.n_out : maxw;
    L.offW = po; po = align4(po + (size_t)L.n_in * L.n_out);
    L.offb = po; po = align4(po + L.n_out);
    if (L.bn) {
      L.offg = po; po = align4(po + L.n_out);
      L.offbe = po; po = align4(po + L.n_out);
      L.offmm = so; so = align4(so + L.n_out);
      L.offmv = so; so = align4(so + L.n_out);
    }
    if (!last) {
      L.offA = wo; wo = align4(wo + (size_t)max_batch * L.n_out);
      if (L.bn || L.dropout > 0.0f) { L.offH = wo; wo = align4(wo + (size_t)max_batch * L.n_out); }
      else L.offH = L.offA;
      L.offMean = wo; wo = align4(wo + 2 * (size_t)L.n_out);
    }
    L.offDz = wo; wo = align4(wo + (size_t)max_batch * L.n_out);
  }
  m->n_params = po;
  m->n_state = so;
  m->max_width = maxw;
  const size_t C = widths[n_layers];
  m->offLogits = wo; wo = align4(wo + (size_t)max_batch * C);
  m->offProb = wo; wo = align4(wo + (size_t)max_batch * C);
  m->offDzLast = wo; wo = align4(wo + (size_t)max_batch * C);
  m->offG0 = wo; wo = align4(wo + (size_t)max_batch * maxw);
  m->offG1 = wo; wo = align4(wo + (size_t)max_batch * maxw);
  m->offPart = wo; wo = align4(wo + 2 * (size_t)part_row_tiles(max_batch) * maxw);  // column partials of the *_STATS epilogues
  m->ws_floats = wo;
  DeviceGuard g(h->device);
  if (hipMalloc(&m->ws, wo * sizeof(float)) != hipSuccess) {
    delete m;
    set_error("lipasr_mlp_create: workspace allocation of %zu bytes failed", wo * sizeof(float));
    return LIPASR_ENOMEM;
  }
  (void)hipMemset(m->ws, 0, wo * sizeof(float));
  // exchange epilogue state (round 5): granules and control words per BatchNorm layer and direction, all zero (tag 0 is never used)
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) == hipSuccess) m->n_cus = prop.multiProcessorCount;
    m->xc_rt_max = std::min(part_row_tiles(max_batch), 64);
    const size_t amax_words = (size_t)LIPASR_MAX_LAYERS * kAmaxSlots * kAmaxStride;
    size_t go = 0, co = 16 + amax_words;  // control words 0 .. 15: the error word (its own 64-byte slot), then amax[layer][slot]
    for (int dir = 0; dir < 2; ++dir)
      for (int l = 0; l + 1 < n_layers; ++l) {
        if (!m->L[l].bn) continue;
        const size_t nblk = (size_t)(m->L[l].n_out + 31) / 32;
        m->xc_gran_off[dir][l] = go; go += nblk * m->xc_rt_max * 128;
        m->xc_ctrl_off[dir][l] = co; co += nblk * 32;
      }
    if (hipMalloc(&m->xc_ctrl, co * sizeof(unsigned)) != hipSuccess) {
      (void)hipGetLastError();
      mlp_plan_free(m);
      set_error("lipasr_mlp_create: control-word allocation failed");
      return LIPASR_ENOMEM;
    }
    (void)hipMemset(m->xc_ctrl, 0, co * sizeof(unsigned));
    m->xc_err = reinterpret_cast<int*>(m->xc_ctrl);
    m->amax = m->xc_ctrl + 16;  // layer l: amax_slot(m, l) (mlp_train.hip)
    if (go > 0) {
      if (hipMalloc(&m->xc_gran, go * sizeof(unsigned long long)) != hipSuccess) {
        (void)hipGetLastError();
        m->xc_gran = nullptr;  // no exchange state: the launch chain is used
      } else {
        (void)hipMemset(m->xc_gran, 0, go * sizeof(unsigned long long));
      }
    }
  }
  h->mlps.push_back(m);
  *out = m;
  return LIPASR_OK;
}

int lipasr_mlp_destroy(lipasr_mlp_t m) {
  LP_CHECK_ARG(m != nullptr, "lipasr_mlp_destroy: null plan");
  DeviceGuard g(m->ctx->device);
  std::vector<lipasr_mlp*>& v = m->ctx->mlps;
  for (size_t i = 0; i < v.size(); ++i)
    if (v[i] == m) { v.erase(v.begin() + i); break; }
  lipasr::mlp_plan_free(m);
  return LIPASR_OK;
}

int lipasr_mlp_sizes(lipasr_mlp_t m, size_t* n_params, size_t* n_state) {
  LP_CHECK_ARG(m && n_params && n_state, "lipasr_mlp_sizes: null argument");
  *n_params = m->n_params;
  *n_state = m->n_state;
  return LIPASR_OK;
}

int lipasr_mlp_segment(lipasr_mlp_t m, int layer, int kind, size_t* offset, size_t* count) {
  LP_CHECK_ARG(m && offset && count, "lipasr_mlp_segment: null argument");
  LP_CHECK_ARG(layer >= 0 && layer < m->n_layers, "lipasr_mlp_segment: layer %d out of range", layer);
  const MlpLayer& L = m->L[layer];
  switch (kind) {
    case LIPASR_SEG_W: *offset = L.offW; *count = (size_t)L.n_in * L.n_out; break;
    case LIPASR_SEG_B: *offset = L.offb; *count = L.n_out; break;
    case LIPASR_SEG_GAMMA: *offset = L.offg; *count = L.bn ? L.n_out : 0; break;
    case LIPASR_SEG_BETA: *offset = L.offbe; *count = L.bn ? L.n_out : 0; break;
    case LIPASR_SEG_MMEAN: *offset = L.offmm; *count = L.bn ? L.n_out : 0; break;
    case LIPASR_SEG_MVAR: *offset = L.offmv; *count = L.bn ? L.n_out : 0; break;
    default: set_error("lipasr_mlp_segment: unknown kind %d", kind); return LIPASR_EINVAL;
  }
  return LIPASR_OK;
}

int lipasr_mlp_set_gemm_tiles(lipasr_mlp_t m, int lds_min_tiles) {
  LP_CHECK_ARG(m != nullptr && lds_min_tiles >= 0, "lipasr_mlp_set_gemm_tiles: bad argument");
  m->lds_min_tiles = lds_min_tiles;
  return LIPASR_OK;
}

int lipasr_mlp_set_fuse_bn(lipasr_mlp_t m, int mode) {
  LP_CHECK_ARG(m != nullptr && (mode == 0 || mode == 1), "lipasr_mlp_set_fuse_bn: bad argument");
  m->fuse_bn = mode;
  return LIPASR_OK;
}

int lipasr_mlp_set_cu_budget(lipasr_mlp_t m, int n_cus) {
  LP_CHECK_ARG(m != nullptr && n_cus >= 0, "lipasr_mlp_set_cu_budget: bad argument");
  m->cu_budget = n_cus;
  return LIPASR_OK;
}

int lipasr_mlp_exchange_errors(lipasr_mlp_t m, int* errors_host) {
  LP_CHECK_ARG(m != nullptr && errors_host != nullptr, "lipasr_mlp_exchange_errors: null argument");
  *errors_host = 0;
  if (!m->xc_err) return LIPASR_OK;
  DeviceGuard g(m->ctx->device);
  LP_HIP(hipMemcpy(errors_host, m->xc_err, sizeof(int), hipMemcpyDeviceToHost));  // synchronises with the device
  if (*errors_host) LP_HIP(hipMemset(m->xc_err, 0, sizeof(int)));
  return LIPASR_OK;
}

int lipasr_mlp_set_compute(lipasr_mlp_t m, int mode) {
  LP_CHECK_ARG(m != nullptr, "lipasr_mlp_set_compute: null plan");
  LP_CHECK_ARG(mode >= 0 && mode <= 2, "lipasr_mlp_set_compute: mode %d (0 = exact fp32, 1 = bf16 operands, 2 = fp16 two-plane split)", mode);
  if (mode == 2) {
    // the split needs operands inside fp16's range: gradients carry a measured scale, kernels are small, and the activations are
    // bounded because they are BatchNorm outputs -- so every hidden layer must have one (the reference's models do:
    // train_constraints.py:67-85); a network without runs its activations up without bound (all-positive kernels: 1e4 and more)
    for (int l = 0; l + 1 < m->n_layers; ++l)
      if (!m->L[l].bn) {
        set_error("lipasr_mlp_set_compute: mode 2 (fp16 two-plane split) needs BatchNormalization after every hidden Dense layer (layer %d has none); use mode 0", l);
        return LIPASR_EUNSUPPORTED;
      }
  }
  m->compute_bf16 = mode;
  return LIPASR_OK;
}

// ---------------------------------------------------------------- test hooks of the training step's own kernels
long lipasr_debug_k2_launches(int kernel) { return (kernel >= 0 && kernel < K2_KERNELS) ? g_k2_launches[kernel] : -1; }

int lipasr_debug_mlp_stage(lipasr_mlp_t m, int layer, int which, int batch, float* out, lipasr_stream_t stream) {
  LP_CHECK_ARG(m != nullptr && out != nullptr, "lipasr_debug_mlp_stage: null argument");
  LP_CHECK_ARG(layer >= 0 && layer < m->n_layers, "lipasr_debug_mlp_stage: layer %d outside [0, %d)", layer, m->n_layers);
  LP_CHECK_ARG(batch >= 1 && batch <= m->max_batch, "lipasr_debug_mlp_stage: batch %d outside [1, %d]", batch, m->max_batch);
  const MlpLayer& L = m->L[layer];
  const bool last = layer == m->n_layers - 1;
  const float* src = nullptr;
  size_t n = (size_t)batch * L.n_out;
  switch (which) {
    case 0: if (!last) src = m->ws + L.offA; break;
    case 1: if (!last) src = m->ws + L.offH; break;
    case 2: if (!last && L.bn) { src = m->ws + L.offMean; n = 2 * (size_t)L.n_out; } break;
    case 3: src = m->ws + (last ? m->offDzLast : L.offDz); break;
    case 4: if (!last && L.bn) src = m->ws + m->offG0; break;
    case 5: if (last) src = m->ws + m->offLogits; break;
    case 6: if (last) src = m->ws + m->offProb; break;
    default: break;
  }
  LP_CHECK_ARG(src != nullptr, "lipasr_debug_mlp_stage: layer %d has no stage %d (0 A, 1 H, 2 [mean | rstd], 3 dz, 4 g, 5 logits, 6 probabilities)",
               layer, which);
  DeviceGuard g(m->ctx->device);
  LP_HIP(hipMemcpyAsync(out, src, n * sizeof(float), hipMemcpyDeviceToDevice, S(stream)));
  return LIPASR_OK;
}

}  // extern "C"
