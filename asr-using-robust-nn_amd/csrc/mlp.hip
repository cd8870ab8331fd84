// The dense classifier's plan: BatchNorm / dropout / softmax-CE kernels and the plan-level forward / backward / predict /
// attack sequences.  Every GEMM goes through the launchers of gemm.hip (gemm.h).
#include "gemm.h"
#include <cstdlib>

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
enum OperandKind { OP_ACT = 0, OP_WEIGHT = 1, OP_GRAD = 2 };
static float grad_scale_for(float g0) {  // g0: bound of the gradient at the logits (inv_batch, or 1 for a caller-given upstream vector)
  int e = 0;
  (void)frexpf(g0 > 0.0f ? g0 : 1.0f, &e);  // g0 = f 2^e, f in [0.5, 1)
  return ldexpf(1.0f, 8 - e);               // 2^8 / 2^e >= 2^8 / (2 g0)
}
static int plan_cus(const lipasr_mlp* m) { return m->cu_budget > 0 ? std::min(m->cu_budget, m->n_cus) : m->n_cus; }  // the CUs the plan's stream may use
static void set_arith(GemmArgs& g, const lipasr_mlp* m, int kind_a, int kind_b, float g0 = 1.0f, bool training = true) {
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
// BatchNorm inside the producing GEMM (the exchange epilogue)?  forward: the NN GEMM, else the input-gradient (NT) GEMM
static bool bnx_fits(const lipasr_mlp* m, bool forward, int M, int N, int K) {
  if (!m->fuse_bn || !m->xc_gran) return false;
  return exchange_fits(forward ? 1 : 0, m->compute_bf16, M, N, K, m->lds_min_tiles, m->xc_rt_max, plan_cus(m));
}
#ifdef LIPASR_PROBES
// LIPASR_XC_NOWAIT=1 (timing probe only, results are WRONG): the exchange epilogue without its wait and sweep, to see what the
// exchange instances cost apart from the exchange.  Compiled in with -DLIPASR_PROBES only; the default build never reads it.
static bool xc_nowait() { static const bool on = getenv("LIPASR_XC_NOWAIT") != nullptr; return on; }
#else
constexpr bool xc_nowait() { return false; }
#endif

// ---------------------------------------------------------------------------------------------
// BatchNorm / dropout apply kernels.  The column statistics arrive as per-row-tile partial sums from
// the producing GEMM's epilogue, so these are plain 2-D elementwise kernels: grid = (column strips of
// 128, row chunks of 32), 256 threads = 32 float4 column lanes x 8 row lanes, each workgroup re-sums
// the (few) partials of its columns in fp64 in its prologue.  No cross-workgroup step, fixed order.
// ---------------------------------------------------------------------------------------------
constexpr int kApplyRows = 32;

struct ColLane {
  int j;      // first of this lane's 4 columns
  bool vec;   // float4 access is legal
  int N;
};

__device__ __forceinline__ void ld4(const float* __restrict__ p, size_t row_off, const ColLane& c, float (&v)[4]) {
  if (c.vec) {
    const float4 t = *reinterpret_cast<const float4*>(p + row_off + c.j);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (c.j + e < c.N) ? p[row_off + c.j + e] : 0.0f;
  }
}
__device__ __forceinline__ void st4(float* __restrict__ p, size_t row_off, const ColLane& c, const float (&v)[4]) {
  if (c.vec) {
    *reinterpret_cast<float4*>(p + row_off + c.j) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c.j + e < c.N) p[row_off + c.j + e] = v[e];
  }
}

// sums the two statistic planes of `part` over the row tiles for this lane's 4 columns (fp64, fixed order)
__device__ __forceinline__ void sum_partials(const float* __restrict__ part, int n_tiles, const ColLane& c, int rl,
                                             double (*lds)[32][8], int cl, double (&s1)[4], double (&s2)[4]) {
  double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int t = rl; t < n_tiles; t += 8) {
    float v1[4], v2[4];
    ld4(part, (size_t)t * c.N, c, v1);
    ld4(part, ((size_t)n_tiles + t) * c.N, c, v2);
#pragma unroll
    for (int e = 0; e < 4; ++e) { a[e] += (double)v1[e]; a[4 + e] += (double)v2[e]; }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) lds[rl][cl][e] = a[e];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    double t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { t1 += lds[k][cl][e]; t2 += lds[k][cl][4 + e]; }
    s1[e] = t1;
    s2[e] = t2;
  }
}

// Synchronized BatchNorm: the row-tile partial sums [2][n_tiles][N] of this rank are reduced to [2][N] IN PLACE before the
// exchange (fp64 accumulation in tile order, one thread per column: it reads all of its 2 n_tiles inputs before it writes the
// two slots, which are inputs of that thread only), so the collective's length is 2 N whatever the rank's row count and tile
// size -- ranks with different shard sizes exchange the same number of floats -- and the apply kernels read
// n_tiles = 1.
__global__ __launch_bounds__(256) void part_reduce_kernel(float* __restrict__ part, int n_tiles, int N) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= N) return;
  double s1 = 0.0, s2 = 0.0;
  for (int t = 0; t < n_tiles; ++t) {
    s1 += (double)part[(size_t)t * N + col];
    s2 += (double)part[((size_t)n_tiles + t) * N + col];
  }
  part[col] = (float)s1;
  part[(size_t)N + col] = (float)s2;
}

struct BnFwdArgs {
  const float* a;  // [B][N] post-ReLU
  float* h;        // [B][N] out
  int B, N, has_bn, n_tiles;
  int Bstat;          // rows the statistics are taken over (= B; synchronized BatchNorm: the global batch)
  const float* part;  // [2][n_tiles][N]: sums of a and a^2 per row tile
  const float* gamma;
  const float* beta;
  float* mmean;
  float* mvar;
  float* save_mean;  // [N], rstd at save_mean + N
  DropArgs drop;
};

// training-mode BatchNorm (batch mean, population variance) + inverted dropout
__global__ __launch_bounds__(256) void bn_apply_fwd_kernel(BnFwdArgs p) {
  __shared__ double lds[8][32][8];
  const int tid = threadIdx.x, cl = tid & 31, rl = tid >> 5;
  ColLane c;
  c.j = blockIdx.x * 128 + 4 * cl;
  c.N = p.N;
  c.vec = ((p.N & 3) == 0) && (c.j + 3 < p.N);
  const bool live = c.j < p.N;
  const int step = p.drop.step_dev ? *p.drop.step_dev : 0;
  float mean[4] = {0, 0, 0, 0}, rstd[4] = {1, 1, 1, 1}, ga[4] = {1, 1, 1, 1}, be[4] = {0, 0, 0, 0};
  // this thread's activations start their trip before the statistics are reduced (one memory round trip less)
  float xin[kApplyRows / 8][4];
#pragma unroll
  for (int i = 0; i < kApplyRows / 8; ++i) {
    const int b = blockIdx.y * kApplyRows + rl + 8 * i;
#pragma unroll
    for (int e = 0; e < 4; ++e) xin[i][e] = 0.0f;
    if (live && b < p.B) ld4(p.a, (size_t)b * p.N, c, xin[i]);
  }
  if (p.has_bn) {
    double s1[4], s2[4];
    ColLane cc = c;
    if (!live) { cc.j = 0; cc.vec = false; cc.N = 0; }
    sum_partials(p.part, p.n_tiles, cc, rl, lds, cl, s1, s2);
    if (live) {
      float var[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double m = s1[e] / (double)p.Bstat;
        double v = s2[e] / (double)p.Bstat - m * m;
        v = v > 0.0 ? v : 0.0;
        mean[e] = (float)m;
        var[e] = (float)v;
        rstd[e] = (float)(1.0 / sqrt(v + (double)kBnEps));
      }
      ld4(p.gamma, 0, c, ga);
      ld4(p.beta, 0, c, be);
      if (blockIdx.y == 0 && rl == 0) {
        float mm[4], mv[4];
        ld4(p.mmean, 0, c, mm);
        ld4(p.mvar, 0, c, mv);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          mm[e] = mm[e] * kBnMomentum + mean[e] * (1.0f - kBnMomentum);
          mv[e] = mv[e] * kBnMomentum + var[e] * (1.0f - kBnMomentum);
        }
        st4(p.mmean, 0, c, mm);
        st4(p.mvar, 0, c, mv);
        st4(p.save_mean, 0, c, mean);
        st4(p.save_mean, (size_t)p.N, c, rstd);
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int i = 0; i < kApplyRows / 8; ++i) {
    const int b = blockIdx.y * kApplyRows + rl + 8 * i;
    if (b >= p.B) break;
    const size_t ro = (size_t)b * p.N;
    float x[4], dm[4];
    dropout_mult4(p.drop, step, b, p.N, c.j, p.N, dm);
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = xin[i][e];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (p.has_bn) x[e] = (x[e] - mean[e]) * rstd[e] * ga[e] + be[e];
      x[e] *= dm[e];
    }
    st4(p.h, ro, c, x);
  }
}

struct BnBwdArgs {
  const float* g;   // [B][N] dh * dropout (from the producing GEMM's epilogue)
  const float* a;   // [B][N] post-ReLU
  float* dz;        // [B][N] gradient w.r.t. the pre-activation
  int B, N, n_tiles;
  int Bstat;          // rows the statistics were taken over (= B; synchronized BatchNorm: the global batch)
  float grad_scale;   // 1, or 1 / world when the partial sums were all-reduced (the gradient all-reduce sums them again)
  const float* part;  // [2][n_tiles][N]: sums of g and g * xhat per row tile
  const float* gamma;
  const float* save_mean;
  float* dgamma;
  float* dbeta;
  unsigned* amax_out;  // arithmetic mode 2: max |dz| is folded into this word (see GemmArgs::amax_out); may be null
};

// backward of BatchNorm(train) -> ReLU given the column sums; also writes dgamma / dbeta
__global__ __launch_bounds__(256) void bn_apply_bwd_kernel(BnBwdArgs p) {
  __shared__ double lds[8][32][8];
  const int tid = threadIdx.x, cl = tid & 31, rl = tid >> 5;
  ColLane c;
  c.j = blockIdx.x * 128 + 4 * cl;
  c.N = p.N;
  c.vec = ((p.N & 3) == 0) && (c.j + 3 < p.N);
  const bool live = c.j < p.N;
  float gin[kApplyRows / 8][4], ain[kApplyRows / 8][4];
#pragma unroll
  for (int i = 0; i < kApplyRows / 8; ++i) {
    const int b = blockIdx.y * kApplyRows + rl + 8 * i;
#pragma unroll
    for (int e = 0; e < 4; ++e) { gin[i][e] = 0.0f; ain[i][e] = 0.0f; }
    if (live && b < p.B) {
      ld4(p.g, (size_t)b * p.N, c, gin[i]);
      ld4(p.a, (size_t)b * p.N, c, ain[i]);
    }
  }
  double s1[4], s2[4];
  ColLane cc = c;
  if (!live) { cc.j = 0; cc.vec = false; cc.N = 0; }
  sum_partials(p.part, p.n_tiles, cc, rl, lds, cl, s1, s2);
  float omax = 0.0f;
  if (live) {
  float mean[4], rstd[4], ga[4], dbt[4], dg[4];
  ld4(p.save_mean, 0, c, mean);
  ld4(p.save_mean, (size_t)p.N, c, rstd);
  ld4(p.gamma, 0, c, ga);
#pragma unroll
  for (int e = 0; e < 4; ++e) { dbt[e] = (float)s1[e]; dg[e] = (float)s2[e]; }
  if (blockIdx.y == 0 && rl == 0) {
    float ob[4], og[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { ob[e] = dbt[e] * p.grad_scale; og[e] = dg[e] * p.grad_scale; }
    st4(p.dbeta, 0, c, ob);
    st4(p.dgamma, 0, c, og);
  }
  const float invB = 1.0f / (float)p.Bstat;
#pragma unroll
  for (int i = 0; i < kApplyRows / 8; ++i) {
    const int b = blockIdx.y * kApplyRows + rl + 8 * i;
    if (b >= p.B) break;
    const size_t ro = (size_t)b * p.N;
    float gv[4], av[4], o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { gv[e] = gin[i][e]; av[e] = ain[i][e]; }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xh = (av[e] - mean[e]) * rstd[e];
      const float d = ga[e] * rstd[e] * (gv[e] - dbt[e] * invB - xh * dg[e] * invB);
      o[e] = av[e] > 0.0f ? d : 0.0f;
      if (c.j + e < c.N) omax = fmaxf(omax, fabsf(o[e]));
    }
    st4(p.dz, ro, c, o);
  }
  }
  if (p.amax_out) amax_publish(p.amax_out, omax);
}

// upstream vector at the network output -> dz at the logits, one thread per row (class_gradient and the
// optimisation-based attacks): on_logits: dz = v;  else out = softmax(z): dz = p * (v - sum_c p_c v_c)
__global__ __launch_bounds__(256) void softmax_vjp_kernel(const float* __restrict__ z, const float* __restrict__ v, int B,
                                                           int C, int on_logits, float* __restrict__ prob,
                                                           float* __restrict__ dz) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const float* zr = z + (size_t)b * C;
  const float* vr = v + (size_t)b * C;
  float mx = zr[0];
  for (int c = 1; c < C; ++c) mx = fmaxf(mx, zr[c]);
  float se = 0.0f;
  for (int c = 0; c < C; ++c) se += expf(zr[c] - mx);
  const float inv = 1.0f / se;
  float dot = 0.0f;
  for (int c = 0; c < C; ++c) dot = fmaf(expf(zr[c] - mx) * inv, vr[c], dot);
  for (int c = 0; c < C; ++c) {
    const float pc = expf(zr[c] - mx) * inv;
    if (prob) prob[(size_t)b * C + c] = pc;
    dz[(size_t)b * C + c] = on_logits ? vr[c] : pc * (vr[c] - dot);
  }
}

// softmax_vjp_kernel for the one-hot upstream vector e_cls, made in registers instead of read: the same operations in the same
// order, so dz is the one softmax_vjp_kernel gives for that vector, bit for bit (lipasr_mlp_jacobian: one launch per class, no
// [B][C] vector to upload)
__global__ __launch_bounds__(256) void softmax_vjp_onehot_kernel(const float* __restrict__ z, int cls, int B, int C, int on_logits,
                                                                  float* __restrict__ prob, float* __restrict__ dz) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const float* zr = z + (size_t)b * C;
  float mx = zr[0];
  for (int c = 1; c < C; ++c) mx = fmaxf(mx, zr[c]);
  float se = 0.0f;
  for (int c = 0; c < C; ++c) se += expf(zr[c] - mx);
  const float inv = 1.0f / se;
  float dot = 0.0f;
  for (int c = 0; c < C; ++c) dot = fmaf(expf(zr[c] - mx) * inv, c == cls ? 1.0f : 0.0f, dot);
  for (int c = 0; c < C; ++c) {
    const float pc = expf(zr[c] - mx) * inv;
    const float vc = c == cls ? 1.0f : 0.0f;
    if (prob) prob[(size_t)b * C + c] = pc;
    dz[(size_t)b * C + c] = on_logits ? vc : pc * (vc - dot);
  }
}

// softmax + categorical cross-entropy from logits, one thread per row.
//   prob (optional), dz = (p - y) * inv_batch (optional), loss_rows = -sum y log_softmax(z) (optional),
//   correct_rows = [argmax p == argmax y] (optional), onehot_out = one-hot argmax z (optional)
__global__ __launch_bounds__(256) void softmax_ce_kernel(const float* __restrict__ z, const float* __restrict__ y, int B,
                                                          int C, float inv_batch, float* __restrict__ prob,
                                                          float* __restrict__ dz, float* __restrict__ loss_rows,
                                                          float* __restrict__ correct_rows,
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
  const float lse = logf(se);
  const float inv = 1.0f / se;
  float loss = 0.0f, ymax = -INFINITY;
  int ay = 0;
  for (int c = 0; c < C; ++c) {
    const float zs = zr[c] - mx;
    const float pc = expf(zs) * inv;
    if (prob) prob[(size_t)b * C + c] = pc;
    if (y) {
      const float yc = y[(size_t)b * C + c];
      if (yc != 0.0f) loss -= yc * (zs - lse);
      if (yc > ymax) { ymax = yc; ay = c; }
      if (dz) dz[(size_t)b * C + c] = (pc - yc) * inv_batch;
    }
    if (onehot_out) onehot_out[(size_t)b * C + c] = (c == am) ? 1.0f : 0.0f;
  }
  if (loss_rows) loss_rows[b] = loss;
  if (correct_rows) correct_rows[b] = (am == ay) ? 1.0f : 0.0f;
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
  m->offG2 = wo; wo = align4(wo + (size_t)max_batch * maxw);
  m->offPart = wo; wo = align4(wo + 2 * (size_t)((max_batch + 31) / 32) * maxw);  // column partials of the *_STATS epilogues
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
    m->xc_rt_max = std::min((max_batch + 31) / 32, 64);
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
    m->amax = m->xc_ctrl + 16;  // layer l: m->amax + l * kAmaxSlots * kAmaxStride
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

}  // extern "C"

namespace lipasr {

static int check_batch(const char* fn, lipasr_mlp_t m, int batch) {
  LP_CHECK_ARG(m != nullptr, "%s: null plan", fn);
  LP_CHECK_ARG(batch >= 1 && batch <= m->max_batch, "%s: batch %d outside [1, %d]", fn, batch, m->max_batch);
  return LIPASR_OK;
}

static DropArgs drop_for_layer(const lipasr_mlp* m, int l, const lipasr_dropout_cfg* cfg) {
  DropArgs d;
  memset(&d, 0, sizeof(d));
  d.rate = m->L[l].dropout;
  d.layer = l;
  if (!cfg || cfg->mode == 0 || d.rate <= 0.0f) { d.mode = 0; return d; }
  d.mode = cfg->mode;
  d.seed = cfg->seed;
  d.step_dev = cfg->step_dev;
  d.mask = (cfg->mode == 2 && cfg->masks) ? cfg->masks[l] : nullptr;
  if (cfg->mode == 2 && d.mask == nullptr) d.mode = 0;
  return d;
}

// inference-mode forward: fills A_l (post-ReLU, if keep_a) and H_l, logits into m->ws
// ce_y != nullptr (and <= 32 classes): the last GEMM's epilogue also produces softmax, and (p - y) / batch at
// m->ws + offDzLast -- the caller then skips softmax_ce_kernel.  Returns through *fused whether it did.
static int forward_infer(lipasr_mlp* m, const float* params, const float* bnstate, const float* x, int batch,
                         bool keep_a, float* logits_out, hipStream_t st, const float* ce_y = nullptr,
                         bool* fused = nullptr) {
  const float* hin = x;
  if (fused) *fused = false;
  for (int l = 0; l < m->n_layers; ++l) {
    const MlpLayer& L = m->L[l];
    const bool last = (l == m->n_layers - 1);
    float* outp = last ? logits_out : (m->ws + L.offH);
    const bool fuse = last && ce_y && L.n_out <= 32;
    GemmArgs g = gemm_args(hin, L.n_in, params + L.offW, L.n_out, outp, L.n_out, batch, L.n_out, L.n_in,
                           last ? (fuse ? EPI_BIAS_SOFTMAX_CE : EPI_BIAS) : EPI_BIAS_RELU_BN);
    g.bias = params + L.offb;
    if (fuse) {
      g.y = ce_y;
      g.inv_batch = 1.0f / (float)batch;
      g.prob = m->ws + m->offProb;
      g.dz = m->ws + m->offDzLast;
      if (fused) *fused = true;
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

}  // namespace lipasr

extern "C" {

// dw_mode 0: every weight gradient from ONE grouped launch; 1: the first layer's [dW; db] as its own launch after the
// grouped launch of the others (LDS-tiled 64x64 kernel when legal); 2: the first layer's left out (lipasr_mlp_train_dw0)
// Segments (synchronized BatchNorm under data parallelism): the launch sequence is cut after every GEMM whose epilogue
// leaves BatchNorm column partial sums (forward: sums of a, a^2; backward: sums of g, g xhat), i.e. right before the
// apply kernel that consumes them.  seg < 0 runs everything; otherwise only the launches of segment `seg`, and the caller
// SUM-all-reduces the partials (segment_exchange_floats) before it runs the next one.  part_ext: caller-owned partials
// buffer (a torch tensor the caller can hand to its collective), stat_batch: rows the statistics cover (global batch).
struct SegArgs {
  int seg = -1;
  float* part_ext = nullptr;
  int stat_batch = 0;
  float grad_scale = 1.0f;
};

static int train_fwd_bwd_impl(lipasr_mlp_t m, const float* params, float* bnstate, const float* x, const float* y_onehot,
                              int batch, float inv_batch, const lipasr_dropout_cfg* dropout, float* grads,
                              float* loss_rows, float* correct_rows, float* probs, lipasr_stream_t stream, int dw_mode,
                              const SegArgs& sa = SegArgs()) {
  int rc = check_batch("lipasr_mlp_train_fwd_bwd", m, batch);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(params && x && y_onehot && grads, "lipasr_mlp_train_fwd_bwd: null argument");
  LP_CHECK_ARG(m->n_state == 0 || bnstate, "lipasr_mlp_train_fwd_bwd: bnstate is null");
  LP_CHECK_ARG(!dropout || (dropout->mode >= 0 && dropout->mode <= 2), "lipasr_mlp_train_fwd_bwd: dropout mode %d",
               dropout ? dropout->mode : 0);
  hipStream_t st = S(stream);
  m->last_inv_batch = inv_batch;
  const int Lc = m->n_layers;
  const int C = m->L[Lc - 1].n_out;
  float* ws = m->ws;
  float* part = sa.part_ext ? sa.part_ext : (ws + m->offPart);
  const dim3 apply_block(256);
  const int bstat = sa.stat_batch > 0 ? sa.stat_batch : batch;
  int cur = 0;  // current segment
#define LP_ON (sa.seg < 0 || sa.seg == cur)

  // ---- forward (training mode): GEMM (+bias, ReLU, column partials) -> BatchNorm/dropout apply
  const float* hin = x;
  for (int l = 0; l < Lc; ++l) {
    const MlpLayer& L = m->L[l];
    const bool last = (l == Lc - 1);
    float* outp = last ? (ws + m->offLogits) : (ws + L.offA);
    const bool fuse_ce = last && C <= 32;  // softmax, loss and (p - y) / B in the last GEMM's epilogue
    // BatchNorm inside this GEMM (exchange epilogue) where the whole grid can be resident; not with synchronized BatchNorm,
    // whose sums leave the device between the GEMM and the apply kernel
    const bool bnx = !last && L.bn && sa.seg < 0 && bnx_fits(m, true, batch, L.n_out, L.n_in);
    GemmArgs g = gemm_args(hin, L.n_in, params + L.offW, L.n_out, outp, L.n_out, batch, L.n_out, L.n_in,
                           last ? (fuse_ce ? EPI_BIAS_SOFTMAX_CE : EPI_BIAS) : (L.bn ? (bnx ? EPI_BIAS_RELU_BNX : EPI_BIAS_RELU_STATS) : EPI_BIAS_RELU));
    g.bias = params + L.offb;
    g.part = part;
    if (m->compute_bf16 == 2 && !last) g.amax_zero = m->amax + (size_t)l * kAmaxSlots * kAmaxStride;  // the backward pass of this step folds max |dz_l| into it
    if (bnx) {
      g.xc_gran = m->xc_gran + m->xc_gran_off[0][l]; g.xc_ctrl = m->xc_ctrl + m->xc_ctrl_off[0][l]; g.xc_err = m->xc_err; g.xc_rt_max = m->xc_rt_max;
      g.Bstat = xc_nowait() ? -bstat : bstat;
      g.h_out = ws + L.offH;
      g.gamma = params + L.offg; g.beta = params + L.offbe;
      g.mmean_w = bnstate + L.offmm; g.mvar_w = bnstate + L.offmv; g.save_w = ws + L.offMean;
      g.drop = drop_for_layer(m, l, dropout);
    }
    if (fuse_ce) {
      g.y = y_onehot;
      g.inv_batch = inv_batch;
      g.prob = probs ? probs : (ws + m->offProb);
      g.dz = ws + m->offDzLast;
      g.loss_rows = loss_rows;
      g.correct_rows = correct_rows;
    }
    set_arith(g, m, OP_ACT, OP_WEIGHT);
    g.lds_min_tiles = m->lds_min_tiles;
    if (LP_ON) {
      rc = launch_gemm(0, 1, g, st);
      if (rc != LIPASR_OK) return rc;
      if (sa.seg >= 0 && !last && L.bn) {  // synchronized BatchNorm: [2][row tiles][N] -> [2][N] before the exchange
        hipLaunchKernelGGL(part_reduce_kernel, dim3((L.n_out + 255) / 256), dim3(256), 0, st, part,
                           gemm_row_tiles(0, 1, g), L.n_out);
        LP_LAUNCH_CHECK();
        ++g_k2_launches[K2_PART_REDUCE];
      }
    }
    if (!last && L.bn) ++cur;  // exchange point: the partial sums of a, a^2 are complete
    if (!last && L.offH != L.offA && LP_ON && !bnx) {
      BnFwdArgs b;
      memset(&b, 0, sizeof(b));
      b.a = ws + L.offA; b.h = ws + L.offH; b.B = batch; b.N = L.n_out; b.has_bn = L.bn ? 1 : 0;
      b.Bstat = bstat;
      b.part = part;
      b.n_tiles = sa.seg >= 0 ? 1 : gemm_row_tiles(0, 1, g);
      if (L.bn) {
        b.gamma = params + L.offg; b.beta = params + L.offbe;
        b.mmean = bnstate + L.offmm; b.mvar = bnstate + L.offmv;
        b.save_mean = ws + L.offMean;
      }
      b.drop = drop_for_layer(m, l, dropout);
      const dim3 grid((L.n_out + 127) / 128, (batch + kApplyRows - 1) / kApplyRows);
      hipLaunchKernelGGL(bn_apply_fwd_kernel, grid, apply_block, 0, st, b);
      LP_LAUNCH_CHECK();
      ++g_k2_launches[b.has_bn ? K2_BN_FWD : K2_DROPOUT_FWD];
    }
    hin = (!last && L.offH != L.offA) ? (ws + L.offH) : outp;
  }
  // ---- loss and gradient at the logits (already done by the last GEMM's epilogue for <= 32 classes)
  if (C > 32 && LP_ON) {
    hipLaunchKernelGGL(softmax_ce_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, ws + m->offLogits, y_onehot, batch,
                       C, inv_batch, probs ? probs : (ws + m->offProb), ws + m->offDzLast, loss_rows, correct_rows,
                       (float*)nullptr);
    LP_LAUNCH_CHECK();
    ++g_k2_launches[K2_SOFTMAX_CE];
  }

  // ---- backward.  The dX chain runs first, layer by layer (dX GEMM fused with the dropout backward and the
  // BatchNorm column sums, then the BatchNorm/ReLU backward apply), keeping every layer's pre-activation gradient;
  // all weight gradients then come from ONE grouped launch.
  float* tmp = ws + m->offG0;
  for (int l = Lc - 1; l >= 1; --l) {
    const MlpLayer& L = m->L[l];
    const MlpLayer& P = m->L[l - 1];
    const float* gin = (l == Lc - 1) ? (ws + m->offDzLast) : (ws + L.offDz);
    // dh_prev[B][n_in] = gin[B][n_out] * W^T
    const bool bnx = P.bn && sa.seg < 0 && bnx_fits(m, false, batch, L.n_in, L.n_out);
    float* out1 = (P.bn && !bnx) ? tmp : (ws + P.offDz);
    GemmArgs gx = gemm_args(gin, L.n_out, params + L.offW, L.n_out, out1, L.n_in, batch, L.n_in, L.n_out,
                            P.bn ? (bnx ? EPI_DH_BNX : EPI_DH_STATS) : EPI_DZ_NOBN);
    gx.aux = ws + P.offA;
    gx.drop = drop_for_layer(m, l - 1, dropout);
    gx.part = part;
    if (P.bn) gx.save_mean = ws + P.offMean;
    if (bnx) {
      gx.xc_gran = m->xc_gran + m->xc_gran_off[1][l - 1]; gx.xc_ctrl = m->xc_ctrl + m->xc_ctrl_off[1][l - 1]; gx.xc_err = m->xc_err;
      gx.xc_rt_max = m->xc_rt_max;
      gx.Bstat = xc_nowait() ? -bstat : bstat; gx.grad_scale = sa.grad_scale;
      gx.gamma = params + P.offg;
      gx.dgamma = grads + P.offg; gx.dbeta = grads + P.offbe;
    }
    set_arith(gx, m, OP_GRAD, OP_WEIGHT, inv_batch);
    // arithmetic mode 2: the size of a gradient is not known beforehand (BatchNorm's rstd can amplify it 30-fold per layer in an
    // untrained network): whoever writes dz_l folds max |dz_l| into amax[l], whoever multiplies with dz_l derives its scale from it
    const bool dyn = m->compute_bf16 == 2;
    if (dyn && l < Lc - 1 && L.bn) gx.sa_dyn = m->amax + (size_t)l * kAmaxSlots * kAmaxStride;
    if (dyn && P.bn) gx.amax_out = m->amax + (size_t)(l - 1) * kAmaxSlots * kAmaxStride;
    gx.lds_min_tiles = m->lds_min_tiles;
    if (LP_ON) {
      rc = launch_gemm(0, 0, gx, st);
      if (rc != LIPASR_OK) return rc;
      if (sa.seg >= 0 && P.bn) {
        hipLaunchKernelGGL(part_reduce_kernel, dim3((P.n_out + 255) / 256), dim3(256), 0, st, part,
                           gemm_row_tiles(0, 0, gx), P.n_out);
        LP_LAUNCH_CHECK();
        ++g_k2_launches[K2_PART_REDUCE];
      }
    }
    if (P.bn) ++cur;  // exchange point: the partial sums of g, g xhat are complete
    if (P.bn && LP_ON && !bnx) {
      BnBwdArgs b;
      memset(&b, 0, sizeof(b));
      b.g = tmp; b.a = ws + P.offA; b.dz = ws + P.offDz; b.B = batch; b.N = P.n_out;
      b.Bstat = bstat; b.grad_scale = sa.grad_scale;
      b.part = part;
      b.n_tiles = sa.seg >= 0 ? 1 : gemm_row_tiles(0, 0, gx);
      b.gamma = params + P.offg; b.save_mean = ws + P.offMean;
      b.dgamma = grads + P.offg; b.dbeta = grads + P.offbe;
      b.amax_out = dyn ? m->amax + (size_t)(l - 1) * kAmaxSlots * kAmaxStride : nullptr;
      const dim3 grid((P.n_out + 127) / 128, (batch + kApplyRows - 1) / kApplyRows);
      hipLaunchKernelGGL(bn_apply_bwd_kernel, grid, apply_block, 0, st, b);
      LP_LAUNCH_CHECK();
      ++g_k2_launches[K2_BN_BWD];
    }
  }
  // [dW ; db] = [lin ; 1]^T[n_in+1][B] * gin[B][n_out] for every layer: the all-ones row yields the bias gradient
  GemmArgs gw[LIPASR_MAX_LAYERS];
  for (int l = 0; l < Lc; ++l) {
    const MlpLayer& L = m->L[l];
    const float* lin = (l == 0) ? x : (ws + m->L[l - 1].offH);
    const float* gin = (l == Lc - 1) ? (ws + m->offDzLast) : (ws + L.offDz);
    gw[l] = gemm_args(lin, L.n_in, gin, L.n_out, grads + L.offW, L.n_out, L.n_in + 1, L.n_out, batch, EPI_STORE);
    gw[l].ones_row = 1;
    gw[l].extra_out = grads + L.offb;
    set_arith(gw[l], m, OP_ACT, OP_GRAD, inv_batch);
    if (m->compute_bf16 == 2 && l < Lc - 1 && L.bn) gw[l].sb_dyn = m->amax + (size_t)l * kAmaxSlots * kAmaxStride;
  }
  if (!LP_ON) return LIPASR_OK;
#undef LP_ON
  if (dw_mode == 0 || Lc == 1) return launch_gemm_group_tn(gw, Lc, st);
  rc = launch_gemm_group_tn(gw + 1, Lc - 1, st);
  if (rc != LIPASR_OK || dw_mode == 2) return rc;
  return launch_gemm(1, 1, gw[0], st);
}

int lipasr_mlp_train_fwd_bwd(lipasr_mlp_t m, const float* params, float* bnstate, const float* x, const float* y_onehot,
                             int batch, float inv_batch, const lipasr_dropout_cfg* dropout, float* grads,
                             float* loss_rows, float* correct_rows, float* probs, lipasr_stream_t stream) {
  return train_fwd_bwd_impl(m, params, bnstate, x, y_onehot, batch, inv_batch, dropout, grads, loss_rows, correct_rows, probs,
                            stream, gemm_knobs().split_dw0 ? 1 : 0);
}

int lipasr_mlp_train_fwd_bwd_head(lipasr_mlp_t m, const float* params, float* bnstate, const float* x, const float* y_onehot,
                                  int batch, float inv_batch, const lipasr_dropout_cfg* dropout, float* grads,
                                  float* loss_rows, float* correct_rows, float* probs, lipasr_stream_t stream) {
  return train_fwd_bwd_impl(m, params, bnstate, x, y_onehot, batch, inv_batch, dropout, grads, loss_rows, correct_rows, probs,
                            stream, 2);
}

int lipasr_mlp_train_dw0(lipasr_mlp_t m, const float* x, int batch, float* grads, lipasr_stream_t stream) {
  int rc = check_batch("lipasr_mlp_train_dw0", m, batch);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(x && grads, "lipasr_mlp_train_dw0: null argument");
  if (m->n_layers == 1) return LIPASR_OK;  // a one-layer plan's head already holds every gradient
  const MlpLayer& L = m->L[0];
  GemmArgs g = gemm_args(x, L.n_in, m->ws + L.offDz, L.n_out, grads + L.offW, L.n_out, L.n_in + 1, L.n_out, batch, EPI_STORE);
  g.ones_row = 1;
  g.extra_out = grads + L.offb;
  set_arith(g, m, OP_ACT, OP_GRAD, m->last_inv_batch);
  if (m->compute_bf16 == 2 && L.bn) g.sb_dyn = m->amax;
  return launch_gemm(1, 1, g, S(stream));
}

int lipasr_mlp_train_segments(lipasr_mlp_t m, int* n_segments) {
  LP_CHECK_ARG(m && n_segments, "lipasr_mlp_train_segments: null argument");
  int n = 1;
  for (int l = 0; l + 1 < m->n_layers; ++l)
    if (m->L[l].bn) n += 2;  // one exchange in the forward pass, one in the backward pass
  *n_segments = n;
  return LIPASR_OK;
}

// floats of the partials buffer to SUM-all-reduce after segment `seg` (0 after the last one)
int lipasr_mlp_train_segment_exchange(lipasr_mlp_t m, int batch, int seg, size_t* floats) {
  int rc = check_batch("lipasr_mlp_train_segment_exchange", m, batch);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(floats != nullptr && seg >= 0, "lipasr_mlp_train_segment_exchange: bad argument");
  *floats = 0;
  int cur = 0;
  for (int l = 0; l + 1 < m->n_layers; ++l)  // forward: layer l's GEMM closes a segment if layer l has BatchNorm
    if (m->L[l].bn) {
      if (cur == seg) { *floats = 2 * (size_t)m->L[l].n_out; return LIPASR_OK; }  // reduced to [2][N] by part_reduce_kernel
      ++cur;
    }
  for (int l = m->n_layers - 1; l >= 1; --l)  // backward: the dX GEMM into layer l-1 closes one if layer l-1 has BatchNorm
    if (m->L[l - 1].bn) {
      if (cur == seg) { *floats = 2 * (size_t)m->L[l - 1].n_out; return LIPASR_OK; }
      ++cur;
    }
  return LIPASR_OK;
}

int lipasr_mlp_part_floats(lipasr_mlp_t m, size_t* floats) {
  LP_CHECK_ARG(m && floats, "lipasr_mlp_part_floats: null argument");
  *floats = 2 * (size_t)((m->max_batch + 31) / 32) * m->max_width;
  return LIPASR_OK;
}

int lipasr_mlp_train_segment(lipasr_mlp_t m, int seg, const float* params, float* bnstate, const float* x, const float* y_onehot,
                             int batch, float inv_batch, const lipasr_dropout_cfg* dropout, float* grads, float* loss_rows,
                             float* correct_rows, float* probs, float* part, int stat_batch, float stat_grad_scale,
                             lipasr_stream_t stream) {
  LP_CHECK_ARG(m != nullptr && part != nullptr, "lipasr_mlp_train_segment: null argument");
  int n = 0;
  (void)lipasr_mlp_train_segments(m, &n);
  LP_CHECK_ARG(seg >= 0 && seg < n, "lipasr_mlp_train_segment: segment %d outside [0, %d)", seg, n);
  LP_CHECK_ARG(stat_batch >= batch && stat_grad_scale > 0.0f, "lipasr_mlp_train_segment: stat_batch=%d (< batch %d) or scale %g", stat_batch,
               batch, (double)stat_grad_scale);
  SegArgs sa;
  sa.seg = seg; sa.part_ext = part; sa.stat_batch = stat_batch; sa.grad_scale = stat_grad_scale;
  return train_fwd_bwd_impl(m, params, bnstate, x, y_onehot, batch, inv_batch, dropout, grads, loss_rows, correct_rows, probs,
                            stream, 0, sa);
}

int lipasr_mlp_grad_split(lipasr_mlp_t m, size_t* late_floats) {
  LP_CHECK_ARG(m && late_floats, "lipasr_mlp_grad_split: null argument");
  // [W0 | b0] come from lipasr_mlp_train_dw0; what follows in the flat layout (gamma0, beta0, layers 1..) is final after the head
  const MlpLayer& L = m->L[0];
  *late_floats = (m->n_layers == 1) ? 0 : (L.bn ? L.offg : m->L[1].offW);
  return LIPASR_OK;
}

int lipasr_mlp_predict(lipasr_mlp_t m, const float* params, const float* bnstate, const float* x, int batch,
                       float* probs, float* logits, lipasr_stream_t stream) {
  int rc = check_batch("lipasr_mlp_predict", m, batch);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(params && x && (probs || logits), "lipasr_mlp_predict: null argument");
  LP_CHECK_ARG(m->n_state == 0 || bnstate, "lipasr_mlp_predict: bnstate is null");
  float* lg = logits ? logits : (m->ws + m->offLogits);
  rc = forward_infer(m, params, bnstate, x, batch, false, lg, S(stream));
  if (rc != LIPASR_OK) return rc;
  if (probs) {
    const int C = m->L[m->n_layers - 1].n_out;
    hipLaunchKernelGGL(softmax_ce_kernel, dim3((batch + 255) / 256), dim3(256), 0, S(stream), lg, (const float*)nullptr,
                       batch, C, 0.0f, probs, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr);
    LP_LAUNCH_CHECK();
    ++g_k2_launches[K2_SOFTMAX_CE];
  }
  return LIPASR_OK;
}

int lipasr_mlp_own_labels(lipasr_mlp_t m, const float* params, const float* bnstate, const float* x, int batch,
                          float* y_onehot_out, lipasr_stream_t stream) {
  int rc = check_batch("lipasr_mlp_own_labels", m, batch);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(params && x && y_onehot_out, "lipasr_mlp_own_labels: null argument");
  LP_CHECK_ARG(m->n_state == 0 || bnstate, "lipasr_mlp_own_labels: bnstate is null");
  float* lg = m->ws + m->offLogits;
  rc = forward_infer(m, params, bnstate, x, batch, false, lg, S(stream));
  if (rc != LIPASR_OK) return rc;
  const int C = m->L[m->n_layers - 1].n_out;
  hipLaunchKernelGGL(softmax_ce_kernel, dim3((batch + 255) / 256), dim3(256), 0, S(stream), lg, (const float*)nullptr,
                     batch, C, 0.0f, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr, y_onehot_out);
  LP_LAUNCH_CHECK();
  ++g_k2_launches[K2_SOFTMAX_CE];
  return LIPASR_OK;
}

static int attack_common(lipasr_mlp_t m, const float* params, const float* bnstate, const float* x_eval,
                         const float* y_onehot, int batch, float* dx, float* x_adv, const float* x0, float alpha,
                         float eps, hipStream_t st) {
  float* lg = m->ws + m->offLogits;
  bool fused = false;
  int rc = forward_infer(m, params, bnstate, x_eval, batch, true, lg, st, y_onehot, &fused);
  if (rc != LIPASR_OK) return rc;
  if (!fused) {
    const int C = m->L[m->n_layers - 1].n_out;
    hipLaunchKernelGGL(softmax_ce_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, lg, y_onehot, batch, C,
                       1.0f / (float)batch, m->ws + m->offProb, m->ws + m->offDzLast, (float*)nullptr, (float*)nullptr,
                       (float*)nullptr);
    LP_LAUNCH_CHECK();
    ++g_k2_launches[K2_SOFTMAX_CE];
  }
  return backward_infer(m, params, bnstate, batch, dx, x_adv, x0, alpha, eps, st, 1.0f / (float)batch);
}

int lipasr_mlp_input_grad(lipasr_mlp_t m, const float* params, const float* bnstate, const float* x,
                          const float* y_onehot, int batch, float* dx, lipasr_stream_t stream) {
  int rc = check_batch("lipasr_mlp_input_grad", m, batch);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(params && x && y_onehot && dx, "lipasr_mlp_input_grad: null argument");
  LP_CHECK_ARG(m->n_state == 0 || bnstate, "lipasr_mlp_input_grad: bnstate is null");
  return attack_common(m, params, bnstate, x, y_onehot, batch, dx, nullptr, nullptr, 0.0f, 0.0f, S(stream));
}

int lipasr_mlp_attack_step(lipasr_mlp_t m, const float* params, const float* bnstate, float* x_adv, const float* x0,
                           const float* y_onehot, int batch, float alpha, float eps, lipasr_stream_t stream) {
  int rc = check_batch("lipasr_mlp_attack_step", m, batch);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(params && x_adv && x0 && y_onehot, "lipasr_mlp_attack_step: null argument");
  LP_CHECK_ARG(m->n_state == 0 || bnstate, "lipasr_mlp_attack_step: bnstate is null");
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
  rc = check_batch("lipasr_mlp_attack_step_lp", m, batch);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(params && x_adv && x0 && y_onehot, "lipasr_mlp_attack_step_lp: null argument");
  LP_CHECK_ARG(m->n_state == 0 || bnstate, "lipasr_mlp_attack_step_lp: bnstate is null");
  LP_CHECK_ARG(eps >= 0.0f && !(alpha != alpha), "lipasr_mlp_attack_step_lp: eps=%g alpha=%g", (double)eps, (double)alpha);
  // backward_infer writes layer n-1's input gradient into G0, then alternates: at layer 0 it reads G[(n-2) % 2]
  float* g = m->ws + (((m->n_layers - 1) & 1) ? m->offG1 : m->offG0);
  rc = attack_common(m, params, bnstate, x_adv, y_onehot, batch, g, nullptr, nullptr, 0.0f, 0.0f, S(stream));
  if (rc != LIPASR_OK) return rc;
  return lp_step_launch(x_adv, x0, g, batch, m->L[0].n_in, code, alpha, eps, S(stream));
}

int lipasr_mlp_output_vjp(lipasr_mlp_t m, const float* params, const float* bnstate, const float* x, const float* v,
                          int on_logits, int batch, float* probs_out, float* dx, lipasr_stream_t stream) {
  int rc = check_batch("lipasr_mlp_output_vjp", m, batch);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(params && x && v && dx, "lipasr_mlp_output_vjp: null argument");
  LP_CHECK_ARG(m->n_state == 0 || bnstate, "lipasr_mlp_output_vjp: bnstate is null");
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
  int rc = check_batch("lipasr_mlp_jacobian", m, batch);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(params && x && jac, "lipasr_mlp_jacobian: null argument");
  LP_CHECK_ARG(m->n_state == 0 || bnstate, "lipasr_mlp_jacobian: bnstate is null");
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
