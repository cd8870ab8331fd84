// The dense classifier's training step: the BatchNorm / dropout apply kernels and the partial-sum reduction of synchronized
// BatchNorm, and the step itself -- forward, dX chain, weight gradients -- whole, as head + first layer's gradient, or segment by
// segment.  Every GEMM goes through the launchers of gemm.hip (gemm.h); the plan is mlp.hip's.
#include "gemm.h"
#include <cstdlib>

namespace lipasr {

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
      o[e] = relu_mask_keep_nan(av[e], d);
      if (c.j + e < c.N) omax = fmaxf(omax, fabsf(o[e]));
    }
    st4(p.dz, ro, c, o);
  }
  }
  if (p.amax_out) amax_publish(p.amax_out, omax);
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

// arithmetic mode 2: the words max |dz_l| of the current step is folded into (kAmaxSlots of them, one per 64-byte line: gemm.h)
static unsigned* amax_slot(const lipasr_mlp* m, int l) { return m->amax + (size_t)l * kAmaxSlots * kAmaxStride; }

// the exchange epilogue's state of BatchNorm layer l (dir 0: forward, 1: backward) and the rows its statistics cover
static void set_exchange(GemmArgs& g, const lipasr_mlp* m, int dir, int l, int bstat) {
  g.xc_gran = m->xc_gran + m->xc_gran_off[dir][l];
  g.xc_ctrl = m->xc_ctrl + m->xc_ctrl_off[dir][l];
  g.xc_err = m->xc_err;
  g.xc_rt_max = m->xc_rt_max;
  g.Bstat = xc_nowait() ? -bstat : bstat;
}

// [dW ; db] of layer l = [lin ; 1]^T[n_in+1][B] * gin[B][n_out]: the all-ones row yields the bias gradient.  g0: the bound of the
// gradient at the logits the step ran with, dz_last: that gradient itself (the plan's own slot, or the caller's of
// lipasr_mlp_train_bwd).  The grouped launch of the step and lipasr_mlp_train_dw0 both take it from here.
static GemmArgs dw_args(const lipasr_mlp* m, int l, const float* x, float* grads, int batch, float g0, const float* dz_last) {
  const MlpLayer& L = m->L[l];
  const bool last = (l == m->n_layers - 1);
  const float* lin = (l == 0) ? x : (m->ws + m->L[l - 1].offH);
  const float* gin = last ? dz_last : (m->ws + L.offDz);
  GemmArgs g = gemm_args(lin, L.n_in, gin, L.n_out, grads + L.offW, L.n_out, L.n_in + 1, L.n_out, batch, EPI_STORE);
  g.ones_row = 1;
  g.extra_out = grads + L.offb;
  set_arith(g, m, OP_ACT, OP_GRAD, g0);
  if (m->compute_bf16 == 2 && L.bn) g.sb_dyn = amax_slot(m, l);  // (a last layer has no BatchNorm: its dz is (p - y) / B, scaled by g0)
  return g;
}

// ---------------------------------------------------------------------------------------------
// Segments (synchronized BatchNorm under data parallelism): the launch sequence is cut after every GEMM whose epilogue
// leaves BatchNorm column partial sums (forward: sums of a, a^2; backward: sums of g, g xhat), i.e. right before the
// apply kernel that consumes them.  exchange_points is the ONE list of those cuts, in launch order: forward, every hidden
// layer with BatchNorm; then backward, every l from the last layer down to 1 whose layer l - 1 has BatchNorm.  The number of
// segments, the floats to exchange after each and the step's own "does this launch belong to the wanted segment" read it.
// ---------------------------------------------------------------------------------------------
struct ExchangePoint {
  bool forward;
  int layer;  // the BatchNorm layer whose partial sums are complete here
  int width;  // its units: part_reduce_kernel leaves [2][width] to SUM-all-reduce
};
struct ExchangePoints {
  int n = 0;
  ExchangePoint p[2 * LIPASR_MAX_LAYERS];
};
static ExchangePoints exchange_points(const lipasr_mlp* m) {
  ExchangePoints e;
  for (int l = 0; l + 1 < m->n_layers; ++l)
    if (m->L[l].bn) e.p[e.n++] = ExchangePoint{true, l, m->L[l].n_out};
  for (int l = m->n_layers - 1; l >= 1; --l)
    if (m->L[l - 1].bn) e.p[e.n++] = ExchangePoint{false, l - 1, m->L[l - 1].n_out};
  return e;
}

// where the step stands in that list.  want < 0 runs everything; otherwise only the launches of segment `want`, and the caller
// SUM-all-reduces the partials (lipasr_mlp_train_segment_exchange) before it runs the next one.
struct SegCursor {
  ExchangePoints pts;
  int want;
  int cur = 0;  // the segment the next launch belongs to
  bool on() const { return want < 0 || want == cur; }
  // called after the GEMM that feeds BatchNorm layer `layer`: passes the exchange point the list has there, if it has one
  void pass(bool forward, int layer) {
    if (cur < pts.n && pts.p[cur].forward == forward && pts.p[cur].layer == layer) ++cur;
  }
};

// one training step's arguments, as its three passes share them
struct Step {
  lipasr_mlp* m;
  const float* params;
  float* bnstate;
  const float* x;
  const float* y_onehot;  // null (lipasr_mlp_train_fwd): the last epilogue writes logits and probabilities only
  const float* dz_last;   // the gradient at the logits the backward passes read: the plan's slot, or the caller's (lipasr_mlp_train_bwd)
  int batch;
  float inv_batch;        // the factor on p - y, and the bound of the gradient at the logits (lipasr_mlp_train_bwd: the caller's dz_bound)
  const lipasr_dropout_cfg* dropout;
  float* grads;
  float* loss_rows;
  float* correct_rows;
  float* probs;
  hipStream_t st;
  float* part;       // column partials: the plan's, or the caller's (a torch tensor it can hand to its collective) in segment mode
  int bstat;         // rows the BatchNorm statistics cover (the batch; synchronized BatchNorm: the global batch)
  float grad_scale;  // factor on dgamma / dbeta
  SegCursor seg;
  bool segmented() const { return seg.want >= 0; }
};

// synchronized BatchNorm: [2][row tiles][N] -> [2][N] before the exchange
static int reduce_partials(const Step& s, int n_tiles, int N) {
  hipLaunchKernelGGL(part_reduce_kernel, dim3((N + 255) / 256), dim3(256), 0, s.st, s.part, n_tiles, N);
  LP_LAUNCH_CHECK();
  ++g_k2_launches[K2_PART_REDUCE];
  return LIPASR_OK;
}

static int apply_fwd(const Step& s, int l, int n_tiles) {
  const lipasr_mlp* m = s.m;
  const MlpLayer& L = m->L[l];
  BnFwdArgs b;
  memset(&b, 0, sizeof(b));
  b.a = m->ws + L.offA; b.h = m->ws + L.offH; b.B = s.batch; b.N = L.n_out; b.has_bn = L.bn ? 1 : 0;
  b.Bstat = s.bstat;
  b.part = s.part;
  b.n_tiles = n_tiles;
  if (L.bn) {
    b.gamma = s.params + L.offg; b.beta = s.params + L.offbe;
    b.mmean = s.bnstate + L.offmm; b.mvar = s.bnstate + L.offmv;
    b.save_mean = m->ws + L.offMean;
  }
  b.drop = drop_for_layer(m, l, s.dropout);
  const dim3 grid((L.n_out + 127) / 128, (s.batch + kApplyRows - 1) / kApplyRows);
  hipLaunchKernelGGL(bn_apply_fwd_kernel, grid, dim3(256), 0, s.st, b);
  LP_LAUNCH_CHECK();
  ++g_k2_launches[b.has_bn ? K2_BN_FWD : K2_DROPOUT_FWD];
  return LIPASR_OK;
}

// l: the BatchNorm layer; its g = dh * dropout is in the first ping-pong buffer
static int apply_bwd(const Step& s, int l, int n_tiles) {
  const lipasr_mlp* m = s.m;
  const MlpLayer& P = m->L[l];
  BnBwdArgs b;
  memset(&b, 0, sizeof(b));
  b.g = m->ws + m->offG0; b.a = m->ws + P.offA; b.dz = m->ws + P.offDz; b.B = s.batch; b.N = P.n_out;
  b.Bstat = s.bstat; b.grad_scale = s.grad_scale;
  b.part = s.part;
  b.n_tiles = n_tiles;
  b.gamma = s.params + P.offg; b.save_mean = m->ws + P.offMean;
  b.dgamma = s.grads + P.offg; b.dbeta = s.grads + P.offbe;
  b.amax_out = m->compute_bf16 == 2 ? amax_slot(m, l) : nullptr;
  const dim3 grid((P.n_out + 127) / 128, (s.batch + kApplyRows - 1) / kApplyRows);
  hipLaunchKernelGGL(bn_apply_bwd_kernel, grid, dim3(256), 0, s.st, b);
  LP_LAUNCH_CHECK();
  ++g_k2_launches[K2_BN_BWD];
  return LIPASR_OK;
}

// ---- forward (training mode): GEMM (+bias, ReLU, column partials) -> BatchNorm/dropout apply; the last GEMM's epilogue gives
// softmax, loss and (p - y) / B
static int step_forward(Step& s) {
  const lipasr_mlp* m = s.m;
  float* ws = m->ws;
  const float* hin = s.x;
  for (int l = 0; l < m->n_layers; ++l) {
    const MlpLayer& L = m->L[l];
    const bool last = (l == m->n_layers - 1);
    float* outp = last ? (ws + m->offLogits) : (ws + L.offA);
    // BatchNorm inside this GEMM (exchange epilogue) where the whole grid can be resident; not with synchronized BatchNorm,
    // whose sums leave the device between the GEMM and the apply kernel
    const bool bnx = L.bn && !s.segmented() && bnx_fits(m, true, s.batch, L.n_out, L.n_in);
    GemmArgs g = gemm_args(hin, L.n_in, s.params + L.offW, L.n_out, outp, L.n_out, s.batch, L.n_out, L.n_in,
                           last ? EPI_BIAS_SOFTMAX_CE : (L.bn ? (bnx ? EPI_BIAS_RELU_BNX : EPI_BIAS_RELU_STATS) : EPI_BIAS_RELU));
    g.bias = s.params + L.offb;
    g.part = s.part;
    if (m->compute_bf16 == 2 && !last) g.amax_zero = amax_slot(m, l);  // the backward pass of this step folds max |dz_l| into it
    if (bnx) {
      set_exchange(g, m, 0, l, s.bstat);
      g.h_out = ws + L.offH;
      g.gamma = s.params + L.offg; g.beta = s.params + L.offbe;
      g.mmean_w = s.bnstate + L.offmm; g.mvar_w = s.bnstate + L.offmv; g.save_w = ws + L.offMean;
      g.drop = drop_for_layer(m, l, s.dropout);
    }
    if (last) {
      g.y = s.y_onehot;
      g.inv_batch = s.inv_batch;
      g.prob = s.probs ? s.probs : (ws + m->offProb);
      g.dz = ws + m->offDzLast;
      g.loss_rows = s.loss_rows;
      g.correct_rows = s.correct_rows;
    }
    set_arith(g, m, OP_ACT, OP_WEIGHT);
    g.lds_min_tiles = m->lds_min_tiles;
    if (s.seg.on()) {
      int rc = launch_gemm(0, 1, g, s.st);
      if (rc == LIPASR_OK && s.segmented() && L.bn) rc = reduce_partials(s, gemm_row_tiles(0, 1, g), L.n_out);
      if (rc != LIPASR_OK) return rc;
    }
    s.seg.pass(true, l);  // the partial sums of a, a^2 are complete
    const bool apply = !last && L.offH != L.offA;  // BatchNorm or dropout
    if (apply && s.seg.on() && !bnx) {
      int rc = apply_fwd(s, l, s.segmented() ? 1 : gemm_row_tiles(0, 1, g));
      if (rc != LIPASR_OK) return rc;
    }
    hin = apply ? (ws + L.offH) : outp;
  }
  return LIPASR_OK;
}

// ---- backward, the dX chain: layer by layer (dX GEMM fused with the dropout backward and the BatchNorm column sums, then the
// BatchNorm/ReLU backward apply), keeping every layer's pre-activation gradient for the weight gradients
static int step_dx_chain(Step& s) {
  const lipasr_mlp* m = s.m;
  float* ws = m->ws;
  const int Lc = m->n_layers;
  for (int l = Lc - 1; l >= 1; --l) {
    const MlpLayer& L = m->L[l];
    const MlpLayer& P = m->L[l - 1];
    const float* gin = (l == Lc - 1) ? s.dz_last : (ws + L.offDz);
    // dh_prev[B][n_in] = gin[B][n_out] * W^T
    const bool bnx = P.bn && !s.segmented() && bnx_fits(m, false, s.batch, L.n_in, L.n_out);
    float* out1 = (P.bn && !bnx) ? (ws + m->offG0) : (ws + P.offDz);
    GemmArgs gx = gemm_args(gin, L.n_out, s.params + L.offW, L.n_out, out1, L.n_in, s.batch, L.n_in, L.n_out,
                            P.bn ? (bnx ? EPI_DH_BNX : EPI_DH_STATS) : EPI_DZ_NOBN);
    gx.aux = ws + P.offA;
    gx.drop = drop_for_layer(m, l - 1, s.dropout);
    gx.part = s.part;
    if (P.bn) gx.save_mean = ws + P.offMean;
    if (bnx) {
      set_exchange(gx, m, 1, l - 1, s.bstat);
      gx.grad_scale = s.grad_scale;
      gx.gamma = s.params + P.offg;
      gx.dgamma = s.grads + P.offg; gx.dbeta = s.grads + P.offbe;
    }
    set_arith(gx, m, OP_GRAD, OP_WEIGHT, s.inv_batch);
    // arithmetic mode 2: the size of a gradient is not known beforehand (BatchNorm's rstd can amplify it 30-fold per layer in an
    // untrained network): whoever writes dz_l folds max |dz_l| into amax[l], whoever multiplies with dz_l derives its scale from it
    const bool dyn = m->compute_bf16 == 2;
    if (dyn && L.bn) gx.sa_dyn = amax_slot(m, l);
    if (dyn && P.bn) gx.amax_out = amax_slot(m, l - 1);
    gx.lds_min_tiles = m->lds_min_tiles;
    if (s.seg.on()) {
      int rc = launch_gemm(0, 0, gx, s.st);
      if (rc == LIPASR_OK && s.segmented() && P.bn) rc = reduce_partials(s, gemm_row_tiles(0, 0, gx), P.n_out);
      if (rc != LIPASR_OK) return rc;
    }
    s.seg.pass(false, l - 1);  // the partial sums of g, g xhat are complete
    if (P.bn && s.seg.on() && !bnx) {
      int rc = apply_bwd(s, l - 1, s.segmented() ? 1 : gemm_row_tiles(0, 0, gx));
      if (rc != LIPASR_OK) return rc;
    }
  }
  return LIPASR_OK;
}

// ---- backward, the weight gradients, after the last exchange point.  dw_mode 0: every layer's from ONE grouped launch; 1: the
// first layer's [dW; db] as its own launch after the grouped launch of the others (LDS-tiled 64x64 kernel when legal); 2: the
// first layer's left out (lipasr_mlp_train_dw0)
static int step_weight_grads(Step& s, int dw_mode) {
  if (!s.seg.on()) return LIPASR_OK;
  const int Lc = s.m->n_layers;
  GemmArgs gw[LIPASR_MAX_LAYERS];
  for (int l = 0; l < Lc; ++l) gw[l] = dw_args(s.m, l, s.x, s.grads, s.batch, s.inv_batch, s.dz_last);
  if (dw_mode == 0 || Lc == 1) return launch_gemm_group_tn(gw, Lc, s.st);
  int rc = launch_gemm_group_tn(gw + 1, Lc - 1, s.st);
  if (rc != LIPASR_OK || dw_mode == 2) return rc;
  return launch_gemm(1, 1, gw[0], s.st);
}

// synchronized BatchNorm's arguments: the segment to run (< 0: all), the caller-owned partials buffer, the rows the statistics
// cover (global batch) and the factor on dgamma / dbeta
struct SegArgs {
  int seg = -1;
  float* part_ext = nullptr;
  int stat_batch = 0;
  float grad_scale = 1.0f;
};

// the step's arguments as every entry point fills them; the caller sets what its passes do not need to null
static Step make_step(lipasr_mlp_t m, const float* params, float* bnstate, const float* x, const float* y_onehot, int batch,
                      float inv_batch, const lipasr_dropout_cfg* dropout, float* grads, float* loss_rows, float* correct_rows,
                      float* probs, lipasr_stream_t stream, const SegArgs& sa) {
  Step s;
  s.m = m; s.params = params; s.bnstate = bnstate; s.x = x; s.y_onehot = y_onehot;
  s.dz_last = m->ws + m->offDzLast;
  s.batch = batch; s.inv_batch = inv_batch; s.dropout = dropout;
  s.grads = grads; s.loss_rows = loss_rows; s.correct_rows = correct_rows; s.probs = probs;
  s.st = S(stream);
  s.part = sa.part_ext ? sa.part_ext : (m->ws + m->offPart);
  s.bstat = sa.stat_batch > 0 ? sa.stat_batch : batch;
  s.grad_scale = sa.grad_scale;
  s.seg.pts = exchange_points(m);
  s.seg.want = sa.seg;
  return s;
}

static int train_fwd_bwd_impl(lipasr_mlp_t m, const float* params, float* bnstate, const float* x, const float* y_onehot,
                              int batch, float inv_batch, const lipasr_dropout_cfg* dropout, float* grads,
                              float* loss_rows, float* correct_rows, float* probs, lipasr_stream_t stream, int dw_mode,
                              const SegArgs& sa = SegArgs()) {
  int rc = check_call("lipasr_mlp_train_fwd_bwd", m, batch, bnstate);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(params && x && y_onehot && grads, "lipasr_mlp_train_fwd_bwd: null argument");
  LP_CHECK_ARG(!dropout || (dropout->mode >= 0 && dropout->mode <= 2), "lipasr_mlp_train_fwd_bwd: dropout mode %d",
               dropout ? dropout->mode : 0);
  m->last_inv_batch = inv_batch;
  Step s = make_step(m, params, bnstate, x, y_onehot, batch, inv_batch, dropout, grads, loss_rows, correct_rows, probs, stream, sa);
  rc = step_forward(s);
  if (rc == LIPASR_OK) rc = step_dx_chain(s);
  if (rc == LIPASR_OK) rc = step_weight_grads(s, dw_mode);
  return rc;
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

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
  return launch_gemm(1, 1, dw_args(m, 0, x, grads, batch, m->last_inv_batch, m->ws + m->offDzLast), S(stream));
}

// The step with the loss gradient supplied from outside: the forward pass alone (the last epilogue runs without labels: logits and
// probabilities, no loss, no gradient), then the two backward passes reading the caller's gradient at the logits.
int lipasr_mlp_train_fwd(lipasr_mlp_t m, const float* params, float* bnstate, const float* x, int batch,
                         const lipasr_dropout_cfg* dropout, float* logits_out, lipasr_stream_t stream) {
  int rc = check_call("lipasr_mlp_train_fwd", m, batch, bnstate);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(params && x && logits_out, "lipasr_mlp_train_fwd: null argument");
  LP_CHECK_ARG(!dropout || (dropout->mode >= 0 && dropout->mode <= 2), "lipasr_mlp_train_fwd: dropout mode %d", dropout ? dropout->mode : 0);
  Step s = make_step(m, params, bnstate, x, nullptr, batch, 1.0f / (float)batch, dropout, nullptr, nullptr, nullptr, nullptr, stream,
                     SegArgs());
  rc = step_forward(s);
  if (rc != LIPASR_OK) return rc;
  const size_t n = (size_t)batch * m->L[m->n_layers - 1].n_out;
  LP_HIP(hipMemcpyAsync(logits_out, m->ws + m->offLogits, n * sizeof(float), hipMemcpyDeviceToDevice, S(stream)));
  return LIPASR_OK;
}

int lipasr_mlp_train_bwd(lipasr_mlp_t m, const float* params, const float* x, const float* dz, int batch, float dz_bound,
                         const lipasr_dropout_cfg* dropout, float* grads, lipasr_stream_t stream) {
  int rc = check_batch("lipasr_mlp_train_bwd", m, batch);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(params && x && dz && grads, "lipasr_mlp_train_bwd: null argument");
  LP_CHECK_ARG(!dropout || (dropout->mode >= 0 && dropout->mode <= 2), "lipasr_mlp_train_bwd: dropout mode %d", dropout ? dropout->mode : 0);
  LP_CHECK_ARG(dz_bound > 0.0f && dz_bound < INFINITY, "lipasr_mlp_train_bwd: dz_bound %g (a finite bound > 0 of max |dz|)", (double)dz_bound);
  m->last_inv_batch = dz_bound;
  Step s = make_step(m, params, nullptr, x, nullptr, batch, dz_bound, dropout, grads, nullptr, nullptr, nullptr, stream, SegArgs());
  s.dz_last = dz;
  rc = step_dx_chain(s);
  if (rc == LIPASR_OK) rc = step_weight_grads(s, gemm_knobs().split_dw0 ? 1 : 0);
  return rc;
}

int lipasr_mlp_train_segments(lipasr_mlp_t m, int* n_segments) {
  LP_CHECK_ARG(m && n_segments, "lipasr_mlp_train_segments: null argument");
  *n_segments = exchange_points(m).n + 1;
  return LIPASR_OK;
}

// floats of the partials buffer to SUM-all-reduce after segment `seg` (0 after the last one)
int lipasr_mlp_train_segment_exchange(lipasr_mlp_t m, int batch, int seg, size_t* floats) {
  int rc = check_batch("lipasr_mlp_train_segment_exchange", m, batch);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(floats != nullptr && seg >= 0, "lipasr_mlp_train_segment_exchange: bad argument");
  const ExchangePoints e = exchange_points(m);
  *floats = seg < e.n ? 2 * (size_t)e.p[seg].width : 0;  // reduced to [2][N] by part_reduce_kernel
  return LIPASR_OK;
}

int lipasr_mlp_part_floats(lipasr_mlp_t m, size_t* floats) {
  LP_CHECK_ARG(m && floats, "lipasr_mlp_part_floats: null argument");
  *floats = 2 * (size_t)part_row_tiles(m->max_batch) * m->max_width;
  return LIPASR_OK;
}

int lipasr_mlp_train_segment(lipasr_mlp_t m, int seg, const float* params, float* bnstate, const float* x, const float* y_onehot,
                             int batch, float inv_batch, const lipasr_dropout_cfg* dropout, float* grads, float* loss_rows,
                             float* correct_rows, float* probs, float* part, int stat_batch, float stat_grad_scale,
                             lipasr_stream_t stream) {
  LP_CHECK_ARG(m != nullptr && part != nullptr, "lipasr_mlp_train_segment: null argument");
  const int n = exchange_points(m).n + 1;
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

}  // extern "C"
