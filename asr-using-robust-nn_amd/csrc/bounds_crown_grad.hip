// CROWN-IBP certified training (lipasr/bounds.py, CrownIBPCrossentropy): the backward pass of the relaxation of bounds.hip with
// respect to the parameters.  DESIGN.md, "CROWN-IBP certified training", derives every line below.  Per row b, from what ONE
// lipasr_mlp_bounds call wrote (margin_ibp, margin_crown and the boxes layer_lo / layer_hi), under norm inf:
//
//   mixed[b][k] = (1 - beta) margin_ibp[b][k] + beta margin_crown[b][k]
//   u[b][k] = -mixed[b][k] (k != y_b), u[b][y_b] = 0      loss_rows[b] = logsumexp_k u[b][k]
//   grads = scale_old grads + scale_new d(sum_b loss_rows[b]) / d params
//
// margin_crown reaches the parameters along two roads: the chain Lambda_l -> nu_l -> Lambda_{l-1} (products with W, b, s, t), and the
// pre-activation boxes that set the slope and the intercept of every unstable neuron's upper line.  The first road is swept here
// over the M = batch x classes rows; the second one ends in a gradient on the z boxes (inj_lo, inj_hi) that the sweep of
// bounds_grad.hip takes on its way down (bg_run_device with a BgMixIn).  With g[m] = d loss / d margin_crown[m] = -beta softmax(u):
//
//   cg_soft_kernel     1 launch   a thread per row b: loss_rows and g
//   cg_relax_kernel    max(L-1,1) the chain again, every level kept: Lambda_{L-1} from W_L, and nu_l from Lambda_l and row m / C's box
//   bounds_back_kernel L - 1      (bounds.hip, bd_launch_product) Lambda_{l-1} = nu_l W_l^T
//   cg_adjoint_kernel  L - 1      ascending: G_nu = G_Lambda_{l-1} W_l + g b_l on the tile of bounds_tile.h (narrow operand by output
//                                 row, W k-major); for the first layer the operand g sel is formed as it is loaded from Lambda_0
//                                 and the input box (cg_operand).  Epilogue: sigma again from the box and the stored Lambda_l,
//                                 G_Lambda_l, and per element the term of ds and of the two injections
//   cg_wgrad_kernel    L - 1      partial products of dW_l = G_Lambda_{l-1}^T nu_l on the same tile (the same operand by reduction
//                                 row, nu k-major), k = M split over blockIdx.z in spans of kCgSpan rows: the pipeline's [begin, end)
//   cg_wreduce_kernel  L - 1      the partials in index order, the two scales, the store into grads
//   cg_colsum_kernel   L - 1      the column sums over M behind db_l, dgamma_l, dbeta_l: 8 columns and one span of kCgSpan rows a block, the
//                                 span through bg_sliced_sum (bounds_grad.h); one fp64 partial per span and column
//   cg_finish_kernel   L - 1      blocks [0, ceil(batch n_l / 256)): inj_lo, inj_hi [batch][n_l], a row's classes in index order, in fp64;
//                                 the blocks after them: the spans' partials in index order, db_l, dgamma_l, dbeta_l and their scales
//   cg_head_kernel     1          dW_L and db_L from G_Lambda_{L-1} and g
//
// then the sweep of bounds_grad.hip at (1, scale_new): 3 (L - 1) + 1 launches (2 for L = 1).  One call: 5 launches for L = 1,
// 10 (L - 1) + 3 for L >= 2.  beta = 0 makes exactly the launches of lipasr_mlp_bounds_grad and writes its bits.
// Every sum has one order that the shapes fix, as in bounds_grad.hip; no atomics; the host twin runs the same inline functions in
// those orders.  Constants of the derivative: the widening, every outward rounding, the running statistics, the slack, the
// (1 + 2^-40) factors of the upper line, the input box.  Conventions, torch's: p < 0 takes the upper line, the lower slope carries no
// gradient, Lambda_0 > 0 selects lo.  A NaN row makes its loss and the whole gradient NaN.
// Loads and stores are single floats, guarded: any width, any batch, any alignment.  Nothing allocates or synchronises.
#include "bounds_grad.h"
#include "bounds_tile.h"

// host and device must round alike
#pragma clang fp contract(off)

namespace lipasr {

long g_bounds_crown_grad_launches[9] = {};
enum { CG_SOFT = 0, CG_RELAX = 1, CG_PRODUCT = 2, CG_ADJOINT = 3, CG_WGRAD = 4, CG_WREDUCE = 5, CG_COLSUM = 6, CG_FINISH = 7, CG_HEAD = 8 };

constexpr int kCgSpan = 1024;  // rows of M one block of cg_wgrad_kernel walks: 32 chunks of 32

// loss_rows[b] and g[b][.] of one row; the orders are those of bg_head_kernel, which writes the same loss again
BD_HD void cg_soft_row(const float* mi, const float* mc, float beta, const int* y, int C, int b, float* g, float* loss_rows) {
  double p[32];
  const int yraw = y[b], yb = bg_label(yraw, C);
  const bool ok = yraw == yb;
  double mx = 0.0, sum = 0.0;
  for (int k = 0; k < C; ++k) {
    p[k] = k == yb ? 0.0 : bg_u(mi, mc, beta, (size_t)b * C + k);
    mx = p[k] > mx ? p[k] : mx;
  }
  for (int k = 0; k < C; ++k) {
    p[k] = ok ? bg_exp(p[k] - mx) : NAN;
    sum = sum + p[k];
  }
  loss_rows[b] = (float)(mx + bg_log(sum));
  for (int k = 0; k < C; ++k) g[(size_t)b * C + k] = k == yb ? 0.0f : (float)(-(double)beta * (p[k] / sum));
}

// Lambda_{L-1}[m][j] as bounds_head_kernel forms it
BD_HD float cg_top(const float* WL, int C, int j, int yb, int k) {
  return k == yb ? 0.0f : (float)((double)WL[(size_t)j * C + yb] - (double)WL[(size_t)j * C + k]);
}
// nu from Lambda, as bd_relax rounds it
BD_HD float cg_nu(float lam, double s, float zlo, float zhi) {
  bool upper;
  const double p = (double)lam * s;
  return (float)(p * bd_slope(p, zlo, zhi, upper));
}
// an element of G_Lambda_0 = g sel: never stored
BD_HD float cg_a0(float g, float lam0, float lo, float hi) { return g * (lam0 > 0.0f ? lo : hi); }
// element (m, i) of the operand A [M][K] of the adjoint and of the weight gradient: G_Lambda_{l-1} as stored, or (lam0 != null, the
// first layer) g sel formed here from Lambda_0 and the input box; 0 from row mend and from unit K on
BD_HD float cg_operand(const float* A, const float* lam0, const float* lo0, const float* hi0, const float* g, int C, int K, int m, int mend,
                       int i) {
  if (m >= mend || i >= K) return 0.0f;
  const size_t at = (size_t)m * K + i;
  if (!lam0) return A[at];
  const size_t bx = (size_t)(m / C) * K + i;
  return cg_a0(g[m], lam0[at], lo0[bx], hi0[bx]);
}

// one element of the adjoint's epilogue.  acc = (G_Lambda_{l-1} W_l)[m][j]; out: G_Lambda_l, the term of ds, the terms of the injections
BD_HD void cg_point(float acc, float g, float lam, const BdAff& a, float zlo, float zhi, float bias, float& gl, float& es, float& ilo,
                    float& ihi) {
  bool upper;
  const double p = (double)lam * a.s;
  const double sig = bd_slope(p, zlo, zhi, upper);
  const double gnu = (double)acc + (double)g * (double)bias;
  double gp = gnu * sig, il = 0.0, ih = 0.0;
  if (upper) {
    const double zl = zlo, zh = zhi, d = zh - zl, gz = (double)g * zl;
    gp = gp - gz * sig;
    const double gsig = gnu * p - gz * p;
    ih = gsig * (-zl) / (d * d);
    il = gsig * zh / (d * d) - (double)g * p * sig;
  }
  gl = (float)(gp * a.s + (double)g * a.t);
  es = (float)(gp * (double)lam);
  ilo = (float)il;
  ihi = (float)ih;
}

// one term of entry e of [dW_L | db_L] from row b.  top: G_Lambda_{L-1} [M][nh], or null (one layer: g sel, formed here)
BD_HD double cg_head_term(int e, int nh, int C, int b, int yb, const float* g, const float* top, const float* lam0, const float* lo0,
                          const float* hi0) {
  const int j = e < nh * C ? e / C : 0, c = e < nh * C ? e % C : e - nh * C;
  auto T = [&](int k) -> double {
    const size_t m = (size_t)b * C + k;
    if (e >= nh * C) return g[m];
    if (top) return top[m * nh + j];
    return cg_a0(g[m], lam0[m * nh + j], lo0[(size_t)b * nh + j], hi0[(size_t)b * nh + j]);
  };
  if (c != yb) return -T(c);
  double v = 0.0;
  for (int k = 0; k < C; ++k)
    if (k != yb) v = v + T(k);
  return v;
}

// ------------------------------------------------------------------------------------------------------------------- the plan
// the workspace, in floats from a 16-byte boundary
struct CgPlan : BdBoxes {
  size_t offG = 0, offLam[LIPASR_MAX_LAYERS] = {}, offNu[LIPASR_MAX_LAYERS] = {}, offGL[2] = {}, offEs = 0, offIlo = 0, offIhi = 0;
  size_t offInjLo = 0, offInjHi = 0, offPart = 0, offCol = 0, offIbp = 0;
  int spans = 1;
  size_t total = 0;
};

static CgPlan cg_plan(const BdShape& sh, int batch) {
  CgPlan p;
  static_cast<BdBoxes&>(p) = bd_boxes(sh, batch);
  const size_t B = batch, C = sh.n[sh.L], M = B * C;
  p.spans = (int)((M + kCgSpan - 1) / kCgSpan);
  size_t maxw = 0, maxprod = 0;
  for (int c = 1; c < sh.L; ++c) {
    maxw = std::max(maxw, (size_t)sh.n[c]);
    maxprod = std::max(maxprod, (size_t)sh.n[c - 1] * sh.n[c]);
  }
  size_t o = 0;
  p.offG = o; o = bd_align4(o + M);
  for (int c = 0; c < sh.L; ++c) {
    p.offLam[c] = o; o = bd_align4(o + M * sh.n[c]);
    if (c >= 1) { p.offNu[c] = o; o = bd_align4(o + M * sh.n[c]); }
  }
  for (int q = 0; q < 2; ++q) { p.offGL[q] = o; o = bd_align4(o + M * maxw); }
  p.offEs = o; o = bd_align4(o + M * maxw);
  p.offIlo = o; o = bd_align4(o + M * maxw);
  p.offIhi = o; o = bd_align4(o + M * maxw);
  if (sh.L > 1) {
    p.offInjLo = o; o = bd_align4(o + p.fam);
    p.offInjHi = o; o = bd_align4(o + p.fam);
  }
  p.offPart = o; o = bd_align4(o + (size_t)p.spans * maxprod);
  p.offCol = o; o = bd_align4(o + 2 * 3 * (size_t)p.spans * maxw);  // doubles: [spans][3][n]
  p.offIbp = o; o = o + bg_workspace_floats(sh, batch);
  p.total = o + 4;
  return p;
}

// -------------------------------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(kBdThreads) void cg_soft_kernel(const float* __restrict__ mi, const float* __restrict__ mc, float beta,
                                                             const int* __restrict__ y, int batch, int C, float* __restrict__ g,
                                                             float* __restrict__ loss_rows) {
  const int b = blockIdx.x * kBdThreads + threadIdx.x;
  if (b < batch) cg_soft_row(mi, mc, beta, y, C, b, g, loss_rows);
}

// an element (m, j) a thread.  WL != null: the top level, Lambda is formed and stored; zlo != null: nu is formed and stored
__global__ __launch_bounds__(kBdThreads) void cg_relax_kernel(const float* __restrict__ WL, const int* __restrict__ y, int M, int C, int N,
                                                              BdBn bn, const float* __restrict__ zlo, const float* __restrict__ zhi,
                                                              float* __restrict__ lam, float* __restrict__ nu) {
  const size_t at = (size_t)blockIdx.x * kBdThreads + threadIdx.x;
  if (at >= (size_t)M * N) return;
  const int m = (int)(at / N), j = (int)(at % N), b = m / C, k = m % C;
  float v;
  if (WL) {
    v = cg_top(WL, C, j, bg_label(y[b], C), k);
    lam[at] = v;
  } else {
    v = lam[at];
  }
  if (zlo) {
    const size_t bx = (size_t)b * N + j;
    nu[at] = cg_nu(v, bd_aff(bn, j).s, zlo[bx], zhi[bx]);
  }
}

// G_nu = A W + g b for rows m0 .. m0 + 31 (blockIdx.x) and columns n0 .. n0 + 127 (blockIdx.y), a wavefront per 32 columns.
// A = G_Lambda_{l-1} [M][K], or (lam0 != null) g sel formed from Lambda_0 and the input box.  W is [K][N].
__global__ __launch_bounds__(kBdThreads) void cg_adjoint_kernel(const float* __restrict__ A, const float* __restrict__ lam0,
                                                                const float* __restrict__ lo0, const float* __restrict__ hi0,
                                                                const float* __restrict__ g, const float* __restrict__ W,
                                                                const float* __restrict__ bias, BdBn bn, const float* __restrict__ zlo,
                                                                const float* __restrict__ zhi, const float* __restrict__ lam, int M, int C,
                                                                int K, int N, float* __restrict__ gl, float* __restrict__ es,
                                                                float* __restrict__ ilo, float* __restrict__ ihi) {
  __shared__ float as[kBtNarrow], wsm[kBtWideK];
  const BtThread t;
  const int m0 = blockIdx.x * 32, n0 = blockIdx.y * 128;
  bd_f32x16 acc = bt_zero();
  float areg[4], wreg[16];
  auto fetch = [&](int k0) {
    bt_narrow_each(t.tid, [&](int q, int row, int kk) { areg[q] = cg_operand(A, lam0, lo0, hi0, g, C, K, m0 + row, M, k0 + kk); });
    bt_wide_k_each(t.tid, [&](int q, int kk, int col) {
      const int k = k0 + kk, j = n0 + col;
      wreg[q] = (k < K && j < N) ? W[(size_t)k * N + j] : 0.0f;
    });
  };
  auto stage = [&] {
    bt_narrow_store(as, t.tid, areg);
    bt_wide_k_store(wsm, t.tid, wreg);
  };
  bt_pipeline(0, K, fetch, stage, [&](int s) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bt_narrow_by_row(as, t, s), bt_wide_k(wsm, t, s), acc, 0, 0, 0);
  });
  const int j = t.col(n0);
  if (j >= N) return;
  const BdAff a = bd_aff(bn, j);
  const float bj = bias[j];
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int m = t.row(m0, e);
    if (m >= M) continue;
    const size_t at = (size_t)m * N + j, bx = (size_t)(m / C) * N + j;
    float vg, vs, vl, vh;
    cg_point(acc[e], g[m], lam[at], a, zlo[bx], zhi[bx], bj, vg, vs, vl, vh);
    gl[at] = vg;
    if (bn.gamma) es[at] = vs;
    ilo[at] = vl;
    ihi[at] = vh;
  }
}

// part[z][i][j] = sum over the rows m of span z of A[m][i] nu[m][j]: rows i0 .. i0 + 31 (blockIdx.x), columns j0 .. j0 + 127
// (blockIdx.y), span z = blockIdx.z, a wavefront per 32 columns, the span in chunks of 32 rows.  A as in cg_adjoint_kernel.
__global__ __launch_bounds__(kBdThreads) void cg_wgrad_kernel(const float* __restrict__ A, const float* __restrict__ lam0,
                                                              const float* __restrict__ lo0, const float* __restrict__ hi0,
                                                              const float* __restrict__ g, const float* __restrict__ nu, int M, int C, int K,
                                                              int N, float* __restrict__ part) {
  __shared__ float as[kBtNarrow], ns[kBtWideK];
  const BtThread t;
  const int i0 = blockIdx.x * 32, j0 = blockIdx.y * 128;
  const int mbeg = blockIdx.z * kCgSpan, mend = min(M, mbeg + kCgSpan);
  bd_f32x16 acc = bt_zero();
  // a row past the span, a unit past K and a column past N read as 0
  float areg[4], nreg[16];
  auto fetch = [&](int r0) {
    bt_narrow_each(t.tid, [&](int q, int rr, int ii) { areg[q] = cg_operand(A, lam0, lo0, hi0, g, C, K, r0 + rr, mend, i0 + ii); });
    bt_wide_k_each(t.tid, [&](int q, int rr, int col) {
      const int m = r0 + rr, j = j0 + col;
      nreg[q] = (m < mend && j < N) ? nu[(size_t)m * N + j] : 0.0f;
    });
  };
  auto stage = [&] {
    bt_narrow_store(as, t.tid, areg);
    bt_wide_k_store(ns, t.tid, nreg);
  };
  bt_pipeline(mbeg, mend, fetch, stage, [&](int s) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bt_narrow_by_k(as, t, s), bt_wide_k(ns, t, s), acc, 0, 0, 0);
  });
  const int j = t.col(j0);
  if (j >= N) return;
  float* out = part + (size_t)blockIdx.z * K * N;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int i = t.row(i0, e);
    if (i < K) out[(size_t)i * N + j] = acc[e];
  }
}

// dW[e] from the spans' partials, in index order
__global__ __launch_bounds__(kBdThreads) void cg_wreduce_kernel(const float* __restrict__ part, int spans, size_t E, float scale_old,
                                                                float scale_new, float* __restrict__ dW) {
  const size_t e = (size_t)blockIdx.x * kBdThreads + threadIdx.x;
  if (e >= E) return;
  float v = part[e];
  for (int z = 1; z < spans; ++z) v = v + part[(size_t)z * E + e];
  dW[e] = bg_mix(dW[e], v, scale_old, scale_new);
}

// kBgCols columns of a hidden layer and one span of rows (blockIdx.y) a block: the span's part of sum_m g nu (db), sum_m es (ds) and
// sum_m g Lambda (dt), as col[span][0 .. 2][j]
__global__ __launch_bounds__(kBdThreads) void cg_colsum_kernel(const float* __restrict__ g, const float* __restrict__ nu,
                                                               const float* __restrict__ lam, const float* __restrict__ es, int bn, int M,
                                                               int N, double* __restrict__ col) {
  const int j = blockIdx.x * kBgCols + threadIdx.x % kBgCols;
  const int mbeg = blockIdx.y * kCgSpan, mend = min(M, mbeg + kCgSpan);
  bg_sliced_sum<3>(
      j < N, mbeg, mend,
      [&](int m, double* acc) {
        const size_t i = (size_t)m * N + j;
        const double gm = g[m];
        acc[0] = acc[0] + gm * (double)nu[i];
        if (bn) {
          acc[1] = acc[1] + (double)es[i];
          acc[2] = acc[2] + gm * (double)lam[i];
        }
      },
      [&](const double* tot) {
        double* out = col + (size_t)blockIdx.y * 3 * N;
        out[j] = tot[0];
        out[N + j] = tot[1];
        out[2 * N + j] = tot[2];
      });
}

// the spans' partials of column j in index order, then db and (BatchNorm) dgamma, dbeta
BD_HD void cg_column_finish(const double* col, int spans, int N, int j, const float* mmean, const float* mvar, float scale_old,
                            float scale_new, float* db, float* dgamma, float* dbeta) {
  double tb = col[j], ts = col[N + j], tt = col[2 * N + j];
  for (int z = 1; z < spans; ++z) {
    const double* p = col + (size_t)z * 3 * N;
    tb = tb + p[j];
    ts = ts + p[N + j];
    tt = tt + p[2 * N + j];
  }
  bg_column_store(j, tb, ts, tt, mmean, mvar, scale_old, scale_new, db, dgamma, dbeta);
}

// an element (b, j) a thread: the classes of row b in index order
BD_HD void cg_inject_point(const float* ilo, const float* ihi, int C, int N, int b, int j, float& lo, float& hi) {
  double sl = 0.0, sh = 0.0;
  for (int k = 0; k < C; ++k) {
    const size_t at = ((size_t)b * C + k) * N + j;
    sl = sl + (double)ilo[at];
    sh = sh + (double)ihi[at];
  }
  lo = (float)sl;
  hi = (float)sh;
}
__global__ __launch_bounds__(kBdThreads) void cg_finish_kernel(const float* __restrict__ ilo, const float* __restrict__ ihi, int batch, int C,
                                                               int N, float* __restrict__ inj_lo, float* __restrict__ inj_hi,
                                                               int inject_blocks, const double* __restrict__ col, int spans,
                                                               const float* __restrict__ mmean, const float* __restrict__ mvar,
                                                               float scale_old, float scale_new, float* __restrict__ db,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta) {
  if ((int)blockIdx.x >= inject_blocks) {
    const int j = ((int)blockIdx.x - inject_blocks) * kBdThreads + threadIdx.x;
    if (j < N) cg_column_finish(col, spans, N, j, mmean, mvar, scale_old, scale_new, db, dgamma, dbeta);
    return;
  }
  const size_t at = (size_t)blockIdx.x * kBdThreads + threadIdx.x;
  if (at >= (size_t)batch * N) return;
  float lo, hi;
  cg_inject_point(ilo, ihi, C, N, (int)(at / N), (int)(at % N), lo, hi);
  inj_lo[at] = lo;
  inj_hi[at] = hi;
}

// kBgCols entries of [dW_L | db_L] a block, the batch in 32 interleaved fp64 slices that meet in index order
__global__ __launch_bounds__(kBdThreads) void cg_head_kernel(const int* __restrict__ y, const float* __restrict__ g,
                                                             const float* __restrict__ top, const float* __restrict__ lam0,
                                                             const float* __restrict__ lo0, const float* __restrict__ hi0, int batch, int C,
                                                             int nh, float scale_old, float scale_new, float* __restrict__ dW,
                                                             float* __restrict__ db) {
  const int e = blockIdx.x * kBgCols + threadIdx.x % kBgCols;
  bg_sliced_sum<1>(
      e < nh * C + C, 0, batch,
      [&](int b, double* acc) { acc[0] = acc[0] + cg_head_term(e, nh, C, b, bg_label(y[b], C), g, top, lam0, lo0, hi0); },
      [&](const double* tot) { bg_head_store(e, nh, C, tot[0], scale_old, scale_new, dW, db); });
}

// ------------------------------------------------------------------------------------------------------------------ host twin
static void cg_host(const BdShape& sh, const CgPlan& pl, const float* params, const float* bnstate, const float* mi, const float* mc,
                    const float* layer_lo, const float* layer_hi, const int* y, int batch, float beta, float* ws, float scale_old,
                    float scale_new, float* grads, float* loss_rows) {
  const int L = sh.L, C = sh.n[L], M = batch * C;
  float* g = ws + pl.offG;
  for (int b = 0; b < batch; ++b) cg_soft_row(mi, mc, beta, y, C, b, g, loss_rows);
  // the chain, every level kept
  const float* WL = params + sh.offW[L - 1];
  std::vector<float> acc;
  for (int c = L - 1; c >= 0; --c) {
    const int N = sh.n[c];
    float* lam = ws + pl.offLam[c];
    const BdBn bn = c >= 1 ? bd_bn(sh, params, bnstate, c - 1) : BdBn{};
    for (int m = 0; m < M; ++m) {
      const int b = m / C, k = m % C;
      for (int j = 0; j < N; ++j) {
        const size_t at = (size_t)m * N + j;
        if (c == L - 1) lam[at] = cg_top(WL, C, j, bg_label(y[b], C), k);
        if (c >= 1) {
          const size_t bx = pl.z[c - 1] + (size_t)b * N + j;
          ws[pl.offNu[c] + at] = cg_nu(lam[at], bd_aff(bn, j).s, layer_lo[bx], layer_hi[bx]);
        }
      }
    }
    if (c == 0) break;
    const int Kp = sh.n[c], Np = sh.n[c - 1];
    const float* W = params + sh.offW[c - 1];
    const float* A = ws + pl.offNu[c];
    float* out = ws + pl.offLam[c - 1];
    for (int m = 0; m < M; ++m) {
      acc.assign(Np, 0.0f);
      for (int k = 0; k < Kp; ++k) {
        const float a = A[(size_t)m * Kp + k];
        for (int i = 0; i < Np; ++i) acc[i] = std::fmaf(a, W[(size_t)i * Kp + k], acc[i]);
      }
      for (int i = 0; i < Np; ++i) out[(size_t)m * Np + i] = acc[i];
    }
  }
  // the sweep, ascending
  const float* lam0 = ws + pl.offLam[0];
  int cur = 0;
  for (int c = 1; c < L; ++c) {
    const int K = sh.n[c - 1], N = sh.n[c];
    const bool first = c == 1;
    const float* A = ws + pl.offGL[cur];
    const float* W = params + sh.offW[c - 1];
    const float* bias = params + sh.offb[c - 1];
    const float* lam = ws + pl.offLam[c];
    const float* nu = ws + pl.offNu[c];
    float* gl = ws + pl.offGL[cur ^ 1];
    float* es = ws + pl.offEs;
    float* ilo = ws + pl.offIlo;
    float* ihi = ws + pl.offIhi;
    const BdBn bn = bd_bn(sh, params, bnstate, c - 1);
    auto a_of = [&](int m, int i) { return cg_operand(first ? nullptr : A, first ? lam0 : nullptr, layer_lo, layer_hi, g, C, K, m, M, i); };
    for (int m = 0; m < M; ++m) {
      acc.assign(N, 0.0f);
      for (int i = 0; i < K; ++i) {
        const float a = a_of(m, i);
        const float* wr = W + (size_t)i * N;
        for (int j = 0; j < N; ++j) acc[j] = std::fmaf(a, wr[j], acc[j]);
      }
      for (int j = 0; j < N; ++j) {
        const size_t at = (size_t)m * N + j, bx = pl.z[c - 1] + (size_t)(m / C) * N + j;
        float vs;
        cg_point(acc[j], g[m], lam[at], bd_aff(bn, j), layer_lo[bx], layer_hi[bx], bias[j], gl[at], vs, ilo[at], ihi[at]);
        if (bn.gamma) es[at] = vs;
      }
    }
    // dW: the spans' partials, then in index order
    for (int i = 0; i < K; ++i) {
      std::vector<float> tot(N, 0.0f);
      for (int z = 0; z < pl.spans; ++z) {
        acc.assign(N, 0.0f);
        const int mend = std::min(M, (z + 1) * kCgSpan);
        for (int m = z * kCgSpan; m < mend; ++m) {
          const float a = a_of(m, i);
          const float* nr = nu + (size_t)m * N;
          for (int j = 0; j < N; ++j) acc[j] = std::fmaf(a, nr[j], acc[j]);
        }
        for (int j = 0; j < N; ++j) tot[j] = z == 0 ? acc[j] : tot[j] + acc[j];
      }
      for (int j = 0; j < N; ++j) {
        float* out = grads + sh.offW[c - 1] + (size_t)i * N + j;
        *out = bg_mix(*out, tot[j], scale_old, scale_new);
      }
    }
    double* col = reinterpret_cast<double*>(ws + pl.offCol);
    for (int z = 0; z < pl.spans; ++z) {
      const int mbeg = z * kCgSpan, mend = std::min(M, mbeg + kCgSpan);
      double* out = col + (size_t)z * 3 * N;
      for (int j = 0; j < N; ++j) {
        out[j] = bg_sliced_sum_host(mbeg, mend, [&](int m) { return (double)g[m] * (double)nu[(size_t)m * N + j]; });
        out[N + j] = bn.gamma ? bg_sliced_sum_host(mbeg, mend, [&](int m) { return (double)es[(size_t)m * N + j]; }) : 0.0;
        out[2 * N + j] = bn.gamma ? bg_sliced_sum_host(mbeg, mend, [&](int m) { return (double)g[m] * (double)lam[(size_t)m * N + j]; }) : 0.0;
      }
    }
    for (int j = 0; j < N; ++j)
      cg_column_finish(col, pl.spans, N, j, bn.mmean, bn.mvar, scale_old, scale_new, grads + sh.offb[c - 1],
                       bn.gamma ? grads + sh.offg[c - 1] : nullptr, bn.gamma ? grads + sh.offbe[c - 1] : nullptr);
    for (int b = 0; b < batch; ++b)
      for (int j = 0; j < N; ++j) {
        const size_t at = pl.z[c - 1] + (size_t)b * N + j;
        cg_inject_point(ilo, ihi, C, N, b, j, ws[pl.offInjLo + at], ws[pl.offInjHi + at]);
      }
    cur ^= 1;
  }
  const int nh = sh.n[L - 1];
  const float* top = L > 1 ? ws + pl.offGL[cur] : nullptr;
  for (int e = 0; e < nh * C + C; ++e) {
    const double tot = bg_sliced_sum_host(0, batch, [&](int b) { return cg_head_term(e, nh, C, b, bg_label(y[b], C), g, top, lam0, layer_lo, layer_hi); });
    bg_head_store(e, nh, C, tot, scale_old, scale_new, grads + sh.offW[L - 1], grads + sh.offb[L - 1]);
  }
  const BgMixIn mix{mc, beta, L > 1 ? ws + pl.offInjLo : nullptr, L > 1 ? ws + pl.offInjHi : nullptr};
  bg_run_host(sh, params, bnstate, mi, layer_lo, layer_hi, y, batch, ws + pl.offIbp, 1.0f, scale_new, grads, loss_rows, &mix);
}

// --------------------------------------------------------------------------------------------------------------------- checks
static int cg_check(const char* fn, const BdShape& sh, const CgPlan& pl, const float* params, const float* bnstate, const float* mi,
                    const float* mc, const float* layer_lo, const float* layer_hi, const int* y, int batch, float beta, const float* ws,
                    size_t ws_floats, const float* grads, const float* loss_rows) {
  LP_CHECK_ARG(params && mi && mc && layer_lo && layer_hi && y && ws && grads && loss_rows, "%s: null argument", fn);
  LP_CHECK_ARG(sh.n_state == 0 || bnstate, "%s: bnstate is null", fn);
  LP_CHECK_ARG(beta >= 0.0f && beta <= 1.0f, "%s: beta = %g outside [0, 1]", fn, (double)beta);
  LP_CHECK_ARG(ws_floats >= pl.total, "%s: workspace of %zu floats; %zu are needed", fn, ws_floats, pl.total);
  const size_t B = batch, C = sh.n[sh.L];
  const BdSpan sp[] = {{params, sh.n_params * 4, false}, {bnstate, sh.n_state * 4, false}, {mi, B * C * 4, false}, {mc, B * C * 4, false},
                       {layer_lo, pl.fam * 4, false}, {layer_hi, pl.fam * 4, false}, {y, B * 4, false}, {ws, ws_floats * 4, true},
                       {grads, sh.n_params * 4, true}, {loss_rows, B * 4, true}};
  return bd_check_spans(fn, sp, sizeof(sp) / sizeof(sp[0]));
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

long lipasr_debug_bounds_crown_grad_launches(int kernel) {
  return (kernel >= 0 && kernel < 9) ? g_bounds_crown_grad_launches[kernel] : -1;
}

int lipasr_mlp_bounds_crown_grad_workspace(lipasr_mlp_t m, int batch, size_t* floats) {
  const char* fn = "lipasr_mlp_bounds_crown_grad_workspace";
  BdShape sh;
  return bd_workspace(fn, bd_shape_of(fn, m, &sh), sh, batch, floats, cg_plan);
}

int lipasr_mlp_bounds_crown_grad_workspace_host(int n_layers, const int* widths, int batch, size_t* floats) {
  const char* fn = "lipasr_mlp_bounds_crown_grad_workspace_host";
  BdShape sh;
  return bd_workspace(fn, bd_shape_from(fn, n_layers, widths, nullptr, &sh), sh, batch, floats, cg_plan);
}

int lipasr_mlp_bounds_crown_grad(lipasr_mlp_t m, const float* params, const float* bnstate, const float* margin_ibp,
                                 const float* margin_crown, const float* layer_lo, const float* layer_hi, const int* y, int batch, float beta,
                                 float* workspace, size_t workspace_floats, float scale_old, float scale_new, float* grads,
                                 float* loss_rows, lipasr_stream_t stream) {
  const char* fn = "lipasr_mlp_bounds_crown_grad";
  BdShape sh;
  if (int rc = bd_shape_of(fn, m, &sh)) return rc;
  if (int rc = bd_batch_check(fn, sh, batch)) return rc;
  const CgPlan pl = cg_plan(sh, batch);
  if (int rc = cg_check(fn, sh, pl, params, bnstate, margin_ibp, margin_crown, layer_lo, layer_hi, y, batch, beta, workspace, workspace_floats,
                        grads, loss_rows))
    return rc;
  DeviceGuard guard(m->ctx->device);
  hipStream_t st = S(stream);
  float* ws = bd_base(workspace);
  if (beta == 0.0f)
    return bg_run_device(sh, st, params, bnstate, margin_ibp, layer_lo, layer_hi, y, batch, ws + pl.offIbp, scale_old, scale_new, grads,
                         loss_rows, nullptr);
  const int L = sh.L, C = sh.n[L], M = batch * C;
  auto blocks = [](size_t n) { return dim3((unsigned)((n + kBdThreads - 1) / kBdThreads)); };
  float* g = ws + pl.offG;
  hipLaunchKernelGGL(cg_soft_kernel, blocks(batch), dim3(kBdThreads), 0, st, margin_ibp, margin_crown, beta, y, batch, C, g, loss_rows);
  LP_LAUNCH_CHECK();
  ++g_bounds_crown_grad_launches[CG_SOFT];
  for (int c = L - 1; c >= 0; --c) {
    const int N = sh.n[c];
    const bool top = c == L - 1;
    if (top || c >= 1) {
      hipLaunchKernelGGL(cg_relax_kernel, blocks((size_t)M * N), dim3(kBdThreads), 0, st, top ? params + sh.offW[L - 1] : nullptr, y, M, C, N,
                         c >= 1 ? bd_bn(sh, params, bnstate, c - 1) : BdBn{}, c >= 1 ? layer_lo + pl.z[c - 1] : nullptr, c >= 1 ? layer_hi + pl.z[c - 1] : nullptr, ws + pl.offLam[c],
                         c >= 1 ? ws + pl.offNu[c] : nullptr);
      LP_LAUNCH_CHECK();
      ++g_bounds_crown_grad_launches[CG_RELAX];
    }
    if (c == 0) break;
    if (int rc = bd_launch_product(st, ws + pl.offNu[c], params + sh.offW[c - 1], M, sh.n[c], sh.n[c - 1], C, ws + pl.offLam[c - 1])) return rc;
    ++g_bounds_crown_grad_launches[CG_PRODUCT];
  }
  const float* lam0 = ws + pl.offLam[0];
  int cur = 0;
  for (int c = 1; c < L; ++c) {
    const int K = sh.n[c - 1], N = sh.n[c];
    const bool first = c == 1;
    const float* A = first ? nullptr : ws + pl.offGL[cur];
    const float* l0 = first ? lam0 : nullptr;
    const BdBn bn = bd_bn(sh, params, bnstate, c - 1);
    hipLaunchKernelGGL(cg_adjoint_kernel, dim3((M + 31) / 32, (N + 127) / 128), dim3(kBdThreads), 0, st, A, l0, layer_lo, layer_hi, g,
                       params + sh.offW[c - 1], params + sh.offb[c - 1], bn, layer_lo + pl.z[c - 1], layer_hi + pl.z[c - 1],
                       ws + pl.offLam[c], M, C, K, N, ws + pl.offGL[cur ^ 1], ws + pl.offEs, ws + pl.offIlo, ws + pl.offIhi);
    LP_LAUNCH_CHECK();
    ++g_bounds_crown_grad_launches[CG_ADJOINT];
    hipLaunchKernelGGL(cg_wgrad_kernel, dim3((K + 31) / 32, (N + 127) / 128, pl.spans), dim3(kBdThreads), 0, st, A, l0, layer_lo, layer_hi, g,
                       ws + pl.offNu[c], M, C, K, N, ws + pl.offPart);
    LP_LAUNCH_CHECK();
    ++g_bounds_crown_grad_launches[CG_WGRAD];
    hipLaunchKernelGGL(cg_wreduce_kernel, blocks((size_t)K * N), dim3(kBdThreads), 0, st, ws + pl.offPart, pl.spans, (size_t)K * N, scale_old,
                       scale_new, grads + sh.offW[c - 1]);
    LP_LAUNCH_CHECK();
    ++g_bounds_crown_grad_launches[CG_WREDUCE];
    double* col = reinterpret_cast<double*>(ws + pl.offCol);
    hipLaunchKernelGGL(cg_colsum_kernel, dim3((N + kBgCols - 1) / kBgCols, pl.spans), dim3(kBdThreads), 0, st, g, ws + pl.offNu[c], ws + pl.offLam[c],
                       ws + pl.offEs, bn.gamma ? 1 : 0, M, N, col);
    LP_LAUNCH_CHECK();
    ++g_bounds_crown_grad_launches[CG_COLSUM];
    const unsigned inject_blocks = blocks((size_t)batch * N).x;
    hipLaunchKernelGGL(cg_finish_kernel, dim3(inject_blocks + (N + kBdThreads - 1) / kBdThreads), dim3(kBdThreads), 0, st, ws + pl.offIlo,
                       ws + pl.offIhi, batch, C, N, ws + pl.offInjLo + pl.z[c - 1], ws + pl.offInjHi + pl.z[c - 1], (int)inject_blocks, col,
                       pl.spans, bn.mmean, bn.mvar, scale_old, scale_new, grads + sh.offb[c - 1], bn.gamma ? grads + sh.offg[c - 1] : nullptr,
                       bn.gamma ? grads + sh.offbe[c - 1] : nullptr);
    LP_LAUNCH_CHECK();
    ++g_bounds_crown_grad_launches[CG_FINISH];
    cur ^= 1;
  }
  {
    const int nh = sh.n[L - 1];
    hipLaunchKernelGGL(cg_head_kernel, dim3((nh * C + C + kBgCols - 1) / kBgCols), dim3(kBdThreads), 0, st, y, g,
                       L > 1 ? ws + pl.offGL[cur] : nullptr, lam0, layer_lo, layer_hi, batch, C, nh, scale_old, scale_new,
                       grads + sh.offW[L - 1], grads + sh.offb[L - 1]);
    LP_LAUNCH_CHECK();
    ++g_bounds_crown_grad_launches[CG_HEAD];
  }
  const BgMixIn mix{margin_crown, beta, L > 1 ? ws + pl.offInjLo : nullptr, L > 1 ? ws + pl.offInjHi : nullptr};
  return bg_run_device(sh, st, params, bnstate, margin_ibp, layer_lo, layer_hi, y, batch, ws + pl.offIbp, 1.0f, scale_new, grads, loss_rows, &mix);
}

int lipasr_mlp_bounds_crown_grad_host(int n_layers, const int* widths, const int* bn, const float* params, const float* bnstate,
                                      const float* margin_ibp, const float* margin_crown, const float* layer_lo, const float* layer_hi,
                                      const int* y, int batch, float beta, float* workspace, size_t workspace_floats, float scale_old,
                                      float scale_new, float* grads, float* loss_rows) {
  const char* fn = "lipasr_mlp_bounds_crown_grad_host";
  BdShape sh;
  if (int rc = bd_shape_from(fn, n_layers, widths, bn, &sh)) return rc;
  if (int rc = bd_batch_check(fn, sh, batch)) return rc;
  const CgPlan pl = cg_plan(sh, batch);
  if (int rc = cg_check(fn, sh, pl, params, bnstate, margin_ibp, margin_crown, layer_lo, layer_hi, y, batch, beta, workspace, workspace_floats,
                        grads, loss_rows))
    return rc;
  float* ws = bd_base(workspace);
  if (beta == 0.0f)
    bg_run_host(sh, params, bnstate, margin_ibp, layer_lo, layer_hi, y, batch, ws + pl.offIbp, scale_old, scale_new, grads, loss_rows, nullptr);
  else
    cg_host(sh, pl, params, bnstate, margin_ibp, margin_crown, layer_lo, layer_hi, y, batch, beta, ws, scale_old, scale_new, grads, loss_rows);
  return LIPASR_OK;
}

}  // extern "C"
