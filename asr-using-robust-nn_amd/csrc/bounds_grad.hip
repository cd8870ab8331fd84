// IBP certified training (lipasr/bounds.py, IBPCrossentropy): the backward pass of the interval bounds of bounds.hip with respect
// to the parameters.  DESIGN.md, "Certified training", derives every line below.  Per row b, from what ONE lipasr_mlp_bounds call
// wrote (margin_ibp and the boxes layer_lo / layer_hi), under norm inf:
//
//   u[b][k] = -margin_ibp[b][k] (k != y_b), u[b][y_b] = 0      loss_rows[b] = logsumexp_k u[b][k]
//   grads = scale_old grads + scale_new d(sum_b loss_rows[b]) / d params
//
//   bg_head_kernel     1 launch   a block per row: softmax of u, loss_rows, d loss / d u, the gradient into the last hidden box
//                                 through the difference rows W_L[y] - W_L[k] (lo where the difference is > 0, hi otherwise), and
//                                 the BatchNorm and ReLU gates of layer L - 1: (gc, gr) of that layer and what its column sums need
//   bg_head_dw_kernel  1          dW_L and db_L: 8 entries a block, the batch through bg_sliced_sum (bounds_grad.h): 32 interleaved
//                                 fp64 slices that meet in index order
//   bg_colsum_kernel   L - 1      db_l, dgamma_l, dbeta_l of a hidden layer: 8 columns a block, three such sums at once
//   bg_wgrad_kernel    L - 1      dW_l = c^T gc + sign(W_l) (r^T gr): both products on the tile of bounds_tile.h, the batch as the k
//                                 dimension (narrow operand by reduction row, two wide k-major operands), c and r formed from
//                                 lo / hi as they are staged; epilogue: the sign of W, the two scales, the store into grads
//   bg_back_kernel     L - 2      (g_c, g_r) = (gc W_l^T, gr |W_l|^T) from ONE read of W_l on the same tile (two narrow operands by
//                                 output row, W n-major); epilogue: g_lo, g_hi, layer l - 1's BatchNorm and ReLU gates, (gc, gr) of
//                                 layer l - 1 and what its column sums need
//
// Launches of one call with L layers: 2 for L = 1, 3 (L - 1) + 1 for L >= 2.  Every sum has one order that the shapes fix: the
// MFMA is an fmaf chain in ascending k, a column sum is 32 interleaved slices in ascending row order that meet in slice order.  No
// atomics: two calls give the same bits, and the host twin, which runs the same inline functions in those orders, gives the same
// values (a zero may differ in sign).  exp and log are written out in + * / below for that reason.  Conventions, torch's:
// relu'(0) = 0, d|w| / dw = 0 at 0, s >= 0 takes the branch that does not swap, a difference of 0 selects hi; the widening and the
// outward roundings of the forward pass are constants; the input box carries no gradient.  A row whose margins are NaN (or whose
// label is outside [0, classes)) makes its loss and the whole gradient NaN.
// Loads and stores are single floats, guarded: any width, any batch, any alignment.  Nothing allocates or synchronises.
// bounds_crown_grad.hip runs the same sweep through bg_run_device / bg_run_host with a BgMixIn (bounds.h): the margins mixed with
// margin_crown, the head weighted by 1 - beta, and a gradient on every z box added in bg_gate.  With a null BgMixIn the extra
// operands are null and every result is what it was without them.
#include "bounds_grad.h"
#include "bounds_tile.h"

// host and device must round alike
#pragma clang fp contract(off)

namespace lipasr {

long g_bounds_grad_launches[4] = {};
enum { BG_HEAD = 0, BG_WGRAD = 1, BG_BACK = 2, BG_COLSUM = 3 };

// the gradient (glo, ghi) on the box of h = s relu(z) + t becomes (gc, gr) = (g_zlo + g_zhi, g_zhi - g_zlo) on the box of z, and
// the terms of d loss / d s and d loss / d t.  A gate multiplies, so that a NaN stays.
// inj: (ilo, ihi), the gradient that reaches the z box by another road (the relaxation of bounds_crown_grad.hip), is added.
BD_HD void bg_gate(double glo, double ghi, double s, float zlo, float zhi, float& gc, float& gr, float& es, float& et, bool inj = false,
                   double ilo = 0.0, double ihi = 0.0) {
  const double alo = zlo > 0.0f ? (double)zlo : 0.0, ahi = zhi > 0.0f ? (double)zhi : 0.0;
  const double ml = zlo > 0.0f ? 1.0 : 0.0, mh = zhi > 0.0f ? 1.0 : 0.0;
  double gzlo, gzhi, ds;
  if (s >= 0.0) {
    gzlo = s * glo * ml;
    gzhi = s * ghi * mh;
    ds = glo * alo + ghi * ahi;
  } else {
    gzhi = s * glo * mh;
    gzlo = s * ghi * ml;
    ds = glo * ahi + ghi * alo;
  }
  if (inj) {
    gzlo = gzlo + ilo;
    gzhi = gzhi + ihi;
  }
  gc = (float)(gzlo + gzhi);
  gr = (float)(gzhi - gzlo);
  es = (float)ds;
  et = (float)(glo + ghi);
}

// one column j of a row's head: p[k] the softmax of u, wl = W_L[j][0 .. C).  ty = d loss / d W_L[j][y]
BD_HD void bg_head_column(const double* p, const float* wl, int C, int yb, float lo, float hi, double& glo, double& ghi, double& ty) {
  const double wy = wl[yb];
  glo = ghi = ty = 0.0;
  for (int k = 0; k < C; ++k) {
    if (k == yb) continue;
    const double d = wy - (double)wl[k], q = -p[k];
    if (d > 0.0) {
      glo = glo + q * d;
      ty = ty + q * (double)lo;
    } else {
      ghi = ghi + q * d;
      ty = ty + q * (double)hi;
    }
  }
}

// one term of entry e of [dW_L | db_L] from row b
BD_HD double bg_head_dw_term(int e, int nh, int C, int b, int yb, const float* WL, const float* coef, const float* ty, const float* lo,
                             const float* hi) {
  if (e >= nh * C) return coef[(size_t)b * C + (e - nh * C)];
  const int j = e / C, k = e % C;
  if (k == yb) return ty[(size_t)b * nh + j];
  const double d = (double)WL[(size_t)j * C + yb] - (double)WL[(size_t)j * C + k];
  return (double)coef[(size_t)b * C + k] * (double)(d > 0.0 ? lo[(size_t)b * nh + j] : hi[(size_t)b * nh + j]);
}

// ------------------------------------------------------------------------------------------------------------------- the plan
// the workspace, in floats from a 16-byte boundary; z / h / fam: the boxes of layer_lo / layer_hi (bd_boxes)
struct BgPlan : BdBoxes {
  size_t offCoef = 0, offTy = 0, offG[2][2] = {}, offE[2][2] = {};
  size_t total = 0;
};

static BgPlan bg_plan(const BdShape& sh, int batch) {
  BgPlan p;
  static_cast<BdBoxes&>(p) = bd_boxes(sh, batch);
  const size_t B = batch, C = sh.n[sh.L];
  size_t maxh = 0;
  for (int l = 0; l + 1 < sh.L; ++l) maxh = std::max(maxh, (size_t)sh.n[l + 1]);
  size_t o = 0;
  p.offCoef = o; o = bd_align4(o + B * C);
  p.offTy = o; o = bd_align4(o + B * sh.n[sh.L - 1]);
  for (int s = 0; s < 2; ++s)
    for (int q = 0; q < 2; ++q) {
      p.offG[s][q] = o; o = bd_align4(o + B * maxh);
      p.offE[s][q] = o; o = bd_align4(o + B * maxh);
    }
  p.total = o + 4;
  return p;
}

// -------------------------------------------------------------------------------------------------------------------- kernels
// a block per row b
__global__ __launch_bounds__(kBdThreads) void bg_head_kernel(const float* __restrict__ margin, const float* __restrict__ margin2, float mixbeta,
                                                             const float* __restrict__ inj_lo, const float* __restrict__ inj_hi,
                                                             const int* __restrict__ y,
                                                             const float* __restrict__ WL, int C, int nh, const float* __restrict__ lo,
                                                             const float* __restrict__ hi, int hidden, BdBn bn,
                                                             const float* __restrict__ zlo, const float* __restrict__ zhi,
                                                             float* __restrict__ loss_rows,
                                                             float* __restrict__ coef, float* __restrict__ ty_out, float* __restrict__ gc,
                                                             float* __restrict__ gr, float* __restrict__ es, float* __restrict__ et) {
  __shared__ double p[32];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int yraw = y[b], yb = bg_label(yraw, C);
  const bool ok = yraw == yb;
  if (tid < C) p[tid] = tid == yb ? 0.0 : bg_u(margin, margin2, mixbeta, (size_t)b * C + tid);
  __syncthreads();
  double mx = 0.0;
  for (int k = 0; k < C; ++k) mx = p[k] > mx ? p[k] : mx;
  __syncthreads();
  if (tid < C) p[tid] = ok ? bg_exp(p[tid] - mx) : NAN;
  __syncthreads();
  double sum = 0.0;
  for (int k = 0; k < C; ++k) sum = sum + p[k];
  __syncthreads();
  if (tid < C) p[tid] = p[tid] / sum;
  __syncthreads();
  if (tid == 0) loss_rows[b] = (float)(mx + bg_log(sum));
  if (margin2) {  // the interval part of the mixed margin carries the weight 1 - beta
    __syncthreads();
    if (tid < C) p[tid] = (1.0 - (double)mixbeta) * p[tid];
    __syncthreads();
  }
  if (tid < C) {
    double v = p[tid];
    if (tid == yb) {
      v = 0.0;
      for (int k = 0; k < C; ++k)
        if (k != yb) v = v - p[k];
    }
    coef[(size_t)b * C + tid] = (float)v;
  }
  for (int j = tid; j < nh; j += kBdThreads) {
    const size_t at = (size_t)b * nh + j;
    double glo, ghi, ty;
    bg_head_column(p, WL + (size_t)j * C, C, yb, lo[at], hi[at], glo, ghi, ty);
    ty_out[at] = (float)ty;
    if (hidden) {
      float vc, vr, vs, vt;
      if (inj_lo) bg_gate(glo, ghi, bd_aff(bn, j).s, zlo[at], zhi[at], vc, vr, vs, vt, true, inj_lo[at], inj_hi[at]);
      else bg_gate(glo, ghi, bd_aff(bn, j).s, zlo[at], zhi[at], vc, vr, vs, vt);
      gc[at] = vc;
      gr[at] = vr;
      if (bn.gamma) {
        es[at] = vs;
        et[at] = vt;
      }
    }
  }
}

// kBgCols entries of [dW_L | db_L] a block
__global__ __launch_bounds__(kBdThreads) void bg_head_dw_kernel(const float* __restrict__ WL, const int* __restrict__ y,
                                                                const float* __restrict__ coef, const float* __restrict__ ty,
                                                                const float* __restrict__ lo, const float* __restrict__ hi, int batch, int C,
                                                                int nh, float scale_old, float scale_new, float* __restrict__ dW,
                                                                float* __restrict__ db) {
  const int e = blockIdx.x * kBgCols + threadIdx.x % kBgCols;
  bg_sliced_sum<1>(
      e < nh * C + C, 0, batch,
      [&](int b, double* acc) { acc[0] = acc[0] + bg_head_dw_term(e, nh, C, b, bg_label(y[b], C), WL, coef, ty, lo, hi); },
      [&](const double* tot) { bg_head_store(e, nh, C, tot[0], scale_old, scale_new, dW, db); });
}

// kBgCols columns of a hidden layer a block: db, and (BatchNorm) dgamma and dbeta
__global__ __launch_bounds__(kBdThreads) void bg_colsum_kernel(const float* __restrict__ gc, const float* __restrict__ es,
                                                               const float* __restrict__ et, const float* __restrict__ mmean,
                                                               const float* __restrict__ mvar, int batch, int N, float scale_old,
                                                               float scale_new, float* __restrict__ db, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta) {
  const int j = blockIdx.x * kBgCols + threadIdx.x % kBgCols;
  bg_sliced_sum<3>(
      j < N, 0, batch,
      [&](int b, double* acc) {
        const size_t i = (size_t)b * N + j;
        acc[0] = acc[0] + (double)gc[i];
        if (dgamma) {
          acc[1] = acc[1] + (double)es[i];
          acc[2] = acc[2] + (double)et[i];
        }
      },
      [&](const double* tot) { bg_column_store(j, tot[0], tot[1], tot[2], mmean, mvar, scale_old, scale_new, db, dgamma, dbeta); });
}

// dW[i][j] = sum_b c[b][i] gc[b][j] + sign(W[i][j]) sum_b r[b][i] gr[b][j]: rows i0 .. i0 + 31 (blockIdx.x), columns
// j0 .. j0 + 127 (blockIdx.y), a wavefront per 32 columns, the batch in chunks of 32.
__global__ __launch_bounds__(kBdThreads) void bg_wgrad_kernel(const float* __restrict__ lo, const float* __restrict__ hi,
                                                              const float* __restrict__ gc, const float* __restrict__ gr,
                                                              const float* __restrict__ W, int batch, int K, int N, float scale_old,
                                                              float scale_new, float* __restrict__ dW) {
  __shared__ float cs[kBtNarrow], rs[kBtNarrow], gcs[kBtWideK], grs[kBtWideK];
  const BtThread t;
  const int i0 = blockIdx.x * 32, j0 = blockIdx.y * 128;
  bd_f32x16 acc_c = bt_zero(), acc_r = bt_zero();
  // a row past the batch, a unit past K and a column past N read as 0
  float lreg[4], hreg[4], creg[16], rreg[16];
  auto fetch = [&](int b0) {
    bt_narrow_each(t.tid, [&](int q, int bb, int ii) {
      const int b = b0 + bb, i = i0 + ii;
      const bool in = b < batch && i < K;
      const size_t at = (size_t)b * K + i;
      lreg[q] = in ? lo[at] : 0.0f;
      hreg[q] = in ? hi[at] : 0.0f;
    });
    bt_wide_k_each(t.tid, [&](int q, int bb, int col) {
      const int b = b0 + bb, j = j0 + col;
      const bool in = b < batch && j < N;
      const size_t at = (size_t)b * N + j;
      creg[q] = in ? gc[at] : 0.0f;
      rreg[q] = in ? gr[at] : 0.0f;
    });
  };
  auto stage = [&] {
    bt_narrow_each(t.tid, [&](int q, int bb, int ii) {
      cs[bt_narrow_at(bb, ii)] = 0.5f * (lreg[q] + hreg[q]);
      rs[bt_narrow_at(bb, ii)] = 0.5f * (hreg[q] - lreg[q]);
    });
    bt_wide_k_each(t.tid, [&](int q, int bb, int col) {
      gcs[bt_wide_k_at(bb, col)] = creg[q];
      grs[bt_wide_k_at(bb, col)] = rreg[q];
    });
  };
  bt_pipeline(0, batch, fetch, stage, [&](int s) {
    acc_c = __builtin_amdgcn_mfma_f32_32x32x2f32(BT_NARROW_BY_K(cs, t, s), BT_WIDE_K(gcs, t, s), acc_c, 0, 0, 0);
    acc_r = __builtin_amdgcn_mfma_f32_32x32x2f32(BT_NARROW_BY_K(rs, t, s), BT_WIDE_K(grs, t, s), acc_r, 0, 0, 0);
  });
  const int j = t.col(j0);
  if (j >= N) return;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int i = t.row(i0, e);
    if (i >= K) continue;
    const size_t at = (size_t)i * N + j;
    const float w = W[at];
    const float sg = w > 0.0f ? 1.0f : (w < 0.0f ? -1.0f : 0.0f);
    dW[at] = bg_mix(dW[at], acc_c[e] + sg * acc_r[e], scale_old, scale_new);
  }
}

// (g_c, g_r)[b][i] = sum_j (gc[b][j] W[i][j], gr[b][j] |W[i][j]|): rows b0 .. b0 + 31 (blockIdx.x), columns i0 .. i0 + 127
// (blockIdx.y).  The epilogue applies the layer below: its BatchNorm scale and the z box of row b.
__global__ __launch_bounds__(kBdThreads) void bg_back_kernel(const float* __restrict__ gc, const float* __restrict__ gr,
                                                             const float* __restrict__ W, int batch, int K, int N, BdBn bn,
                                                             const float* __restrict__ zlo, const float* __restrict__ zhi,
                                                             const float* __restrict__ inj_lo, const float* __restrict__ inj_hi,
                                                             float* __restrict__ gc_out, float* __restrict__ gr_out,
                                                             float* __restrict__ es, float* __restrict__ et) {
  __shared__ float a1[kBtNarrow], a2[kBtNarrow], wt[kBtWideN];
  const BtThread t;
  const int b0 = blockIdx.x * 32, i0 = blockIdx.y * 128;
  bd_f32x16 acc_c = bt_zero(), acc_r = bt_zero();
  float creg[4], rreg[4], wreg[16];
  auto fetch = [&](int k0) {
    bt_narrow_each(t.tid, [&](int q, int row, int kk) {
      const int b = b0 + row, k = k0 + kk;
      const bool in = b < batch && k < K;
      const size_t at = (size_t)b * K + k;
      creg[q] = in ? gc[at] : 0.0f;
      rreg[q] = in ? gr[at] : 0.0f;
    });
    bt_wide_n_each(t.tid, [&](int q, int il, int kk) {
      const int i = i0 + il, k = k0 + kk;
      wreg[q] = (i < N && k < K) ? W[(size_t)i * K + k] : 0.0f;
    });
  };
  auto stage = [&] {
    bt_narrow_each(t.tid, [&](int q, int row, int kk) {
      a1[bt_narrow_at(row, kk)] = creg[q];
      a2[bt_narrow_at(row, kk)] = rreg[q];
    });
    bt_wide_n_store(wt, t.tid, wreg);
  };
  bt_pipeline(0, K, fetch, stage, [&](int s) {
    const float w = BT_WIDE_N(wt, t, s);
    acc_c = __builtin_amdgcn_mfma_f32_32x32x2f32(BT_NARROW_BY_ROW(a1, t, s), w, acc_c, 0, 0, 0);
    acc_r = __builtin_amdgcn_mfma_f32_32x32x2f32(BT_NARROW_BY_ROW(a2, t, s), fabsf(w), acc_r, 0, 0, 0);
  });
  const int i = t.col(i0);
  if (i >= N) return;
  const double s = bd_aff(bn, i).s;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int b = t.row(b0, e);
    if (b >= batch) continue;
    const size_t at = (size_t)b * N + i;
    const double c = acc_c[e], r = acc_r[e];
    float vc, vr, vs, vt;
    if (inj_lo) bg_gate(0.5 * (c - r), 0.5 * (c + r), s, zlo[at], zhi[at], vc, vr, vs, vt, true, inj_lo[at], inj_hi[at]);
    else bg_gate(0.5 * (c - r), 0.5 * (c + r), s, zlo[at], zhi[at], vc, vr, vs, vt);
    gc_out[at] = vc;
    gr_out[at] = vr;
    if (bn.gamma) {
      es[at] = vs;
      et[at] = vt;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ host twin
static void bg_host(const BdShape& sh, const BgPlan& pl, const float* params, const float* bnstate, const float* margin,
                    const float* layer_lo, const float* layer_hi, const int* y, int batch, float* ws, float scale_old, float scale_new,
                    float* grads, float* loss_rows, const BgMixIn* mix) {
  const float* margin2 = mix ? mix->margin2 : nullptr;
  const float mixbeta = mix ? mix->beta : 0.0f;
  const int L = sh.L, C = sh.n[L], nh = sh.n[L - 1];
  const bool hidden = L > 1;
  float* coef = ws + pl.offCoef;
  float* ty = ws + pl.offTy;
  const float* WL = params + sh.offW[L - 1];
  const float* hlo = hidden ? layer_lo + pl.h[L - 2] : layer_lo;
  const float* hhi = hidden ? layer_hi + pl.h[L - 2] : layer_hi;
  int cur = 0;
  // head
  BdBn bn = hidden ? bd_bn(sh, params, bnstate, L - 2) : BdBn{};
  for (int b = 0; b < batch; ++b) {
    double p[32];
    const int yb = bg_label(y[b], C);
    const bool ok = yb == y[b];
    double mx = 0.0, sum = 0.0;
    for (int k = 0; k < C; ++k) {
      p[k] = k == yb ? 0.0 : bg_u(margin, margin2, mixbeta, (size_t)b * C + k);
      mx = p[k] > mx ? p[k] : mx;
    }
    for (int k = 0; k < C; ++k) {
      p[k] = ok ? bg_exp(p[k] - mx) : NAN;
      sum = sum + p[k];
    }
    for (int k = 0; k < C; ++k) p[k] = p[k] / sum;
    loss_rows[b] = (float)(mx + bg_log(sum));
    if (margin2)
      for (int k = 0; k < C; ++k) p[k] = (1.0 - (double)mixbeta) * p[k];
    double vy = 0.0;
    for (int k = 0; k < C; ++k)
      if (k != yb) vy = vy - p[k];
    for (int k = 0; k < C; ++k) coef[(size_t)b * C + k] = (float)(k == yb ? vy : p[k]);
    for (int j = 0; j < nh; ++j) {
      const size_t at = (size_t)b * nh + j;
      double glo, ghi, t;
      bg_head_column(p, WL + (size_t)j * C, C, yb, hlo[at], hhi[at], glo, ghi, t);
      ty[at] = (float)t;
      if (hidden) {
        float vs, vt;
        bg_gate(glo, ghi, bd_aff(bn, j).s, layer_lo[pl.z[L - 2] + at], layer_hi[pl.z[L - 2] + at], ws[pl.offG[cur][0] + at],
                ws[pl.offG[cur][1] + at], vs, vt, mix != nullptr, mix ? mix->inj_lo[pl.z[L - 2] + at] : 0.0,
                mix ? mix->inj_hi[pl.z[L - 2] + at] : 0.0);
        if (bn.gamma) { ws[pl.offE[cur][0] + at] = vs; ws[pl.offE[cur][1] + at] = vt; }
      }
    }
  }
  for (int e = 0; e < nh * C + C; ++e) {
    const double tot = bg_sliced_sum_host(0, batch, [&](int b) { return bg_head_dw_term(e, nh, C, b, bg_label(y[b], C), WL, coef, ty, hlo, hhi); });
    bg_head_store(e, nh, C, tot, scale_old, scale_new, grads + sh.offW[L - 1], grads + sh.offb[L - 1]);
  }
  // hidden layers, top down
  std::vector<float> accc, accr;
  for (int l = L - 2; l >= 0; --l) {
    const int K = sh.n[l], N = sh.n[l + 1];
    const float* gc = ws + pl.offG[cur][0];
    const float* gr = ws + pl.offG[cur][1];
    const float* es = ws + pl.offE[cur][0];
    const float* et = ws + pl.offE[cur][1];
    const float* W = params + sh.offW[l];
    bn = bd_bn(sh, params, bnstate, l);
    for (int j = 0; j < N; ++j) {
      const double tb = bg_sliced_sum_host(0, batch, [&](int b) { return (double)gc[(size_t)b * N + j]; });
      const double ts = bn.gamma ? bg_sliced_sum_host(0, batch, [&](int b) { return (double)es[(size_t)b * N + j]; }) : 0.0;
      const double tt = bn.gamma ? bg_sliced_sum_host(0, batch, [&](int b) { return (double)et[(size_t)b * N + j]; }) : 0.0;
      bg_column_store(j, tb, ts, tt, bn.mmean, bn.mvar, scale_old, scale_new, grads + sh.offb[l], bn.gamma ? grads + sh.offg[l] : nullptr,
                      bn.gamma ? grads + sh.offbe[l] : nullptr);
    }
    const float* ilo = l == 0 ? layer_lo : layer_lo + pl.h[l - 1];
    const float* ihi = l == 0 ? layer_hi : layer_hi + pl.h[l - 1];
    for (int i = 0; i < K; ++i) {
      accc.assign(N, 0.0f); accr.assign(N, 0.0f);
      for (int b = 0; b < batch; ++b) {
        const float lo = ilo[(size_t)b * K + i], hi = ihi[(size_t)b * K + i];
        const float c = 0.5f * (lo + hi), r = 0.5f * (hi - lo);
        for (int j = 0; j < N; ++j) {
          accc[j] = std::fmaf(c, gc[(size_t)b * N + j], accc[j]);
          accr[j] = std::fmaf(r, gr[(size_t)b * N + j], accr[j]);
        }
      }
      for (int j = 0; j < N; ++j) {
        const size_t at = (size_t)i * N + j;
        const float w = W[at];
        const float sg = w > 0.0f ? 1.0f : (w < 0.0f ? -1.0f : 0.0f);
        float* out = grads + sh.offW[l] + at;
        *out = bg_mix(*out, accc[j] + sg * accr[j], scale_old, scale_new);
      }
    }
    if (l == 0) break;
    // back: the gradient into the box of layer l - 1, through its gates
    bn = bd_bn(sh, params, bnstate, l - 1);
    for (int b = 0; b < batch; ++b) {
      accc.assign(K, 0.0f); accr.assign(K, 0.0f);
      for (int j = 0; j < N; ++j) {
        const float vc = gc[(size_t)b * N + j], vr = gr[(size_t)b * N + j];
        for (int i = 0; i < K; ++i) {
          const float w = W[(size_t)i * N + j];
          accc[i] = std::fmaf(vc, w, accc[i]);
          accr[i] = std::fmaf(vr, std::fabs(w), accr[i]);
        }
      }
      for (int i = 0; i < K; ++i) {
        const size_t at = (size_t)b * K + i;
        const double c = accc[i], r = accr[i];
        float vs, vt;
        bg_gate(0.5 * (c - r), 0.5 * (c + r), bd_aff(bn, i).s, layer_lo[pl.z[l - 1] + at], layer_hi[pl.z[l - 1] + at],
                ws[pl.offG[cur ^ 1][0] + at], ws[pl.offG[cur ^ 1][1] + at], vs, vt, mix != nullptr, mix ? mix->inj_lo[pl.z[l - 1] + at] : 0.0,
                mix ? mix->inj_hi[pl.z[l - 1] + at] : 0.0);
        if (bn.gamma) { ws[pl.offE[cur ^ 1][0] + at] = vs; ws[pl.offE[cur ^ 1][1] + at] = vt; }
      }
    }
    cur ^= 1;
  }
}

// --------------------------------------------------------------------------------------------------------------------- checks
static int bg_check(const char* fn, const BdShape& sh, const BgPlan& pl, const float* params, const float* bnstate, const float* margin,
                    const float* layer_lo, const float* layer_hi, const int* y, int batch, const float* ws, size_t ws_floats,
                    const float* grads, const float* loss_rows) {
  LP_CHECK_ARG(params && margin && layer_lo && layer_hi && y && ws && grads && loss_rows, "%s: null argument", fn);
  LP_CHECK_ARG(sh.n_state == 0 || bnstate, "%s: bnstate is null", fn);
  LP_CHECK_ARG(ws_floats >= pl.total, "%s: workspace of %zu floats; %zu are needed", fn, ws_floats, pl.total);
  const size_t B = batch, C = sh.n[sh.L];
  const BdSpan sp[] = {{params, sh.n_params * 4, false}, {bnstate, sh.n_state * 4, false}, {margin, B * C * 4, false},
                       {layer_lo, pl.fam * 4, false}, {layer_hi, pl.fam * 4, false}, {y, B * 4, false}, {ws, ws_floats * 4, true},
                       {grads, sh.n_params * 4, true}, {loss_rows, B * 4, true}};
  return bd_check_spans(fn, sp, sizeof(sp) / sizeof(sp[0]));
}

size_t bg_workspace_floats(const BdShape& sh, int batch) { return bg_plan(sh, batch).total; }

void bg_run_host(const BdShape& sh, const float* params, const float* bnstate, const float* margin, const float* layer_lo,
                 const float* layer_hi, const int* y, int batch, float* ws, float scale_old, float scale_new, float* grads, float* loss_rows,
                 const BgMixIn* mix) {
  bg_host(sh, bg_plan(sh, batch), params, bnstate, margin, layer_lo, layer_hi, y, batch, ws, scale_old, scale_new, grads, loss_rows, mix);
}

int bg_run_device(const BdShape& sh, hipStream_t st, const float* params, const float* bnstate, const float* margin, const float* layer_lo,
                  const float* layer_hi, const int* y, int batch, float* ws, float scale_old, float scale_new, float* grads, float* loss_rows,
                  const BgMixIn* mix) {
  const BgPlan pl = bg_plan(sh, batch);
  const float* margin2 = mix ? mix->margin2 : nullptr;
  const float mixbeta = mix ? mix->beta : 0.0f;
  const float* ilo = mix ? mix->inj_lo : nullptr;
  const float* ihi = mix ? mix->inj_hi : nullptr;
  const int L = sh.L, C = sh.n[L], nh = sh.n[L - 1];
  const bool hidden = L > 1;
  float* coef = ws + pl.offCoef;
  float* ty = ws + pl.offTy;
  const float* WL = params + sh.offW[L - 1];
  const float* hlo = hidden ? layer_lo + pl.h[L - 2] : layer_lo;
  const float* hhi = hidden ? layer_hi + pl.h[L - 2] : layer_hi;
  int cur = 0;
  hipLaunchKernelGGL(bg_head_kernel, dim3(batch), dim3(kBdThreads), 0, st, margin, margin2, mixbeta,
                     (hidden && ilo) ? ilo + pl.z[L - 2] : nullptr, (hidden && ihi) ? ihi + pl.z[L - 2] : nullptr, y, WL, C, nh, hlo, hhi,
                     hidden ? 1 : 0, hidden ? bd_bn(sh, params, bnstate, L - 2) : BdBn{},
                     hidden ? layer_lo + pl.z[L - 2] : nullptr, hidden ? layer_hi + pl.z[L - 2] : nullptr, loss_rows, coef, ty,
                     ws + pl.offG[cur][0], ws + pl.offG[cur][1], ws + pl.offE[cur][0], ws + pl.offE[cur][1]);
  LP_LAUNCH_CHECK();
  ++g_bounds_grad_launches[BG_HEAD];
  hipLaunchKernelGGL(bg_head_dw_kernel, dim3((nh * C + C + kBgCols - 1) / kBgCols), dim3(kBdThreads), 0, st, WL, y, coef, ty, hlo, hhi, batch, C, nh,
                     scale_old, scale_new, grads + sh.offW[L - 1], grads + sh.offb[L - 1]);
  LP_LAUNCH_CHECK();
  ++g_bounds_grad_launches[BG_HEAD];
  for (int l = L - 2; l >= 0; --l) {
    const int K = sh.n[l], N = sh.n[l + 1];
    const float* gc = ws + pl.offG[cur][0];
    const float* gr = ws + pl.offG[cur][1];
    const BdBn bn = bd_bn(sh, params, bnstate, l);
    hipLaunchKernelGGL(bg_colsum_kernel, dim3((N + kBgCols - 1) / kBgCols), dim3(kBdThreads), 0, st, gc, ws + pl.offE[cur][0], ws + pl.offE[cur][1],
                       bn.mmean, bn.mvar, batch, N, scale_old, scale_new, grads + sh.offb[l], bn.gamma ? grads + sh.offg[l] : nullptr,
                       bn.gamma ? grads + sh.offbe[l] : nullptr);
    LP_LAUNCH_CHECK();
    ++g_bounds_grad_launches[BG_COLSUM];
    hipLaunchKernelGGL(bg_wgrad_kernel, dim3((K + 31) / 32, (N + 127) / 128), dim3(kBdThreads), 0, st, l == 0 ? layer_lo : layer_lo + pl.h[l - 1],
                       l == 0 ? layer_hi : layer_hi + pl.h[l - 1], gc, gr, params + sh.offW[l], batch, K, N, scale_old, scale_new,
                       grads + sh.offW[l]);
    LP_LAUNCH_CHECK();
    ++g_bounds_grad_launches[BG_WGRAD];
    if (l == 0) break;
    hipLaunchKernelGGL(bg_back_kernel, dim3((batch + 31) / 32, (K + 127) / 128), dim3(kBdThreads), 0, st, gc, gr, params + sh.offW[l], batch, N,
                       K, bd_bn(sh, params, bnstate, l - 1), layer_lo + pl.z[l - 1], layer_hi + pl.z[l - 1], ilo ? ilo + pl.z[l - 1] : nullptr,
                       ihi ? ihi + pl.z[l - 1] : nullptr, ws + pl.offG[cur ^ 1][0], ws + pl.offG[cur ^ 1][1],
                       ws + pl.offE[cur ^ 1][0], ws + pl.offE[cur ^ 1][1]);
    LP_LAUNCH_CHECK();
    ++g_bounds_grad_launches[BG_BACK];
    cur ^= 1;
  }
  return LIPASR_OK;
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

long lipasr_debug_bounds_grad_launches(int kernel) { return (kernel >= 0 && kernel < 4) ? g_bounds_grad_launches[kernel] : -1; }

int lipasr_mlp_bounds_grad_workspace(lipasr_mlp_t m, int batch, size_t* floats) {
  const char* fn = "lipasr_mlp_bounds_grad_workspace";
  BdShape sh;
  return bd_workspace(fn, bd_shape_of(fn, m, &sh), sh, batch, floats, bg_plan);
}

int lipasr_mlp_bounds_grad_workspace_host(int n_layers, const int* widths, int batch, size_t* floats) {
  const char* fn = "lipasr_mlp_bounds_grad_workspace_host";
  BdShape sh;
  return bd_workspace(fn, bd_shape_from(fn, n_layers, widths, nullptr, &sh), sh, batch, floats, bg_plan);
}

int lipasr_mlp_bounds_grad(lipasr_mlp_t m, const float* params, const float* bnstate, const float* margin_ibp, const float* layer_lo,
                           const float* layer_hi, const int* y, int batch, float* workspace, size_t workspace_floats, float scale_old,
                           float scale_new, float* grads, float* loss_rows, lipasr_stream_t stream) {
  const char* fn = "lipasr_mlp_bounds_grad";
  BdShape sh;
  if (int rc = bd_shape_of(fn, m, &sh)) return rc;
  if (int rc = bd_batch_check(fn, sh, batch)) return rc;
  const BgPlan pl = bg_plan(sh, batch);
  if (int rc = bg_check(fn, sh, pl, params, bnstate, margin_ibp, layer_lo, layer_hi, y, batch, workspace, workspace_floats, grads, loss_rows))
    return rc;
  DeviceGuard guard(m->ctx->device);
  return bg_run_device(sh, S(stream), params, bnstate, margin_ibp, layer_lo, layer_hi, y, batch, bd_base(workspace), scale_old, scale_new, grads,
                       loss_rows, nullptr);
}

int lipasr_mlp_bounds_grad_host(int n_layers, const int* widths, const int* bn, const float* params, const float* bnstate,
                                const float* margin_ibp, const float* layer_lo, const float* layer_hi, const int* y, int batch,
                                float* workspace, size_t workspace_floats, float scale_old, float scale_new, float* grads,
                                float* loss_rows) {
  const char* fn = "lipasr_mlp_bounds_grad_host";
  BdShape sh;
  if (int rc = bd_shape_from(fn, n_layers, widths, bn, &sh)) return rc;
  if (int rc = bd_batch_check(fn, sh, batch)) return rc;
  const BgPlan pl = bg_plan(sh, batch);
  if (int rc = bg_check(fn, sh, pl, params, bnstate, margin_ibp, layer_lo, layer_hi, y, batch, workspace, workspace_floats, grads, loss_rows))
    return rc;
  bg_host(sh, pl, params, bnstate, margin_ibp, layer_lo, layer_hi, y, batch, bd_base(workspace), scale_old, scale_new, grads, loss_rows, nullptr);
  return LIPASR_OK;
}

}  // extern "C"
