// Certified robustness of the dense classifier by bound propagation (lipasr/bounds.py): interval bounds (IBP) forward through the
// layers, one backward linear-relaxation pass (CROWN-IBP) for the margins z_y - z_k.  DESIGN.md, "Bound propagation", derives every
// constant below.
//
//   bounds_prep_kernel   1 launch   the input box [x - eps_b, x + eps_b] /\ [clip_lo, clip_hi] rounded outward, the row's NaN flag,
//                                   and (norm 2) the column norms of W_1
//   bounds_layer_kernel  L - 1      one hidden layer: the tile of bounds_tile.h (narrow operand by output row, W k-major) with (W c,
//                                   |W| r, |W| |c|) from ONE read of W, three accumulators per wavefront (48 accumulator registers),
//                                   c and r formed as the box is staged, |W| and |c| in registers; epilogue: bias, widening, store
//                                   (lo_z, hi_z, S), ReLU, BatchNorm affine with the sign of s, outward rounding, store the next (lo, hi)
//   bounds_head_kernel   1          Lambda_L[b][k] = W_L[y_b] - W_L[k], the IBP margins, and the relaxation of layer L - 1
//   bounds_back_kernel   L - 1      Lambda_{l-1} = Lambda_l W_l^T for M = batch x classes rows on the same tile, W n-major; epilogue: layer
//                                   l - 1's BatchNorm and ReLU relaxation from row b = m / C's bounds, the constant and the slack of
//                                   the row's 32 columns as ONE partial each (a butterfly over the 32 lanes: fixed order, no atomics)
//   bounds_tail_kernel   1          the input reduction, the partials in index order, margin_crown and slack
//
// Forward L + 1 launches, backward L (none when margin_crown is null).  Every sum has one order that depends on the shapes alone:
// the MFMA is an fmaf chain in ascending k, a row's constant is the butterfly of each 32-column tile, then the tiles in ascending
// order, then the stages top-down.  Head, tail and prep run one BD_HD function per element and per row (bd_head_point,
// bd_head_finish, bd_tail_point, bd_tail_finish, bd_prep_point) that the host twin calls too, in those orders, so host and device give the
// same values (a zero may differ in sign: the padded k steps of a tile turn a -0 accumulator into +0).
// Rows are independent everywhere, so a NaN stays in its row; the flag of bounds_prep_kernel makes such a row's margins NaN.
// Loads and stores are single floats, guarded: any width, any batch, any alignment.  Nothing allocates or synchronises.
#include "bounds_tile.h"

// host and device must round alike, and a product that is rounded before its sum is what the error bounds below assume
#pragma clang fp contract(off)

namespace lipasr {

long g_bounds_launches[5] = {};
enum { BD_PREP = 0, BD_LAYER = 1, BD_HEAD = 2, BD_BACK = 3, BD_TAIL = 4 };

BD_HD unsigned bd_bits(float f) { return __builtin_bit_cast(unsigned, f); }
BD_HD float bd_float(unsigned u) { return __builtin_bit_cast(float, u); }
// the next fp32 above / below; a NaN and the infinity on that side stay
BD_HD float bd_step_up(float f) {
  if (f != f || f == INFINITY) return f;
  if (f == 0.0f) return bd_float(1u);
  const unsigned u = bd_bits(f);
  return bd_float(f > 0.0f ? u + 1u : u - 1u);
}
BD_HD float bd_step_dn(float f) {
  if (f != f || f == -INFINITY) return f;
  if (f == 0.0f) return bd_float(0x80000001u);
  const unsigned u = bd_bits(f);
  return bd_float(f > 0.0f ? u - 1u : u + 1u);
}
// the largest fp32 <= v / the smallest fp32 >= v
BD_HD float bd_dn(double v) {
  const float f = (float)v;
  return (double)f > v ? bd_step_dn(f) : f;
}
BD_HD float bd_up(double v) {
  const float f = (float)v;
  return (double)f < v ? bd_step_up(f) : f;
}
BD_HD double bd_gamma(int n) { return n * kBdU / (1.0 - n * kBdU); }
// what an fmaf chain of K products plus the bias can be off by, given S >= sum of the magnitudes: two chains meet in one bound
BD_HD double bd_widen(int K, double S) { return bd_gamma(K + 1) * S + 2.0 * (K + 1) * kBdTiny; }

// the input box of one element: [x - eps, x + eps] /\ [clip_lo, clip_hi], rounded outward (exact at eps = 0)
BD_HD void bd_input_box(float x, float eps, float clip_lo, float clip_hi, float& lo, float& hi) {
  if (eps == 0.0f) {
    lo = hi = x;
  } else {
    const double d = kBdD * (fabs((double)x) + (double)eps);
    lo = bd_dn((double)x - (double)eps - d);
    hi = bd_up((double)x + (double)eps + d);
  }
  if (lo < clip_lo) lo = clip_lo;
  if (hi > clip_hi) hi = clip_hi;
}

// centre and radius with [c - r, c + r] a superset of [lo, hi]
BD_HD void bd_mid_rad(float lo, float hi, float& c, float& r) {
  if (lo == hi) { c = lo; r = 0.0f; return; }
  const double dl = lo, dh = hi;
  c = (float)(0.5 * (dl + dh));
  const double dc = c;
  r = bd_up(bd_max(dh - dc, dc - dl) + kBdD * (fabs(dl) + fabs(dh)));
  if (r < 0.0f) r = 0.0f;  // an empty box (the clip box does not meet the ball)
}
// norm 2, first layer: the centre stays x, the radius covers the box on both sides
BD_HD void bd_sym_rad(float x, float lo, float hi, float& c, float& r) {
  c = x;
  if (lo == hi && lo == x) { r = 0.0f; return; }
  const double dx = x;
  r = bd_up(bd_max((double)hi - dx, dx - (double)lo) + kBdD * (fabs((double)lo) + fabs((double)hi) + fabs(dx)));
  if (r < 0.0f) r = 0.0f;
}

// one pre-activation box from the three sums of a column: ac = fl(W c), ar = fl(|W| r), as = fl(|W| |c|)
BD_HD void bd_z_box(float ac, float ar, float as, float bias, int K, bool l2, float eps, float colnorm, float& zlo, float& zhi,
                    float& S) {
  const double g = bd_gamma(K + 1);
  S = bd_up((((double)as + (double)ar) * (1.0 + 2.0 * g) + fabs((double)bias) + 2.0 * (K + 1) * kBdTiny) * (1.0 + kBdD));
  const double w = bd_widen(K, (double)S);
  double rad = ar;
  if (l2) {
    const double r2 = (double)eps * (double)colnorm * (1.0 + kBdD);
    if (r2 < rad) rad = r2;
  }
  const double zc = (double)ac + (double)bias;
  zlo = bd_dn(zc - rad - w);
  zhi = bd_up(zc + rad + w);
}

// ReLU, then the affine map with lo and hi swapped where s < 0, rounded outward.  v < 0 ? 0 : v keeps a NaN.
BD_HD void bd_post_box(float zlo, float zhi, const BdAff& a, float& hlo, float& hhi) {
  const double alo = zlo < 0.0f ? 0.0 : (double)zlo, ahi = zhi < 0.0f ? 0.0 : (double)zhi;
  const double d = kBdD * (fabs(a.s) * ahi + a.tm);
  const double vlo = a.s >= 0.0 ? a.s * alo + a.t : a.s * ahi + a.t;
  const double vhi = a.s >= 0.0 ? a.s * ahi + a.t : a.s * alo + a.t;
  hlo = bd_dn(vlo - d);
  hhi = bd_up(vhi + d);
}

// Lambda on h_j = s relu(z_j) + t becomes nu on z_j: dc goes to the row's constant, ds to its slack.
//   lam       the coefficient as stored (fp32); kin: the K of the product that made it (0: none), whose subnormal term sits here
//   zlo, zhi  the pre-activation box of the row, S its sum of magnitudes, bias the b_j of z_j = (W h)_j + b_j; kout: the K of the
//             product nu goes into
BD_HD void bd_relax(float lam, const BdAff& a, float zlo, float zhi, float S, float bias, int kin, int kout, float& nu, double& dc,
                    double& ds) {
  const double p = (double)lam * a.s;
  const double ahi = zhi < 0.0f ? 0.0 : (double)zhi;
  const double Z = bd_max(fabs((double)zlo), fabs((double)zhi));
  bool upper;
  const double slope = bd_slope(p, zlo, zhi, upper);
  const double icpt = upper ? -(p * slope * (double)zlo) * (1.0 + kBdD) : 0.0;  // <= 0, rounded away from 0
  nu = (float)(p * slope);
  const double lt = (double)lam * a.t, nb = (double)nu * (double)bias;
  dc = lt + icpt + nb;
  ds = kBdD * (fabs(lt) + fabs((double)lam) * a.tm + fabs(icpt) + fabs(nb))  // fp64 roundings of t and of the three terms
       + (2.0 * kBdU * fabs((double)nu) + kBdTiny) * Z                        // nu is the real p * slope rounded to fp32
       + bd_gamma(kout + 1) * fabs((double)nu) * (double)S;                   // the product nu W that follows
  if (kin) ds = ds + (kin + 1) * kBdTiny * (fabs(a.s) * ahi + a.tm) * (1.0 + kBdD);  // subnormal steps of the product before
}

// min over the input set of a . v, term by term: box form, and (norm 2) the ball form around x
struct BdRed { double boxmin, dot, sq, mag; };
BD_HD void bd_red_add(BdRed& r, double a, float lo, float hi, bool l2, float x) {
  const double pl = a * (double)lo, ph = a * (double)hi;
  r.boxmin = pl < ph ? pl : ph;
  double mx = bd_max(fabs((double)lo), fabs((double)hi));
  r.dot = 0.0;
  r.sq = 0.0;
  if (l2) {
    r.dot = a * (double)x;
    r.sq = a * a;
    mx = bd_max(mx, fabs((double)x));
  }
  r.mag = fabs(a) * mx;
}
BD_HD double bd_red_finish(const BdRed& r, bool l2, float eps) {
  double v = r.boxmin;
  if (l2) {
    const double v2 = r.dot - (double)eps * sqrt(r.sq) * (1.0 + kBdD);
    if (v2 > v) v = v2;
  }
  return v - kBdD * r.mag;
}

// --------------------------------------------------------------------------------- the steps the kernels and the host twin share
// a row of bounds_prep_kernel: what makes it a NaN row apart from its x / one element: the input box, and whether x is a NaN
BD_HD int bd_prep_row(float eps, int y, int classes) { return !(eps >= 0.0f) || y < 0 || y >= classes; }
BD_HD int bd_prep_point(const float* x, size_t at, float eps, float clip_lo, float clip_hi, float* lo0, float* hi0) {
  const float v = x[at];
  bd_input_box(v, eps, clip_lo, clip_hi, lo0[at], hi0[at]);
  return v != v;
}
BD_HD float bd_colnorm(double sum_sq) { return bd_up(sqrt(sum_sq) * (1.0 + kBdD)); }

// the label a row is bounded for: a flagged row takes class 0 and ends as NaN
BD_HD int bd_row_label(const int* flag, const int* y, int b) { return flag[b] ? 0 : y[b]; }

// column j of row (b, k) in the head: d = W_L[j][y] - W_L[j][k] in fp64, lam its fp32 rounding (0 on the row's own class).
// lo / hi: the box of h_{L-1} [batch][nh], x = null; one layer: the input box, and x its centre.  rx.on: the relaxation of layer
// L - 1 turns lam into nu.  r: the terms of the IBP margin; dc, ds: the column's constant and slack
struct BdRelaxAt {  // the layer a relaxation applies: its BatchNorm, its z box and S [batch][n], its bias [n]; on = false: none
  bool on;
  BdBn bn;
  const float *zlo, *zhi, *S, *bias;
};
BD_HD void bd_head_point(const float* WL, int C, int nh, int b, int k, int yb, int j, const float* lo, const float* hi, const float* x,
                         bool l2, const BdRelaxAt& rx, float& nu, double& dc, double& ds, BdRed& r) {
  const size_t at = (size_t)b * nh + j;
  const double d = (double)WL[(size_t)j * C + yb] - (double)WL[(size_t)j * C + k];
  const float lam = k == yb ? 0.0f : (float)d;
  const float l = lo[at], u = hi[at];
  bd_red_add(r, d, l, u, l2, x ? x[at] : 0.0f);
  // lam is the real difference rounded to fp32
  const double H = bd_max(bd_max(fabs((double)l), fabs((double)u)), x ? fabs((double)x[at]) : 0.0);
  dc = 0.0;
  ds = 2.0 * kBdU * fabs((double)lam) * H;
  nu = lam;
  if (rx.on) {
    double rc, rs;
    bd_relax(lam, bd_aff(rx.bn, j), rx.zlo[at], rx.zhi[at], rx.S[at], rx.bias[j], 0, nh, nu, rc, rs);
    dc = rc;
    ds = ds + rs;
  }
}
// the head's row (b, k) from its sums: the constant and the slack so far (acc[0 .. 1]) and the IBP margin.  own: k == y_b
BD_HD void bd_head_finish(double csum, double ssum, const BdRed& tot, float by, float bk, bool l2, float eps, bool bad, bool own,
                          double* acc, float* margin_ibp) {
  const double c0 = (double)by - (double)bk;
  acc[0] = csum + c0;
  acc[1] = ssum + kBdD * (fabs((double)by) + fabs((double)bk) + fabs(csum));
  const double v = bd_red_finish(tot, l2, eps) + c0 - kBdD * (fabs((double)by) + fabs((double)bk) + fabs(tot.boxmin));
  *margin_ibp = bad ? NAN : (own ? INFINITY : bd_dn(v));
}

// column j of a row in the tail: the term of the input reduction of Lambda_0 and the subnormal steps of the product that made it
BD_HD void bd_tail_point(const float* lam0, size_t m, int n0, int b, int j, const float* lo0, const float* hi0, const float* x, bool l2,
                         int kin, double& ds, BdRed& r) {
  const size_t at = (size_t)b * n0 + j;
  const float l = lo0[at], u = hi0[at];
  bd_red_add(r, (double)lam0[m * n0 + j], l, u, l2, x[at]);
  ds = kin ? (kin + 1) * kBdTiny * bd_max(fabs((double)l), fabs((double)u)) : 0.0;
}
// the partial sums of the back stages, top-down, as the tail reads them
struct BdStages {
  int count;
  int tiles[LIPASR_MAX_LAYERS];
  const double* part[LIPASR_MAX_LAYERS];
};
// the tail's row m: the head's (constant, slack), the stages' partials in their fixed order, margin_crown and the slack
BD_HD void bd_tail_finish(const double* rowacc, double ssum, const BdRed& tot, const BdStages& st, size_t m, bool l2, float eps,
                          bool bad, bool own, float* margin_crown, float* slack) {
  double c = rowacc[2 * m], s = rowacc[2 * m + 1] + ssum, cm = fabs(c);
  for (int g = 0; g < st.count; ++g) {
    const double* p = st.part[g] + 2 * m * st.tiles[g];
    for (int t = 0; t < st.tiles[g]; ++t) {
      c = c + p[2 * t];
      cm = cm + fabs(p[2 * t]);
      s = s + p[2 * t + 1];
    }
  }
  const double red = bd_red_finish(tot, l2, eps);
  s = (s + kBdD * (cm + fabs(red))) * (1.0 + kBdD);
  margin_crown[m] = bad ? NAN : (own ? INFINITY : bd_dn(red + c - s));
  if (slack) slack[m] = bad ? NAN : (own ? 0.0f : bd_up(s));
}

// ------------------------------------------------------------------------------------------------------------------- the plan
// the workspace, in floats from a 16-byte boundary.  The lo family is one span [lo0 | zlo_1 | hlo_1 | zlo_2 | ...], the hi family
// likewise: layer_lo / layer_hi are one copy each.
struct BdPlan : BdBoxes {              // fam: floats of one family; z / h: offsets inside a family, hidden layers 0 .. L - 2
  size_t offLo = 0, offHi = 0;         // the families
  size_t offS[LIPASR_MAX_LAYERS] = {};
  size_t offNorm = 0, offFlag = 0, offLam[2] = {}, offAcc = 0, offPart[LIPASR_MAX_LAYERS] = {};
  int tiles[LIPASR_MAX_LAYERS] = {};   // partial columns of back stage l (the product with W_l, l = 1 .. L - 2): 4 ceil(n_l / 128)
  size_t total = 0;                    // with the slack of the alignment
};

static BdPlan bd_plan(const BdShape& sh, int batch) {
  BdPlan p;
  static_cast<BdBoxes&>(p) = bd_boxes(sh, batch);
  const size_t B = batch, C = sh.n[sh.L], M = B * C, f = p.fam;
  size_t o = 0;
  p.offLo = o; o = bd_align4(o + f);
  p.offHi = o; o = bd_align4(o + f);
  int maxw = sh.n[0];
  for (int l = 0; l + 1 < sh.L; ++l) {
    p.offS[l] = o; o = bd_align4(o + B * sh.n[l + 1]);
    maxw = std::max(maxw, sh.n[l + 1]);
  }
  p.offNorm = o; o = bd_align4(o + (sh.L > 1 ? sh.n[1] : 0));
  p.offFlag = o; o = bd_align4(o + B);
  p.offLam[0] = o; o = bd_align4(o + M * maxw);
  p.offLam[1] = o; o = bd_align4(o + M * maxw);
  p.offAcc = o; o = bd_align4(o + 2 * 2 * M);  // doubles: [M][2]
  for (int l = 1; l + 1 < sh.L; ++l) {
    p.tiles[l] = 4 * ((sh.n[l] + 127) / 128);
    p.offPart[l] = o; o = bd_align4(o + 2 * 2 * M * p.tiles[l]);  // doubles: [M][tiles][2]
  }
  p.total = o + 4;
  return p;
}

// the stages of a call in the tail's order: l = L - 2 down to 1
static BdStages bd_stages(const BdShape& sh, const BdPlan& pl, const float* ws) {
  BdStages stg;
  stg.count = 0;
  for (int l = sh.L - 2; l >= 1; --l) {
    stg.tiles[stg.count] = pl.tiles[l];
    stg.part[stg.count] = reinterpret_cast<const double*>(ws + pl.offPart[l]);
    ++stg.count;
  }
  return stg;
}

// -------------------------------------------------------------------------------------------------------------------- kernels
constexpr int kBdNormSlices = kBdThreads / 32;

__device__ __forceinline__ double bd_sum32(double v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// the same order on the host: v[0] of 32 terms
static inline double bd_sum32_host(double (&v)[32]) {
  for (int o = 16; o > 0; o >>= 1)
    for (int i = 0; i < o; ++i) v[i] = v[i] + v[i + o];
  return v[0];
}
// tot += the 32 lanes' terms of the input reduction, each field under the butterfly; on the host the lanes are r[0 .. 32)
__device__ __forceinline__ void bd_red_sum32(BdRed& tot, const BdRed& r) {
  tot.boxmin = tot.boxmin + bd_sum32(r.boxmin);
  tot.dot = tot.dot + bd_sum32(r.dot);
  tot.sq = tot.sq + bd_sum32(r.sq);
  tot.mag = tot.mag + bd_sum32(r.mag);
}
static inline void bd_red_sum32_host(BdRed& tot, const BdRed (&r)[32]) {
  for (double BdRed::*f : {&BdRed::boxmin, &BdRed::dot, &BdRed::sq, &BdRed::mag}) {
    double v[32];
    for (int q = 0; q < 32; ++q) v[q] = r[q].*f;
    tot.*f = tot.*f + bd_sum32_host(v);
  }
}

// blocks [0, batch): one row's input box and flag.  blocks from batch on (norm 2): 32 column norms of W_1 each, a column's squares
// in 8 interleaved fp64 partial sums (thread slice s takes i = s, s + 8, ...) that meet in index order.
__global__ __launch_bounds__(kBdThreads) void bounds_prep_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                                 const int* __restrict__ y, int batch, int n0, int classes,
                                                                 float clip_lo, float clip_hi, float* __restrict__ lo0,
                                                                 float* __restrict__ hi0, int* __restrict__ flag,
                                                                 const float* __restrict__ W1, int n1, float* __restrict__ colnorm) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < batch) {
    const int b = blockIdx.x;
    const float e = eps[b];
    int bad = bd_prep_row(e, y[b], classes);
    for (int i = tid; i < n0; i += kBdThreads) bad |= bd_prep_point(x, (size_t)b * n0 + i, e, clip_lo, clip_hi, lo0, hi0);
    bad = __syncthreads_or(bad);
    if (tid == 0) flag[b] = bad;
  } else {
    __shared__ double parts[kBdNormSlices][32];
    const int jl = tid & 31, sl = tid >> 5;
    const int j = ((int)blockIdx.x - batch) * 32 + jl;
    double acc = 0.0;
    if (j < n1) {
      for (int i = sl; i < n0; i += kBdNormSlices) {
        const double w = W1[(size_t)i * n1 + j];
        acc = acc + w * w;
      }
    }
    parts[sl][jl] = acc;
    __syncthreads();
    if (sl == 0 && j < n1) {
      double tot = parts[0][jl];
      for (int q = 1; q < kBdNormSlices; ++q) tot = tot + parts[q][jl];
      colnorm[j] = bd_colnorm(tot);
    }
  }
}

// z = W h + b over a box of h: rows b0 .. b0 + 31 (blockIdx.x), columns n0 .. n0 + 127 (blockIdx.y), a wavefront per 32 columns.
// x != null: the first layer under norm 2 (centre x, radius min(|W| r, eps ||W_j||_2)).
__global__ __launch_bounds__(kBdThreads) void bounds_layer_kernel(const float* __restrict__ lo, const float* __restrict__ hi,
                                                                  const float* __restrict__ x, const float* __restrict__ eps,
                                                                  const float* __restrict__ colnorm, const float* __restrict__ W,
                                                                  const float* __restrict__ bias, BdBn bn, int batch, int K, int N,
                                                                  float* __restrict__ zlo, float* __restrict__ zhi,
                                                                  float* __restrict__ Sout, float* __restrict__ hlo,
                                                                  float* __restrict__ hhi) {
  __shared__ float cs[kBtNarrow], rs[kBtNarrow], wsm[kBtWideK];
  const BtThread t;
  const int b0 = blockIdx.x * 32, n0 = blockIdx.y * 128;
  bd_f32x16 acc_c = bt_zero(), acc_r = bt_zero(), acc_s = bt_zero();
  // 28 loads per thread and chunk, 48 MFMAs per wavefront; an element past the batch or past K is the point box 0, whose centre
  // and radius are 0.  |W| and |c| are formed in registers, the centre and the radius as the box is staged
  float lreg[4], hreg[4], xreg[4], wreg[16];
  auto fetch = [&](int k0) {
    bt_narrow_each(t.tid, [&](int q, int row, int kk) {
      const int b = b0 + row, k = k0 + kk;
      const bool in = b < batch && k < K;
      const size_t at = (size_t)b * K + k;
      lreg[q] = in ? lo[at] : 0.0f;
      hreg[q] = in ? hi[at] : 0.0f;
      xreg[q] = (in && x) ? x[at] : 0.0f;
    });
    bt_wide_k_each(t.tid, [&](int q, int kk, int col) {
      const int k = k0 + kk, j = n0 + col;
      wreg[q] = (k < K && j < N) ? W[(size_t)k * N + j] : 0.0f;
    });
  };
  auto stage = [&] {
    bt_narrow_each(t.tid, [&](int q, int row, int kk) {
      float c, r;
      if (x) bd_sym_rad(xreg[q], lreg[q], hreg[q], c, r);
      else bd_mid_rad(lreg[q], hreg[q], c, r);
      cs[bt_narrow_at(row, kk)] = c;
      rs[bt_narrow_at(row, kk)] = r;
    });
    bt_wide_k_store(wsm, t.tid, wreg);
  };
  bt_pipeline(0, K, fetch, stage, [&](int s) {
    const float c = bt_narrow_by_row(cs, t, s), r = bt_narrow_by_row(rs, t, s);
    const float w = bt_wide_k(wsm, t, s), aw = fabsf(w);
    acc_c = __builtin_amdgcn_mfma_f32_32x32x2f32(c, w, acc_c, 0, 0, 0);
    acc_r = __builtin_amdgcn_mfma_f32_32x32x2f32(r, aw, acc_r, 0, 0, 0);
    acc_s = __builtin_amdgcn_mfma_f32_32x32x2f32(fabsf(c), aw, acc_s, 0, 0, 0);
  });
  const int j = t.col(n0);
  if (j >= N) return;
  const BdAff a = bd_aff(bn, j);
  const float bj = bias[j];
  const float cn = x ? colnorm[j] : 0.0f;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int b = t.row(b0, e);
    if (b >= batch) continue;
    const size_t at = (size_t)b * N + j;
    float l, u, S, pl, pu;
    bd_z_box(acc_c[e], acc_r[e], acc_s[e], bj, K, x != nullptr, x ? eps[b] : 0.0f, cn, l, u, S);
    zlo[at] = l;
    zhi[at] = u;
    Sout[at] = S;
    bd_post_box(l, u, a, pl, pu);
    hlo[at] = pl;
    hhi[at] = pu;
  }
}

// 32 lanes per row m = b C + k: Lambda_L, the IBP margin, and (hidden layers) the relaxation of the last hidden layer.
// hidden: lo / hi = the box of h_{L-1}, x = null.  One layer: lo / hi = the input box, x and eps and l2 as the caller gave them.
__global__ __launch_bounds__(kBdThreads) void bounds_head_kernel(const float* __restrict__ WL, const float* __restrict__ bL,
                                                                 const int* __restrict__ y, const int* __restrict__ flag, int M, int C,
                                                                 int nh, const float* __restrict__ lo, const float* __restrict__ hi,
                                                                 const float* __restrict__ x, const float* __restrict__ eps, int l2,
                                                                 int hidden, BdBn bn, const float* __restrict__ zlo,
                                                                 const float* __restrict__ zhi, const float* __restrict__ S,
                                                                 const float* __restrict__ bias, float* __restrict__ lam_out,
                                                                 double* __restrict__ rowacc,
                                                                 float* __restrict__ margin_ibp) {
  const int li = threadIdx.x & 31;
  const int m = blockIdx.x * (kBdThreads / 32) + (threadIdx.x >> 5);
  if (m >= M) return;  // whole 32-lane groups leave; the butterflies below stay inside a group
  const int b = m / C, k = m % C, yb = bd_row_label(flag, y, b);
  const BdRelaxAt rx{hidden != 0, bn, zlo, zhi, S, bias};
  double csum = 0.0, ssum = 0.0;
  BdRed tot{0.0, 0.0, 0.0, 0.0};
  for (int j0 = 0; j0 < nh; j0 += 32) {
    const int j = j0 + li;
    double dc = 0.0, ds = 0.0;
    BdRed r{0.0, 0.0, 0.0, 0.0};
    if (j < nh) {
      float nu;
      bd_head_point(WL, C, nh, b, k, yb, j, lo, hi, x, l2 != 0, rx, nu, dc, ds, r);
      lam_out[(size_t)m * nh + j] = nu;
    }
    csum = csum + bd_sum32(dc);
    ssum = ssum + bd_sum32(ds);
    bd_red_sum32(tot, r);
  }
  if (li == 0)
    bd_head_finish(csum, ssum, tot, bL[yb], bL[k], l2 != 0, eps[b], flag[b] != 0, k == yb, rowacc + 2 * (size_t)m, margin_ibp + m);
}

// out[m][i] = sum_j A[m][j] W[i][j]: rows m0 .. m0 + 31 (blockIdx.x), columns i0 .. i0 + 127 (blockIdx.y).  relax: the epilogue
// applies the layer below (its BatchNorm parameters and the z box and S of row m / C) and writes one partial per row and wavefront.
__global__ __launch_bounds__(kBdThreads) void bounds_back_kernel(const float* __restrict__ A, const float* __restrict__ W, int M, int K,
                                                                 int N, int C, int relax, BdBn bn, const float* __restrict__ zlo,
                                                                 const float* __restrict__ zhi, const float* __restrict__ S,
                                                                 const float* __restrict__ bias, float* __restrict__ out,
                                                                 double* __restrict__ part, int tiles) {
  __shared__ float as[kBtNarrow], wt[kBtWideN];
  const BtThread t;
  const int m0 = blockIdx.x * 32, i0 = blockIdx.y * 128, li = t.li, wave = t.wave;
  bd_f32x16 acc = bt_zero();
  float areg[4], wreg[16];
  auto fetch = [&](int k0) {
    bt_narrow_each(t.tid, [&](int q, int row, int kk) {
      const int m = m0 + row, k = k0 + kk;
      areg[q] = (m < M && k < K) ? A[(size_t)m * K + k] : 0.0f;
    });
    bt_wide_n_each(t.tid, [&](int q, int il, int kk) {
      const int i = i0 + il, k = k0 + kk;
      wreg[q] = (i < N && k < K) ? W[(size_t)i * K + k] : 0.0f;
    });
  };
  auto stage = [&] {
    bt_narrow_store(as, t.tid, areg);
    bt_wide_n_store(wt, t.tid, wreg);
  };
  bt_pipeline(0, K, fetch, stage, [&](int s) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bt_narrow_by_row(as, t, s), bt_wide_n(wt, t, s), acc, 0, 0, 0);
  });
  const int i = t.col(i0);
  const bool col = i < N;
  BdAff a{1.0, 0.0, 0.0};
  if (relax && col) a = bd_aff(bn, i);
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int m = t.row(m0, e);
    const bool ok = col && m < M;
    float nu = acc[e];
    double dc = 0.0, ds = 0.0;
    if (relax && ok) {
      const size_t at = (size_t)(m / C) * N + i;
      bd_relax(acc[e], a, zlo[at], zhi[at], S[at], bias[i], K, N, nu, dc, ds);
    }
    if (ok) out[(size_t)m * N + i] = nu;
    if (relax) {
      dc = bd_sum32(dc);
      ds = bd_sum32(ds);
      if (li == 0 && m < M) {
        double* p = part + 2 * ((size_t)m * tiles + (blockIdx.y * 4 + wave));
        p[0] = dc;
        p[1] = ds;
      }
    }
  }
}

// the plain product out = A W^T of bounds_back_kernel (no relaxation, no partials), for the chain that bounds_crown_grad.hip keeps
int bd_launch_product(hipStream_t st, const float* A, const float* W, int M, int K, int N, int C, float* out) {
  hipLaunchKernelGGL(bounds_back_kernel, dim3((M + 31) / 32, (N + 127) / 128), dim3(kBdThreads), 0, st, A, W, M, K, N, C, 0, BdBn{}, nullptr,
                     nullptr, nullptr, nullptr, out, nullptr, 0);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

// 32 lanes per row m: the input reduction of Lambda_0, the constants and slacks in their fixed order, the two outputs.
__global__ __launch_bounds__(kBdThreads) void bounds_tail_kernel(const float* __restrict__ lam0, const int* __restrict__ y,
                                                                 const int* __restrict__ flag, int M, int C, int n0, int kin,
                                                                 const float* __restrict__ lo0, const float* __restrict__ hi0,
                                                                 const float* __restrict__ x, const float* __restrict__ eps, int l2,
                                                                 const double* __restrict__ rowacc, BdStages st,
                                                                 float* __restrict__ margin_crown, float* __restrict__ slack) {
  const int li = threadIdx.x & 31;
  const int m = blockIdx.x * (kBdThreads / 32) + (threadIdx.x >> 5);
  if (m >= M) return;
  const int b = m / C, k = m % C, yb = bd_row_label(flag, y, b);
  double ssum = 0.0;
  BdRed tot{0.0, 0.0, 0.0, 0.0};
  for (int j0 = 0; j0 < n0; j0 += 32) {
    const int j = j0 + li;
    double ds = 0.0;
    BdRed r{0.0, 0.0, 0.0, 0.0};
    if (j < n0) bd_tail_point(lam0, m, n0, b, j, lo0, hi0, x, l2 != 0, kin, ds, r);
    ssum = ssum + bd_sum32(ds);
    bd_red_sum32(tot, r);
  }
  if (li == 0) bd_tail_finish(rowacc, ssum, tot, st, m, l2 != 0, eps[b], flag[b] != 0, k == yb, margin_crown, slack);
}

// ------------------------------------------------------------------------------------------------------------------ host twin
static void bd_host(const BdShape& sh, const BdPlan& pl, const float* params, const float* bnstate, const float* x, const float* eps,
                    bool l2, float clip_lo, float clip_hi, const int* y, int batch, float* ws, float* margin_ibp, float* margin_crown,
                    float* slack) {
  const int L = sh.L, C = sh.n[L], n0 = sh.n[0], M = batch * C;
  float* lo = ws + pl.offLo;
  float* hi = ws + pl.offHi;
  int* flag = reinterpret_cast<int*>(ws + pl.offFlag);
  float* colnorm = ws + pl.offNorm;
  // prep
  for (int b = 0; b < batch; ++b) {
    flag[b] = bd_prep_row(eps[b], y[b], C);
    for (int i = 0; i < n0; ++i) flag[b] |= bd_prep_point(x, (size_t)b * n0 + i, eps[b], clip_lo, clip_hi, lo, hi);
  }
  if (l2 && L > 1) {
    const float* W1 = params + sh.offW[0];
    const int n1 = sh.n[1];
    for (int j = 0; j < n1; ++j) {
      double part[kBdNormSlices] = {};
      for (int i = 0; i < n0; ++i) {
        const double w1 = W1[(size_t)i * n1 + j];
        part[i % kBdNormSlices] = part[i % kBdNormSlices] + w1 * w1;
      }
      for (int q = 1; q < kBdNormSlices; ++q) part[0] = part[0] + part[q];
      colnorm[j] = bd_colnorm(part[0]);
    }
  }
  // hidden layers
  std::vector<float> c, r, ac, ar, as;
  for (int l = 0; l + 1 < L; ++l) {
    const int K = sh.n[l], N = sh.n[l + 1];
    const float* W = params + sh.offW[l];
    const float* bias = params + sh.offb[l];
    const BdBn bn = bd_bn(sh, params, bnstate, l);
    const float* ilo = l == 0 ? lo : lo + pl.h[l - 1];
    const float* ihi = l == 0 ? hi : hi + pl.h[l - 1];
    const bool first2 = l2 && l == 0;
    c.assign(K, 0.0f); r.assign(K, 0.0f);
    for (int b = 0; b < batch; ++b) {
      for (int k = 0; k < K; ++k) {
        const size_t at = (size_t)b * K + k;
        if (first2) bd_sym_rad(x[at], ilo[at], ihi[at], c[k], r[k]);
        else bd_mid_rad(ilo[at], ihi[at], c[k], r[k]);
      }
      ac.assign(N, 0.0f); ar.assign(N, 0.0f); as.assign(N, 0.0f);
      for (int k = 0; k < K; ++k) {
        const float ck = c[k], rk = r[k], ak = std::fabs(ck);
        const float* wr = W + (size_t)k * N;
        for (int j = 0; j < N; ++j) {
          const float w = wr[j], aw = std::fabs(w);
          ac[j] = std::fmaf(ck, w, ac[j]);
          ar[j] = std::fmaf(rk, aw, ar[j]);
          as[j] = std::fmaf(ak, aw, as[j]);
        }
      }
      for (int j = 0; j < N; ++j) {
        const size_t at = (size_t)b * N + j;
        float zl, zu, S;
        bd_z_box(ac[j], ar[j], as[j], bias[j], K, first2, first2 ? eps[b] : 0.0f, first2 ? colnorm[j] : 0.0f, zl, zu, S);
        lo[pl.z[l] + at] = zl;
        hi[pl.z[l] + at] = zu;
        ws[pl.offS[l] + at] = S;
        bd_post_box(zl, zu, bd_aff(bn, j), lo[pl.h[l] + at], hi[pl.h[l] + at]);
      }
    }
  }
  // head
  const bool hidden = L > 1;
  const int nh = sh.n[L - 1];
  const float* WL = params + sh.offW[L - 1];
  const float* bL = params + sh.offb[L - 1];
  const float* hl = hidden ? lo + pl.h[L - 2] : lo;
  const float* hu = hidden ? hi + pl.h[L - 2] : hi;
  const bool hl2 = l2 && !hidden;
  double* rowacc = reinterpret_cast<double*>(ws + pl.offAcc);
  float* lam = ws + pl.offLam[0];
  BdRelaxAt rx{false, BdBn{}, nullptr, nullptr, nullptr, nullptr};
  if (hidden) rx = BdRelaxAt{true, bd_bn(sh, params, bnstate, L - 2), lo + pl.z[L - 2], hi + pl.z[L - 2], ws + pl.offS[L - 2], params + sh.offb[L - 2]};
  double vc[32], vs[32];
  BdRed vr[32];
  for (int m = 0; m < M; ++m) {
    const int b = m / C, k = m % C, yb = bd_row_label(flag, y, b);
    double csum = 0.0, ssum = 0.0;
    BdRed tot{0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < nh; j0 += 32) {
      for (int q = 0; q < 32; ++q) {
        const int j = j0 + q;
        vc[q] = vs[q] = 0.0;
        vr[q] = BdRed{0.0, 0.0, 0.0, 0.0};
        if (j < nh)
          bd_head_point(WL, C, nh, b, k, yb, j, hl, hu, hidden ? nullptr : x, hl2, rx, lam[(size_t)m * nh + j], vc[q], vs[q], vr[q]);
      }
      csum = csum + bd_sum32_host(vc);
      ssum = ssum + bd_sum32_host(vs);
      bd_red_sum32_host(tot, vr);
    }
    bd_head_finish(csum, ssum, tot, bL[yb], bL[k], hl2, eps[b], flag[b] != 0, k == yb, rowacc + 2 * (size_t)m, margin_ibp + m);
  }
  if (!margin_crown) return;
  // back
  int cur = 0;
  std::vector<float> acc;
  for (int l = L - 2; l >= 0; --l) {
    const int K = sh.n[l + 1], N = sh.n[l];
    const float* W = params + sh.offW[l];
    const float* A = ws + pl.offLam[cur];
    float* out = ws + pl.offLam[cur ^ 1];
    const bool relax = l > 0;
    const BdBn bn = relax ? bd_bn(sh, params, bnstate, l - 1) : BdBn{};
    double* part = relax ? reinterpret_cast<double*>(ws + pl.offPart[l]) : nullptr;
    const int tiles = pl.tiles[l];
    for (int m = 0; m < M; ++m) {
      acc.assign(N, 0.0f);
      for (int k = 0; k < K; ++k) {
        const float a = A[(size_t)m * K + k];
        for (int i = 0; i < N; ++i) acc[i] = std::fmaf(a, W[(size_t)i * K + k], acc[i]);
      }
      if (!relax) {
        for (int i = 0; i < N; ++i) out[(size_t)m * N + i] = acc[i];
        continue;
      }
      for (int t = 0; t < tiles; ++t) {
        for (int q = 0; q < 32; ++q) {
          const int i = 32 * t + q;
          double dc = 0.0, ds = 0.0;
          if (i < N) {
            const size_t at = (size_t)(m / C) * N + i;
            float nu;
            bd_relax(acc[i], bd_aff(bn, i), lo[pl.z[l - 1] + at], hi[pl.z[l - 1] + at], ws[pl.offS[l - 1] + at],
                     params[sh.offb[l - 1] + i], K, N, nu, dc, ds);
            out[(size_t)m * N + i] = nu;
          }
          vc[q] = dc; vs[q] = ds;
        }
        part[2 * ((size_t)m * tiles + t)] = bd_sum32_host(vc);
        part[2 * ((size_t)m * tiles + t) + 1] = bd_sum32_host(vs);
      }
    }
    cur ^= 1;
  }
  // tail
  const float* lam0 = ws + pl.offLam[cur];
  const int kin = hidden ? sh.n[1] : 0;
  const BdStages stg = bd_stages(sh, pl, ws);
  for (int m = 0; m < M; ++m) {
    const int b = m / C, k = m % C, yb = bd_row_label(flag, y, b);
    double ssum = 0.0;
    BdRed tot{0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < n0; j0 += 32) {
      for (int q = 0; q < 32; ++q) {
        const int j = j0 + q;
        vs[q] = 0.0;
        vr[q] = BdRed{0.0, 0.0, 0.0, 0.0};
        if (j < n0) bd_tail_point(lam0, m, n0, b, j, lo, hi, x, l2, kin, vs[q], vr[q]);
      }
      ssum = ssum + bd_sum32_host(vs);
      bd_red_sum32_host(tot, vr);
    }
    bd_tail_finish(rowacc, ssum, tot, stg, m, l2, eps[b], flag[b] != 0, k == yb, margin_crown, slack);
  }
}

// --------------------------------------------------------------------------------------------------------------------- checks
int bd_shape_from(const char* fn, int n_layers, const int* widths, const int* bn, BdShape* sh) {
  LP_CHECK_ARG(widths != nullptr, "%s: null argument", fn);
  LP_CHECK_ARG(n_layers >= 1 && n_layers <= LIPASR_MAX_LAYERS, "%s: n_layers=%d outside [1,%d]", fn, n_layers, LIPASR_MAX_LAYERS);
  for (int l = 0; l <= n_layers; ++l)
    LP_CHECK_ARG(widths[l] >= 1 && widths[l] <= kBdMaxWidth, "%s: widths[%d]=%d outside [1,%d]", fn, l, widths[l], kBdMaxWidth);
  LP_CHECK_ARG(widths[n_layers] <= 32, "%s: %d classes; at most 32 are supported", fn, widths[n_layers]);
  sh->L = n_layers;
  size_t po = 0, so = 0;
  for (int l = 0; l < n_layers; ++l) {
    const size_t ni = widths[l], no = widths[l + 1];
    sh->n[l] = widths[l];
    sh->bn[l] = l + 1 < n_layers && bn && bn[l];
    // the flat layout of lipasr_mlp_create
    sh->offW[l] = po; po = bd_align4(po + ni * no);
    sh->offb[l] = po; po = bd_align4(po + no);
    if (sh->bn[l]) {
      sh->offg[l] = po; po = bd_align4(po + no);
      sh->offbe[l] = po; po = bd_align4(po + no);
      sh->offmm[l] = so; so = bd_align4(so + no);
      sh->offmv[l] = so; so = bd_align4(so + no);
    }
  }
  sh->n[n_layers] = widths[n_layers];
  sh->n_params = po;
  sh->n_state = so;
  return LIPASR_OK;
}

int bd_shape_of(const char* fn, lipasr_mlp_t m, BdShape* sh) {
  LP_CHECK_ARG(m != nullptr, "%s: null argument", fn);
  sh->L = m->n_layers;
  for (int l = 0; l < m->n_layers; ++l) {
    const MlpLayer& P = m->L[l];
    sh->n[l] = P.n_in;
    sh->n[l + 1] = P.n_out;
    sh->bn[l] = P.bn;
    sh->offW[l] = P.offW; sh->offb[l] = P.offb; sh->offg[l] = P.offg; sh->offbe[l] = P.offbe;
    sh->offmm[l] = P.offmm; sh->offmv[l] = P.offmv;
  }
  sh->n_params = m->n_params;
  sh->n_state = m->n_state;
  for (int l = 0; l <= sh->L; ++l)
    LP_CHECK_ARG(sh->n[l] <= kBdMaxWidth, "%s: a layer of %d units; at most %d are supported", fn, sh->n[l], kBdMaxWidth);
  LP_CHECK_ARG(sh->n[sh->L] <= 32, "%s: %d classes; at most 32 are supported", fn, sh->n[sh->L]);
  return LIPASR_OK;
}

int bd_batch_check(const char* fn, const BdShape& sh, int batch) {
  LP_CHECK_ARG(batch >= 1 && (long long)batch * sh.n[sh.L] <= (1 << 24), "%s: batch %d", fn, batch);
  return LIPASR_OK;
}

int bd_check_spans(const char* fn, const BdSpan* sp, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      LP_CHECK_ARG(!((sp[i].written || sp[j].written) && sp[i].p && sp[j].p && spans_overlap(sp[i].p, sp[i].bytes, sp[j].p, sp[j].bytes)),
                   "%s: an output or the workspace overlaps another argument", fn);
  return LIPASR_OK;
}

static int bd_check(const char* fn, const BdShape& sh, const BdPlan& pl, const float* params, const float* bnstate, const float* x,
                    const float* eps, float norm, float clip_lo, float clip_hi, const int* y, int batch, const float* ws,
                    size_t ws_floats, const float* margin_ibp, const float* margin_crown, const float* slack, const float* layer_lo,
                    const float* layer_hi, bool* l2) {
  LP_CHECK_ARG(params && x && eps && y && ws && margin_ibp, "%s: null argument", fn);
  LP_CHECK_ARG(sh.n_state == 0 || bnstate, "%s: bnstate is null", fn);
  LP_CHECK_ARG(norm == 2.0f || norm == INFINITY, "%s: norm %g; inf and 2 are supported", fn, (double)norm);
  LP_CHECK_ARG(!(clip_lo != clip_lo) && !(clip_hi != clip_hi) && clip_lo <= clip_hi, "%s: clip box [%g, %g]", fn, (double)clip_lo,
               (double)clip_hi);
  LP_CHECK_ARG(!slack || margin_crown, "%s: the slack is that of margin_crown, which is null", fn);
  LP_CHECK_ARG(ws_floats >= pl.total, "%s: workspace of %zu floats; %zu are needed", fn, ws_floats, pl.total);
  *l2 = norm == 2.0f;
  const size_t B = batch, C = sh.n[sh.L];
  const BdSpan sp[] = {{params, sh.n_params * 4, false}, {bnstate, sh.n_state * 4, false}, {x, B * sh.n[0] * 4, false},
                       {eps, B * 4, false}, {y, B * 4, false}, {ws, ws_floats * 4, true}, {margin_ibp, B * C * 4, true},
                       {margin_crown, margin_crown ? B * C * 4 : 0, true}, {slack, slack ? B * C * 4 : 0, true},
                       {layer_lo, layer_lo ? pl.fam * 4 : 0, true}, {layer_hi, layer_hi ? pl.fam * 4 : 0, true}};
  return bd_check_spans(fn, sp, sizeof(sp) / sizeof(sp[0]));
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

long lipasr_debug_bounds_launches(int kernel) { return (kernel >= 0 && kernel < 5) ? g_bounds_launches[kernel] : -1; }

int lipasr_mlp_bounds_workspace(lipasr_mlp_t m, int batch, size_t* floats) {
  const char* fn = "lipasr_mlp_bounds_workspace";
  BdShape sh;
  return bd_workspace(fn, bd_shape_of(fn, m, &sh), sh, batch, floats, bd_plan);
}

int lipasr_mlp_bounds_workspace_host(int n_layers, const int* widths, int batch, size_t* floats) {
  const char* fn = "lipasr_mlp_bounds_workspace_host";
  BdShape sh;
  return bd_workspace(fn, bd_shape_from(fn, n_layers, widths, nullptr, &sh), sh, batch, floats, bd_plan);
}

int lipasr_mlp_bounds(lipasr_mlp_t m, const float* params, const float* bnstate, const float* x, const float* eps, float norm,
                      float clip_lo, float clip_hi, const int* y, int batch, float* workspace, size_t workspace_floats,
                      float* margin_ibp, float* margin_crown, float* slack, float* layer_lo, float* layer_hi, lipasr_stream_t stream) {
  const char* fn = "lipasr_mlp_bounds";
  BdShape sh;
  if (int rc = bd_shape_of(fn, m, &sh)) return rc;
  if (int rc = bd_batch_check(fn, sh, batch)) return rc;
  const BdPlan pl = bd_plan(sh, batch);
  bool l2 = false;
  if (int rc = bd_check(fn, sh, pl, params, bnstate, x, eps, norm, clip_lo, clip_hi, y, batch, workspace, workspace_floats, margin_ibp,
                        margin_crown, slack, layer_lo, layer_hi, &l2))
    return rc;
  DeviceGuard guard(m->ctx->device);
  hipStream_t st = S(stream);
  float* ws = bd_base(workspace);
  const int L = sh.L, C = sh.n[L], n0 = sh.n[0], M = batch * C;
  float* lo = ws + pl.offLo;
  float* hi = ws + pl.offHi;
  int* flag = reinterpret_cast<int*>(ws + pl.offFlag);
  float* colnorm = ws + pl.offNorm;
  const bool hidden = L > 1;
  {
    const bool norms = l2 && hidden;
    const int n1 = hidden ? sh.n[1] : 0;
    const unsigned blocks = (unsigned)batch + (norms ? (unsigned)((n1 + 31) / 32) : 0u);
    hipLaunchKernelGGL(bounds_prep_kernel, dim3(blocks), dim3(kBdThreads), 0, st, x, eps, y, batch, n0, C, clip_lo, clip_hi, lo, hi, flag,
                       params + sh.offW[0], n1, colnorm);
    LP_LAUNCH_CHECK();
    ++g_bounds_launches[BD_PREP];
  }
  for (int l = 0; l + 1 < L; ++l) {
    const int K = sh.n[l], N = sh.n[l + 1];
    const bool first2 = l2 && l == 0;
    hipLaunchKernelGGL(bounds_layer_kernel, dim3((batch + 31) / 32, (N + 127) / 128), dim3(kBdThreads), 0, st,
                       l == 0 ? lo : lo + pl.h[l - 1], l == 0 ? hi : hi + pl.h[l - 1], first2 ? x : nullptr, eps, colnorm,
                       params + sh.offW[l], params + sh.offb[l], bd_bn(sh, params, bnstate, l), batch, K, N, lo + pl.z[l], hi + pl.z[l],
                       ws + pl.offS[l], lo + pl.h[l], hi + pl.h[l]);
    LP_LAUNCH_CHECK();
    ++g_bounds_launches[BD_LAYER];
  }
  double* rowacc = reinterpret_cast<double*>(ws + pl.offAcc);
  const unsigned rowblocks = (unsigned)((M + kBdThreads / 32 - 1) / (kBdThreads / 32));
  {
    const int nh = sh.n[L - 1];
    hipLaunchKernelGGL(bounds_head_kernel, dim3(rowblocks), dim3(kBdThreads), 0, st, params + sh.offW[L - 1], params + sh.offb[L - 1], y,
                       flag, M, C, nh, hidden ? lo + pl.h[L - 2] : lo, hidden ? hi + pl.h[L - 2] : hi, hidden ? nullptr : x, eps,
                       (l2 && !hidden) ? 1 : 0, hidden ? 1 : 0, hidden ? bd_bn(sh, params, bnstate, L - 2) : BdBn{}, hidden ? lo + pl.z[L - 2] : nullptr,
                       hidden ? hi + pl.z[L - 2] : nullptr, hidden ? ws + pl.offS[L - 2] : nullptr,
                       hidden ? params + sh.offb[L - 2] : nullptr, ws + pl.offLam[0], rowacc,
                       margin_ibp);
    LP_LAUNCH_CHECK();
    ++g_bounds_launches[BD_HEAD];
  }
  if (margin_crown) {
    int cur = 0;
    for (int l = L - 2; l >= 0; --l) {
      const int K = sh.n[l + 1], N = sh.n[l];
      const bool relax = l > 0;
      double* part = relax ? reinterpret_cast<double*>(ws + pl.offPart[l]) : nullptr;
      hipLaunchKernelGGL(bounds_back_kernel, dim3((M + 31) / 32, (N + 127) / 128), dim3(kBdThreads), 0, st, ws + pl.offLam[cur],
                         params + sh.offW[l], M, K, N, C, relax ? 1 : 0, relax ? bd_bn(sh, params, bnstate, l - 1) : BdBn{}, relax ? lo + pl.z[l - 1] : nullptr,
                         relax ? hi + pl.z[l - 1] : nullptr, relax ? ws + pl.offS[l - 1] : nullptr,
                         relax ? params + sh.offb[l - 1] : nullptr, ws + pl.offLam[cur ^ 1], part,
                         pl.tiles[l]);
      LP_LAUNCH_CHECK();
      ++g_bounds_launches[BD_BACK];
      cur ^= 1;
    }
    hipLaunchKernelGGL(bounds_tail_kernel, dim3(rowblocks), dim3(kBdThreads), 0, st, ws + pl.offLam[cur], y, flag, M, C, n0,
                       hidden ? sh.n[1] : 0, lo, hi, x, eps, l2 ? 1 : 0, rowacc, bd_stages(sh, pl, ws), margin_crown, slack);
    LP_LAUNCH_CHECK();
    ++g_bounds_launches[BD_TAIL];
  }
  if (layer_lo) LP_HIP(hipMemcpyAsync(layer_lo, lo, pl.fam * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (layer_hi) LP_HIP(hipMemcpyAsync(layer_hi, hi, pl.fam * sizeof(float), hipMemcpyDeviceToDevice, st));
  return LIPASR_OK;
}

int lipasr_mlp_bounds_host(int n_layers, const int* widths, const int* bn, const float* params, const float* bnstate, const float* x,
                           const float* eps, float norm, float clip_lo, float clip_hi, const int* y, int batch, float* workspace,
                           size_t workspace_floats, float* margin_ibp, float* margin_crown, float* slack, float* layer_lo,
                           float* layer_hi) {
  const char* fn = "lipasr_mlp_bounds_host";
  BdShape sh;
  if (int rc = bd_shape_from(fn, n_layers, widths, bn, &sh)) return rc;
  if (int rc = bd_batch_check(fn, sh, batch)) return rc;
  const BdPlan pl = bd_plan(sh, batch);
  bool l2 = false;
  if (int rc = bd_check(fn, sh, pl, params, bnstate, x, eps, norm, clip_lo, clip_hi, y, batch, workspace, workspace_floats, margin_ibp,
                        margin_crown, slack, layer_lo, layer_hi, &l2))
    return rc;
  // the host can look at what the device entry point only flags: eps and y are refused here
  for (int b = 0; b < batch; ++b) {
    LP_CHECK_ARG(eps[b] >= 0.0f, "%s: eps[%d] = %g", fn, b, (double)eps[b]);
    LP_CHECK_ARG(y[b] >= 0 && y[b] < sh.n[sh.L], "%s: y[%d] = %d outside [0,%d)", fn, b, y[b], sh.n[sh.L]);
  }
  float* ws = bd_base(workspace);
  bd_host(sh, pl, params, bnstate, x, eps, l2, clip_lo, clip_hi, y, batch, ws, margin_ibp, margin_crown, slack);
  if (layer_lo) std::memcpy(layer_lo, ws + pl.offLo, pl.fam * sizeof(float));
  if (layer_hi) std::memcpy(layer_hi, ws + pl.offHi, pl.fam * sizeof(float));
  return LIPASR_OK;
}

}  // extern "C"
