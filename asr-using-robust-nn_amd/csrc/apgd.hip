// Auto-PGD (Croce & Hein 2020): the two kernels around the estimator's forward and backward pass in one iteration.
// (include/lipasr.h, lipasr_apgd_loss / lipasr_apgd_step, fixes the conventions; this file says how they are met.)
//
// apgd_loss_kernel: one THREAD per row of logits (classes <= 32): the row is read from memory (L1) as often as the formulas need
//   it, never copied into a private array, and every sum runs over the classes in index order in fp64 -- the same bits on every
//   run.  Cross-entropy in the forms that do not cancel: logsumexp = m + log1p(sum_{c != argmax} exp(z_c - m)), and the
//   gradient at the label is -(sum_{c != y} p_c), not p_y - 1.
//
// apgd_step_kernel<T, NQ>: T threads per row.  A thread owns the quads q = t, t + T, ... of its row (row.h states the row contract).
//     T = 64,  NQ = 1, 2, 4, 8   one wavefront per row, four rows per block, the four row arrays of the step (the start point, its
//                                gradient, the previous iterate, the clean row) in registers, as lp_step_kernel holds its three:
//                                n <= 2 048, the 880 and 2 020 feature rows (NQ 4 and 8).  No LDS, no barrier.
//     T = 512, NQ = 4, 8, 11     one workgroup per row, the row held ONCE in registers across its eight wavefronts (44 floats x 4
//                                arrays per thread at NQ 11): n <= 22 528, the 16 000 and 22 050 sample rows (NQ 8 and 11).  The
//                                three dependent norms of norm 2 -- of the gradient, of the first projection, of the second -- go
//                                wave butterfly -> eight doubles in LDS -> every thread adds them in index order.
//     T = 512, NQ = 0            anything wider: the same arithmetic in the same summation order per thread, the row re-read from
//                                memory in every pass.
//   apgd_instance() is the one selector; lipasr_debug_apgd_path reports it.  The per-row state machine (step size, best loss,
//   counters, checkpoint decisions) is computed by every thread of the row from the same loads, and thread 0 writes it back; the
//   copies into x_best / g_best / x_adv are a loop of their own over the thread's quads before the step loads its working set, and
//   the step never reads an array that loop has written in the same launch.  The element-wise arithmetic of the step is fp64 on
//   the fp32 inputs and rounded once, so that a projection of a point that is already a corner of the ball returns its bits.
//   No atomics, no workspace, nothing waits on another workgroup.  Nothing about its speed has been measured.
#include "common.h"
#include "row.h"

namespace lipasr {

constexpr int kApgdMaxC = 32;
constexpr double kApgdTol = 1e-7;   // ART's tol = 10e-8, as lipasr_lp_step
constexpr double kDlrTol = 1e-12;   // the DLR denominator's, as the paper's authors add it
constexpr int kApgdWgThreads = 512;

__global__ __launch_bounds__(64) void apgd_loss_kernel(const float* __restrict__ logits, const int* __restrict__ labels, int batch,
                                                        int C, int loss_type, int targeted, float* __restrict__ f,
                                                        float* __restrict__ dz, int* __restrict__ hit) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= batch) return;
  const float* __restrict__ r = logits + (size_t)b * C;
  float* __restrict__ d = dz + (size_t)b * C;
  const int y = labels[b];
  bool bad = y < 0 || y >= C;
  float m = -INFINITY;
  int p1 = 0;  // argmax, the lowest index on a tie
  for (int c = 0; c < C; ++c) {
    const float v = r[c];
    bad |= !isfinite(v);
    if (v > m) { m = v; p1 = c; }
  }
  if (bad) {
    f[b] = __int_as_float(0x7fc00000);
    for (int c = 0; c < C; ++c) d[c] = 0.0f;
    hit[b] = 0;
    return;
  }
  hit[b] = targeted ? (p1 == y) : (p1 != y);
  if (loss_type == 0) {
    double s1 = 0.0;  // sum_{c != argmax} exp(z_c - m)
    for (int c = 0; c < C; ++c)
      if (c != p1) s1 += exp((double)r[c] - (double)m);
    const double fv = ((double)m - (double)r[y]) + log1p(s1);
    const double inv = 1.0 / (1.0 + s1);
    double others = 0.0;  // sum_{c != y} p_c
    for (int c = 0; c < C; ++c)
      if (c != y) others += exp((double)r[c] - (double)m) * inv;
    const double sg = targeted ? -1.0 : 1.0;
    for (int c = 0; c < C; ++c) d[c] = (float)(sg * (c == y ? -others : exp((double)r[c] - (double)m) * inv));
    f[b] = (float)(sg * fv);
    return;
  }
  // DLR: the three largest, the lowest index first on ties
  int p2 = -1, p3 = -1;
  float v2 = -INFINITY, v3 = -INFINITY;
  for (int c = 0; c < C; ++c)
    if (c != p1 && r[c] > v2) { v2 = r[c]; p2 = c; }
  for (int c = 0; c < C; ++c)
    if (c != p1 && c != p2 && r[c] > v3) { v3 = r[c]; p3 = c; }
  const int o = p1 != y ? p1 : p2;
  const double D = ((double)r[p1] - (double)r[p3]) + kDlrTol, N = (double)r[y] - (double)r[o];
  const double iD = 1.0 / D, q = N / (D * D);
  for (int c = 0; c < C; ++c) {
    double gd = 0.0;
    if (c == y) gd -= iD;
    if (c == o) gd += iD;
    if (c == p1) gd += q;
    if (c == p3) gd -= q;
    d[c] = (float)gd;
  }
  f[b] = (float)(-N / D);
}

struct ApgdArgs {
  float* x; float* x_prev; const float* x0; const float* g; float* x_best; float* g_best; float* x_adv;
  const float* f; const int* hit; const int* n_valid;
  float* eta; float* f_best; float* f_prev; float* f_best_ckpt; int* improved; int* reduced_last; int* fooled; int* halvings;
  int rows, n, norm2, flags, ckpt_len, vec;
  float eps, eta0, lo, hi, momentum, rho;
};

template <int T, int NQ>
__global__ __launch_bounds__(T == 64 ? 256 : T) void apgd_step_kernel(ApgdArgs a) {
  __shared__ double red[T == 64 ? 1 : T / 64];
  const int t = T == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  const int row = T == 64 ? (int)(blockIdx.x * 4 + (threadIdx.x >> 6)) : (int)blockIdx.x;
  if (row >= a.rows) return;  // uniform over the row's threads; a T = 64 block never meets a barrier
  const int n = a.n;
  const bool vec = a.vec != 0;  // n is a multiple of 4 and every base sits on 16 bytes: each quad is whole
  const size_t base = (size_t)row * n;
  const int nv = row_valid(a.n_valid, row, n);
  const int quads = (n + 3) >> 2;
  const bool first = (a.flags & 1) != 0, last = (a.flags & 2) != 0;

  // ---- 1. bookkeeping at x: every thread of the row computes the same state from the same loads
  const float fr = a.f[row];
  const bool hitr = a.hit[row] != 0;
  float eta, f_best, f_prev, f_ckpt;
  int improved, reduced, fooled, halv;
  bool upd_best;
  if (first) {
    const float f0 = fr != fr ? -INFINITY : fr;
    eta = a.eta0;
    f_best = f_prev = f_ckpt = f0;
    improved = reduced = fooled = halv = 0;
    upd_best = true;
  } else {
    eta = a.eta[row]; f_best = a.f_best[row]; f_prev = a.f_prev[row]; f_ckpt = a.f_best_ckpt[row];
    improved = a.improved[row]; reduced = a.reduced_last[row]; fooled = a.fooled[row]; halv = a.halvings[row];
    if (fr > f_prev) ++improved;
    f_prev = fr;
    upd_best = fr > f_best;
    if (upd_best) f_best = fr;
  }
  if (hitr) fooled = 1;
  if constexpr (T > 64) __syncthreads();  // every thread has read the state before thread 0 writes it

  if (upd_best || hitr) {  // x_best <- x, g_best <- g, x_adv <- x; the padding takes the bits of x0
    for (int q = t; q < quads; q += T) {
      const int k0 = 4 * q;
      float xv[4], cv[4];
      ld4(a.x0 + base, k0, n, vec, cv);
      ld4(a.x + base, k0, n, vec, xv);
#pragma unroll
      for (int e = 0; e < 4; ++e) xv[e] = (k0 + e < nv) ? xv[e] : cv[e];
      if (hitr) st4(a.x_adv + base, k0, n, vec, xv);
      if (upd_best) {
        st4(a.x_best + base, k0, n, vec, xv);
        float gv[4];
        ld4(a.g + base, k0, n, vec, gv);
#pragma unroll
        for (int e = 0; e < 4; ++e) gv[e] = (k0 + e < nv) ? gv[e] : cv[e];
        st4(a.g_best + base, k0, n, vec, gv);
      }
    }
  }

  // ---- 2. LAST (and a row without a clip) stops here; 3. the checkpoint
  const bool stop = last || nv == 0;
  bool restart = false;
  if (!stop && a.ckpt_len > 0) {
    const bool c1 = (double)improved < (double)a.rho * (double)a.ckpt_len;
    const bool c2 = reduced == 0 && f_ckpt == f_best;
    restart = c1 || c2;
    if (restart) { eta *= 0.5f; ++halv; reduced = 1; } else { reduced = 0; }
    improved = 0;
    f_ckpt = f_best;
  }
  if (t == 0) {
    a.eta[row] = eta; a.f_best[row] = f_best; a.f_prev[row] = f_prev; a.f_best_ckpt[row] = f_ckpt;
    a.improved[row] = improved; a.reduced_last[row] = reduced; a.fooled[row] = fooled; a.halvings[row] = halv;
  }
  if (stop) return;

  // ---- 4. the step from (xc, gc, xp).  A restart whose best point is x itself (just copied above) starts from x: the step never
  // reads what this launch has written.
  const bool from_best = restart && !upd_best;
  const float* __restrict__ xs = (from_best ? a.x_best : a.x) + base;
  const float* __restrict__ gs = (from_best ? a.g_best : a.g) + base;
  const bool no_mom = restart || first;  // xp := xc: no momentum term (on FIRST x_prev is not read at all)
  const double am = first ? 1.0 : (double)a.momentum, bm = 1.0 - am;
  const double etad = (double)eta, epsd = (double)a.eps, lo = (double)a.lo, hi = (double)a.hi;
  const bool l2 = a.norm2 != 0;

  constexpr int R = NQ > 0 ? NQ : 1;
  float XC[R][4], GC[R][4], XP[R][4], X0[R][4];
  auto fetch = [&](int s, int q) {
    if (q < quads) {
      const int k0 = 4 * q;
      ld4(xs, k0, n, vec, XC[s]);
      ld4(gs, k0, n, vec, GC[s]);
      ld4(a.x0 + base, k0, n, vec, X0[s]);
      if (no_mom) {
#pragma unroll
        for (int e = 0; e < 4; ++e) XP[s][e] = XC[s][e];
      } else {
        ld4(a.x_prev + base, k0, n, vec, XP[s]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) GC[s][e] = GC[s][e] != GC[s][e] ? 0.0f : GC[s][e];  // NaN -> 0
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) XC[s][e] = GC[s][e] = XP[s][e] = X0[s][e] = 0.0f;
    }
  };
  const int nj = (quads + T - 1) / T;
  auto for_quads = [&](auto&& body) {  // body(slot, quad): NQ > 0 from registers, NQ == 0 re-reading
    if constexpr (NQ > 0) {
#pragma unroll
      for (int j = 0; j < NQ; ++j) body(j, t + T * j);
    } else {
      for (int j = 0; j < nj; ++j) {
        fetch(0, t + T * j);
        body(0, t + T * j);
      }
    }
  };
  if constexpr (NQ > 0) {
#pragma unroll
    for (int j = 0; j < NQ; ++j) fetch(j, t + T * j);
  }

  double kdir = 0.0;
  if (l2) {
    double s = 0.0;
    for_quads([&](int sl, int q) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * q + e < nv) s += (double)GC[sl][e] * (double)GC[sl][e];
    });
    const double nrm = sqrt(block_sum_d<T>(s, red));
    kdir = isfinite(nrm) ? 1.0 / (nrm + kApgdTol) : 0.0;
  }
  // u = clamp(xc + eta d) - x0, the argument of the first projection
  auto dl1 = [&](int sl, int e) {
    const float gq = GC[sl][e];
    const double d = l2 ? (isfinite(gq) ? (double)gq * kdir : 0.0) : (gq > 0.0f ? 1.0 : (gq < 0.0f ? -1.0 : 0.0));
    return clampf((double)XC[sl][e] + etad * d, lo, hi) - (double)X0[sl][e];
  };
  double fz = 1.0;
  if (l2) {
    double s = 0.0;
    for_quads([&](int sl, int q) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * q + e < nv) { const double dl = dl1(sl, e); s += dl * dl; }
    });
    fz = fmin(1.0, epsd / (sqrt(block_sum_d<T>(s, red)) + kApgdTol));
  }
  // the argument of the second projection: clamp(xc + a (z - xc) + (1 - a)(xc - xp)) - x0
  auto dl2 = [&](int sl, int e) {
    const double dl = dl1(sl, e), c = (double)X0[sl][e], xc = (double)XC[sl][e];
    const double z = c + (l2 ? dl * fz : clampf(dl, -epsd, epsd));
    const double v = xc + am * (z - xc) + bm * (xc - (double)XP[sl][e]);
    return clampf(v, lo, hi) - c;
  };
  double fv = 1.0;
  if (l2) {
    double s = 0.0;
    for_quads([&](int sl, int q) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * q + e < nv) { const double dl = dl2(sl, e); s += dl * dl; }
    });
    fv = fmin(1.0, epsd / (sqrt(block_sum_d<T>(s, red)) + kApgdTol));
  }
  for_quads([&](int sl, int q) {
    if (q >= quads) return;
    const int k0 = 4 * q;
    float xn[4], xo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = k0 + e < nv;
      const double dl = dl2(sl, e), c = (double)X0[sl][e];
      xn[e] = in ? (float)(c + (l2 ? dl * fv : clampf(dl, -epsd, epsd))) : X0[sl][e];
      xo[e] = in ? XC[sl][e] : X0[sl][e];
    }
    st4(a.x_prev + base, k0, n, vec, xo);
    st4(a.x + base, k0, n, vec, xn);
  });
}

// The one selector: the instance a row width takes.  0 .. 3: a wavefront per row, 1 / 2 / 4 / 8 quads per lane (n <= 256, 512,
// 1 024, 2 048); 4 .. 6: a workgroup per row, 4 / 8 / 11 quads per thread (n <= 8 192, 16 384, 22 528); 7: the re-reading fallback.
static int apgd_instance(int n) {
  if (n <= 256) return 0;
  if (n <= 512) return 1;
  if (n <= 1024) return 2;
  if (n <= 2048) return 3;
  if (n <= 4 * 4 * kApgdWgThreads) return 4;
  if (n <= 4 * 8 * kApgdWgThreads) return 5;
  if (n <= 4 * 11 * kApgdWgThreads) return 6;
  return 7;
}

template <int T, int NQ>
static void apgd_launch(const ApgdArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)(T == 64 ? (a.rows + 3) / 4 : a.rows));
  hipLaunchKernelGGL((apgd_step_kernel<T, NQ>), grid, dim3(T == 64 ? 256 : T), 0, st, a);
}

struct ApgdSpan { const void* p; size_t bytes; bool written; const char* name; };

}  // namespace lipasr

using namespace lipasr;

extern "C" {

int lipasr_debug_apgd_path(int n, int aligned) {
  if (n <= 0) return -1;
  return apgd_instance(n) | ((aligned && n % 4 == 0) ? 8 : 0);
}

int lipasr_apgd_loss(lipasr_handle_t h, const float* logits, const int* labels, int batch, int classes, int loss_type, int targeted,
                     float* f, float* dz, int* hit, lipasr_stream_t stream) {
  const char* fn = "lipasr_apgd_loss";
  LP_CHECK_ARG(classes >= 1 && classes <= kApgdMaxC, "%s: %d classes; 1 to %d are supported", fn, classes, kApgdMaxC);
  LP_CHECK_ARG(loss_type == 0 || loss_type == 1, "%s: loss_type %d; 0 (cross-entropy) or 1 (DLR)", fn, loss_type);
  LP_CHECK_ARG(loss_type == 0 || !targeted, "%s: the DLR loss is untargeted only", fn);
  LP_CHECK_ARG(loss_type == 0 || classes >= 3, "%s: the DLR loss needs at least 3 classes, got %d", fn, classes);
  LP_CHECK_ARG(batch >= 0, "%s: batch %d", fn, batch);
  LP_CHECK_ARG(h != nullptr, "%s: null handle", fn);
  if (batch == 0) return LIPASR_OK;
  LP_CHECK_ARG(logits != nullptr && labels != nullptr && f != nullptr && dz != nullptr && hit != nullptr, "%s: a null pointer", fn);
  hipLaunchKernelGGL(apgd_loss_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, S(stream), logits, labels, batch, classes,
                     loss_type, targeted ? 1 : 0, f, dz, hit);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_apgd_step(lipasr_handle_t h, float* x, float* x_prev, const float* x0, const float* g, float* x_best, float* g_best,
                     float* x_adv, const float* f, const int* hit, const int* n_valid, float* eta, float* f_best, float* f_prev,
                     float* f_best_ckpt, int* improved, int* reduced_last, int* fooled, int* halvings, int rows, int n, float norm,
                     float eps, float eta0, float clip_lo, float clip_hi, float momentum, float rho, int flags, int ckpt_len,
                     lipasr_stream_t stream) {
  const char* fn = "lipasr_apgd_step";
  LP_CHECK_ARG(rows >= 0 && n >= 0, "%s: bad shape %d x %d", fn, rows, n);
  LP_CHECK_ARG(norm == 2.0f || (std::isinf(norm) && norm > 0.0f), "%s: norm=%g; 2 and inf are supported", fn, (double)norm);
  LP_CHECK_ARG(eps >= 0.0f && eps < INFINITY, "%s: eps %g", fn, (double)eps);
  LP_CHECK_ARG(eta0 >= 0.0f && eta0 < INFINITY, "%s: eta0 %g", fn, (double)eta0);
  LP_CHECK_ARG(clip_lo <= clip_hi, "%s: clip range [%g, %g]", fn, (double)clip_lo, (double)clip_hi);
  LP_CHECK_ARG(momentum >= 0.0f && momentum <= 1.0f && rho >= 0.0f && rho <= 1.0f, "%s: momentum %g, rho %g; both in [0, 1]", fn,
               (double)momentum, (double)rho);
  LP_CHECK_ARG((flags & ~3) == 0 && ckpt_len >= 0, "%s: flags %d, ckpt_len %d", fn, flags, ckpt_len);
  LP_CHECK_ARG(!((flags & LIPASR_APGD_FIRST) && ckpt_len > 0), "%s: the first iteration is no checkpoint", fn);
  LP_CHECK_ARG(h != nullptr, "%s: null handle", fn);
  if (rows == 0 || n == 0) return LIPASR_OK;
  LP_CHECK_ARG(x && x_prev && x0 && g && x_best && g_best && x_adv && f && hit && eta && f_best && f_prev && f_best_ckpt && improved &&
                   reduced_last && fooled && halvings,
               "%s: a null pointer", fn);
  const size_t rb = (size_t)rows * n * sizeof(float), sb = (size_t)rows * 4;
  const ApgdSpan sp[] = {{x, rb, true, "x"}, {x_prev, rb, true, "x_prev"}, {x0, rb, false, "x0"}, {g, rb, false, "g"},
                         {x_best, rb, true, "x_best"}, {g_best, rb, true, "g_best"}, {x_adv, rb, true, "x_adv"}, {f, sb, false, "f"},
                         {hit, sb, false, "hit"}, {n_valid, n_valid ? sb : 0, false, "n_valid"}, {eta, sb, true, "eta"},
                         {f_best, sb, true, "f_best"}, {f_prev, sb, true, "f_prev"}, {f_best_ckpt, sb, true, "f_best_ckpt"},
                         {improved, sb, true, "improved"}, {reduced_last, sb, true, "reduced_last"}, {fooled, sb, true, "fooled"},
                         {halvings, sb, true, "halvings"}};
  constexpr int ns = (int)(sizeof(sp) / sizeof(sp[0]));
  for (int i = 0; i < ns; ++i)
    for (int j = i + 1; j < ns; ++j) {
      if (!(sp[i].written || sp[j].written)) continue;
      LP_CHECK_ARG(!spans_overlap(sp[i].p, sp[i].bytes, sp[j].p, sp[j].bytes), "%s: %s overlaps %s", fn, sp[i].name, sp[j].name);
    }
  ApgdArgs a;
  a.x = x; a.x_prev = x_prev; a.x0 = x0; a.g = g; a.x_best = x_best; a.g_best = g_best; a.x_adv = x_adv;
  a.f = f; a.hit = hit; a.n_valid = n_valid;
  a.eta = eta; a.f_best = f_best; a.f_prev = f_prev; a.f_best_ckpt = f_best_ckpt;
  a.improved = improved; a.reduced_last = reduced_last; a.fooled = fooled; a.halvings = halvings;
  a.rows = rows; a.n = n; a.norm2 = norm == 2.0f ? 1 : 0; a.flags = flags; a.ckpt_len = ckpt_len;
  a.eps = eps; a.eta0 = eta0; a.lo = clip_lo; a.hi = clip_hi; a.momentum = momentum; a.rho = rho;
  uintptr_t bits = 0;
  for (int i = 0; i < 7; ++i) bits |= reinterpret_cast<uintptr_t>(sp[i].p);
  a.vec = (n % 4 == 0 && (bits & 15) == 0) ? 1 : 0;
  const hipStream_t st = S(stream);
  switch (apgd_instance(n)) {
    case 0: apgd_launch<64, 1>(a, st); break;
    case 1: apgd_launch<64, 2>(a, st); break;
    case 2: apgd_launch<64, 4>(a, st); break;   // 880
    case 3: apgd_launch<64, 8>(a, st); break;   // 2 020
    case 4: apgd_launch<kApgdWgThreads, 4>(a, st); break;
    case 5: apgd_launch<kApgdWgThreads, 8>(a, st); break;   // 16 000
    case 6: apgd_launch<kApgdWgThreads, 11>(a, st); break;  // 22 050
    default: apgd_launch<kApgdWgThreads, 0>(a, st); break;
  }
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

}  // extern "C"
