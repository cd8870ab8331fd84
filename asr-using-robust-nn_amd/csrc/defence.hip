// Input-transformation defences over audio (lipasr/defences.py, estimators.DefendedClassifier): a chain of 1 to 4 stages over rows
// x [clips][n], applied in one launch, and the chain's vector-Jacobian product in one launch.  (include/lipasr.h,
// lipasr_defence_apply, fixes the formulas.)
//
//   median k     out[t] = the element of rank (k - 1) / 2 of x[t - h .. t + h], ordered by (value, position); h = (k - 1) / 2
//   fir taps     out[t] = sum_k h[k] x[t + c - k], c = (taps - 1) / 2, an fmaf chain in ascending k from 0
//   quantize b   out[t] = clamp(rintf(x[t] q), -q, q - 1) / q, q = 2^(b - 1)
//
// Every stage reads its input as 0 outside [0, nv) and writes exactly 0 there, so the chain is the composition of its stages.
//
// defence_apply_kernel: 256 threads own (a clip, a tile of kDefTile = 1 024 output positions).  With H the sum of the chain's
//   half-widths, the workgroup stages x over [t0 - H, t0 + 1 024 + H) and walks the stages between two LDS buffers; stage i is
//   valid on a range that is h_i narrower at either end than its input, so after the last one the tile itself is left.
// defence_vjp_kernel: the same tile of gx.  The cotangent of stage i's output is needed over the tile +- (h_1 + .. + h_i), and the
//   selection of a median there reads that stage's input h_i further out: the forward pass is recomputed from x over
//   [t0 - 2 H, t0 + 1 024 + 2 H), up to the last median or quantiser (a FIR needs nothing of it).  What the backward pass needs
//   of it is one byte per (stage, position): the offset of the element a median selected, or whether a quantiser's clamp was
//   idle.  Then g is staged over the tile +- H and walks the stages in reverse through the same two buffers.
//   LDS: apply 2 x (1 024 + 2 H) floats = 12 kB at H = 256; vjp 2 x (1 024 + 4 H) floats + 4 x (1 024 + 2 H) bytes = 22 kB;
//   both 1 kB more for the taps of the FIR stage at work.
//   kDefMaxHalo = 256 follows from the tile: the recomputed range is at most twice the tile.
// A lane of the median reads its window at consecutive LDS addresses and neighbouring lanes read neighbouring windows, so every
// ds_read_b32 is conflict-free.  A lane of the FIR owns four neighbouring outputs and reads aligned float4 chunks, neighbouring
// lanes neighbouring chunks (ds_read_b128, conflict-free, 16 fmaf each); its taps are staged in LDS and read at wave-uniform
// addresses (broadcasts).  Measured against one output, one ds_read_b32 and one tap from memory per fmaf:
// profiles/defence_timing.txt.
// Every output element is its own chain over values that do not depend on the tile, so the grid cannot change a bit, and the host
// twins run the same inline functions (for the FIR: the same chain, element by element) over whole rows.  Loads and stores are guarded single floats: any n, any alignment.
// Nothing here allocates, synchronises, uses an atomic or waits on another workgroup.
#include "common.h"
#include "row.h"

#pragma clang fp contract(off)

namespace lipasr {

constexpr int kDefTile = 1024;
constexpr int kDefThreads = 256;
constexpr int kDefMaxHalo = LIPASR_DEFENCE_MAX_HALO;
constexpr int kDefMaxStages = LIPASR_DEFENCE_MAX_STAGES;
constexpr int kDefApplyLen = kDefTile + 2 * kDefMaxHalo;  // staged positions of the forward launch, and of g
constexpr int kDefVjpLen = kDefTile + 4 * kDefMaxHalo;    // staged positions of the recomputed forward pass
constexpr int kDefTapsLds = 272;  // a FIR stage's taps in LDS: a pad of at most 3, 255 taps, and the float4 a chunk reads past them
constexpr int kDefMaxN = 1 << 30;
constexpr signed char kDefDropped = 127;  // a median whose selected element is a padding zero, or an output outside the clip
static_assert(kDefApplyLen % 4 == 0 && kDefVjpLen % 4 == 0, "the LDS buffers are read as float4");
static_assert(kDefMaxHalo == 256 && kDefMaxStages == 4, "include/lipasr.h states the limits");
static_assert((2 * kDefVjpLen + kDefTapsLds) * sizeof(float) + kDefMaxStages * kDefApplyLen <= 48 * 1024, "static LDS of the vjp kernel");

long g_defence_launches[2] = {};

struct DefStage {
  int kind, arg, half;
  const float* taps;
};
struct DefChain {
  int stages, halo;
  int routed;  // the stages up to the last median or quantiser: as far as the backward launch recomputes the forward pass
  DefStage s[kDefMaxStages];
};

// ------------------------------------------------------------------------------------------- one element of one stage
// w[j] is the element at position t - h + j; the j whose element has rank (K - 1) / 2 under (value, position).  A pair i < j is
// compared once: i comes first unless w[j] < w[i], so w[i] <= w[j] (a tie included) adds to j's rank and the opposite to i's; the
// ranks are a permutation of 0 .. K - 1 on finite input.
template <int K>
__host__ __device__ __forceinline__ int def_median_pick_k(const float* w) {
  float v[K];
  int r[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    v[j] = w[j];
    r[j] = 0;
  }
#pragma unroll
  for (int j = 1; j < K; ++j) {
#pragma unroll
    for (int i = 0; i < j; ++i) {
      const int first = v[i] <= v[j] ? 1 : 0;
      r[j] += first;
      r[i] += 1 - first;
    }
  }
  int sel = (K - 1) / 2;
#pragma unroll
  for (int j = 0; j < K; ++j) sel = r[j] == (K - 1) / 2 ? j : sel;
  return sel;
}

__host__ __device__ __forceinline__ int def_median_pick(const float* w, int k) {
  switch (k) {
    case 3: return def_median_pick_k<3>(w);
    case 5: return def_median_pick_k<5>(w);
    case 7: return def_median_pick_k<7>(w);
    case 9: return def_median_pick_k<9>(w);
    case 11: return def_median_pick_k<11>(w);
    case 13: return def_median_pick_k<13>(w);
    default: return def_median_pick_k<15>(w);
  }
}

// xc points at position t
__host__ __device__ __forceinline__ float def_fir_at(const float* xc, const float* __restrict__ h, int taps) {
  const int c = (taps - 1) >> 1;
  float acc = 0.0f;
  for (int k = 0; k < taps; ++k) acc = fmaf(h[k], xc[c - k], acc);
  return acc;
}

// gc points at position s
__host__ __device__ __forceinline__ float def_fir_adj_at(const float* gc, const float* __restrict__ h, int taps) {
  const int c = (taps - 1) >> 1;
  float acc = 0.0f;
  for (int k = 0; k < taps; ++k) acc = fmaf(h[k], gc[k - c], acc);
  return acc;
}

__host__ __device__ __forceinline__ float def_quantize(float x, float q, bool& idle) {
  const float r = rintf(x * q);
  idle = r >= -q && r <= q - 1.0f;
  return clampf(r, -q, q - 1.0f) * (1.0f / q);
}

// gin points at position s, sel at the selection bytes of position s: the cotangents of the outputs that selected s, in ascending t
__host__ __device__ __forceinline__ float def_median_adj_at(const float* gin, const signed char* sel, int h) {
  float acc = 0.0f;
  for (int d = -h; d <= h; ++d)
    if (sel[d] == (signed char)(-d)) acc = acc + gin[d];
  return acc;
}

// stage `st` at position p of the clip [0, nv); src points at position p of the stage's input (zeros outside the clip).
// route: what the backward pass needs of this element.
__host__ __device__ __forceinline__ float def_stage_at(const DefStage& st, const float* src, int p, int nv, signed char& route) {
  route = st.kind == LIPASR_DEFENCE_MEDIAN ? kDefDropped : 0;
  if (p < 0 || p >= nv) return 0.0f;
  if (st.kind == LIPASR_DEFENCE_MEDIAN) {
    const int j = def_median_pick(src - st.half, st.arg);
    const int s = p - st.half + j;
    if (s >= 0 && s < nv) route = (signed char)(j - st.half);
    return src[j - st.half];
  }
  if (st.kind == LIPASR_DEFENCE_FIR) return def_fir_at(src, st.taps, st.arg);
  bool idle;
  const float v = def_quantize(src[0], (float)(1 << (st.arg - 1)), idle);
  route = idle ? 1 : 0;
  return v;
}

// the adjoint of stage `st` at input position s; gin points at position s of the cotangent of the stage's output (zeros outside
// the clip), rt at the stage's route bytes of position s
__host__ __device__ __forceinline__ float def_stage_adj_at(const DefStage& st, const float* gin, const signed char* rt, int s, int nv) {
  if (s < 0 || s >= nv) return 0.0f;
  if (st.kind == LIPASR_DEFENCE_MEDIAN) return def_median_adj_at(gin, rt, st.half);
  if (st.kind == LIPASR_DEFENCE_FIR) return def_fir_adj_at(gin, st.taps, st.arg);
  return rt[0] ? gin[0] : 0.0f;
}

// ------------------------------------------------------------------------------------------------------------ kernels
// buf[idx] = row[base + idx] inside the clip, 0 outside, idx in [0, len)
__device__ __forceinline__ void def_stage_in(const float* __restrict__ row, int base, int len, int nv, float* buf) {
  for (int idx = threadIdx.x; idx < len; idx += kDefThreads) {
    const int p = base + idx;
    buf[idx] = (p >= 0 && p < nv) ? row[p] : 0.0f;
  }
}

// A FIR stage (ADJ: its adjoint) over the buffer indices [lo, hi): a thread takes four neighbouring outputs, idx 4 q .. 4 q + 3,
// and reads the input as aligned float4 chunks, chunk q + r for a wave-uniform r: 16 fmaf per ds_read_b128.  Output j takes the
// chunk's element e (position 4 (q + r) + e) at tap k = j + c - 4 r - e (ADJ: 4 r + e - j + c); the chunks run downwards (ADJ:
// upwards), so every output's chain is def_fir_at's (def_fir_adj_at's) ascending-k chain over every k.  The taps are staged in hs
// behind a pad P = (3 - c) mod 4, which puts the seven taps a chunk needs, k0 .. k0 + 6 with k0 = c - 3 -+ 4 r, on a 16-byte
// boundary: two broadcast ds_read_b128.  (Read from memory the taps came as one global load and one wait per fmaf.)  A chunk at
// the ends of the window, where some (j, e) has no tap, takes them one by one.  An output outside [lo, hi) is computed from
// whatever its window holds and not stored; a chunk outside the buffer's `quads` chunks is needed by no stored output and is read
// as zeros.  The caller has passed a barrier since hs was last read.
template <bool ADJ>
__device__ __forceinline__ void def_fir_stage(const float* a, float* b, int quads, int lo, int hi, int base, int nv,
                                              const float* __restrict__ h, int taps, float* hs) {
  const int c = (taps - 1) >> 1;
  const int P = (3 - c) & 3;
  for (int k = threadIdx.x; k < kDefTapsLds; k += kDefThreads) hs[k] = (k >= P && k - P < taps) ? h[k - P] : 0.0f;
  __syncthreads();
  const int reach = (c + 3) >> 2;  // chunks to either side that hold a tap of some output
  const int inner = c >= 3 ? (c - 3) >> 2 : -1;  // |r| <= inner: 4 r + 3 <= c and 4 r - 3 >= -c, every (j, e) has a tap
  const int s1 = inner < 0 ? 2 * reach + 1 : reach - inner, s2 = inner < 0 ? 2 * reach + 1 : reach + inner + 1;
  const float4* a4 = reinterpret_cast<const float4*>(a);
  const float4* hs4 = reinterpret_cast<const float4*>(hs);
  for (int q = (lo >> 2) + (int)threadIdx.x; 4 * q < hi; q += kDefThreads) {
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (base + 4 * q < nv && base + 4 * q + 3 >= 0) {  // else: no output of the four lies inside the clip
      // chunk number s of the window, r = +-(s - reach); k0: its lowest tap, of (j, e) = (0, 3), ADJ (3, 0)
      auto load = [&](int s, int& k0) {
        const int r = ADJ ? s - reach : reach - s;
        const int m = q + r;
        k0 = c - 3 + (ADJ ? 4 * r : -4 * r);
        return (m >= 0 && m < quads) ? a4[m] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      };
      auto edge = [&](int s) {  // some (j, e) of the chunk has no tap
        int k0;
        const float4 t = load(s, k0);
        const float v[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int ee = 0; ee < 4; ++ee) {
          const int e = ADJ ? ee : 3 - ee;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int k = k0 + (ADJ ? e + 3 - j : j + 3 - e);
            if (k >= 0 && k < taps) acc[j] = fmaf(hs[P + k], v[e], acc[j]);
          }
        }
      };
      for (int s = 0; s < s1; ++s) edge(s);
#pragma unroll 4
      for (int s = s1; s < s2; ++s) {  // every (j, e) of the chunk has a tap: no branch, so the loads of the next chunks are in flight
        int k0;
        const float4 t = load(s, k0);
        const float v[4] = {t.x, t.y, t.z, t.w};
        const float4 wa = hs4[(k0 + P) >> 2], wb = hs4[((k0 + P) >> 2) + 1];
        const float w[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
        for (int ee = 0; ee < 4; ++ee) {
          const int e = ADJ ? ee : 3 - ee;
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] = fmaf(w[ADJ ? e + 3 - j : j + 3 - e], v[e], acc[j]);
        }
      }
      for (int s = s2; s <= 2 * reach; ++s) edge(s);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int idx = 4 * q + j, p = base + idx;
      if (idx >= lo && idx < hi) b[idx] = (p >= 0 && p < nv) ? acc[j] : 0.0f;
    }
  }
}

// The forward chain over LDS.  a holds the input at positions base + [0, len); the result is returned (a or b) and is valid at
// idx in [halo, len - halo) (of the first `stages` stages: all of them, or as many as the backward pass needs); both buffers hold
// `quads` aligned float4.  ROUTE: the route byte of stage i at position p goes to route[i][p - rbase] for p in the tile
// +- (h_1 + .. + h_i), rbase = t0 - halo.
template <bool ROUTE>
__device__ __forceinline__ float* def_forward(const DefChain& ch, int stages, float* a, float* b, int quads, int base, int len, int nv, int t0,
                                              signed char (*route)[kDefApplyLen], float* hs) {
  int lo = 0, hi = len, reach = 0;
  for (int i = 0; i < stages; ++i) {
    const DefStage st = ch.s[i];
    lo += st.half;
    hi -= st.half;
    reach += st.half;
    __syncthreads();  // a is written
    if (st.kind == LIPASR_DEFENCE_FIR) {  // nothing of it is needed on the way back
      def_fir_stage<false>(a, b, quads, lo, hi, base, nv, st.taps, st.arg, hs);
    } else {
      for (int idx = lo + (int)threadIdx.x; idx < hi; idx += kDefThreads) {
        const int p = base + idx;
        signed char r;
        b[idx] = def_stage_at(st, a + idx, p, nv, r);
        if (ROUTE && p >= t0 - reach && p < t0 + kDefTile + reach) route[i][p - (t0 - ch.halo)] = r;
      }
    }
    float* t = a;
    a = b;
    b = t;
  }
  return a;
}

__global__ __launch_bounds__(kDefThreads) void defence_apply_kernel(const float* __restrict__ x, const int* __restrict__ n_valid,
                                                                    DefChain ch, int n, int tiles, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float bufs[2][kDefApplyLen];
  __shared__ __attribute__((aligned(16))) float hs[kDefTapsLds];
  const int clip = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * kDefTile;
  const int nv = row_valid(n_valid, clip, n);
  const int tend = min(t0 + kDefTile, n);
  float* orow = out + (size_t)clip * n;
  if (t0 >= nv) {  // the whole tile lies beyond the clip
    for (int t = t0 + threadIdx.x; t < tend; t += kDefThreads) orow[t] = 0.0f;
    return;
  }
  const int base = t0 - ch.halo, len = kDefTile + 2 * ch.halo;
  def_stage_in(x + (size_t)clip * n, base, len, nv, bufs[0]);
  const float* res = def_forward<false>(ch, ch.stages, bufs[0], bufs[1], kDefApplyLen / 4, base, len, nv, t0, nullptr, hs);
  __syncthreads();
  for (int t = t0 + threadIdx.x; t < tend; t += kDefThreads) orow[t] = res[t - base];
}

__global__ __launch_bounds__(kDefThreads) void defence_vjp_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                  const int* __restrict__ n_valid, DefChain ch, int n, int tiles,
                                                                  float* __restrict__ gx) {
  __shared__ __attribute__((aligned(16))) float bufs[2][kDefVjpLen];
  __shared__ __attribute__((aligned(16))) float hs[kDefTapsLds];
  __shared__ signed char route[kDefMaxStages][kDefApplyLen];
  const int clip = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * kDefTile;
  const int nv = row_valid(n_valid, clip, n);
  const int tend = min(t0 + kDefTile, n);
  float* orow = gx + (size_t)clip * n;
  if (t0 >= nv) {
    for (int t = t0 + threadIdx.x; t < tend; t += kDefThreads) orow[t] = 0.0f;
    return;
  }
  if (ch.routed > 0) def_stage_in(x + (size_t)clip * n, t0 - 2 * ch.halo, kDefTile + 4 * ch.halo, nv, bufs[0]);
  def_forward<true>(ch, ch.routed, bufs[0], bufs[1], kDefVjpLen / 4, t0 - 2 * ch.halo, kDefTile + 4 * ch.halo, nv, t0, route, hs);
  __syncthreads();  // the forward pass is read; its buffers now carry the cotangent
  const int base = t0 - ch.halo, len = kDefTile + 2 * ch.halo;
  float *a = bufs[0], *b = bufs[1];
  def_stage_in(g + (size_t)clip * n, base, len, nv, a);
  int lo = 0, hi = len;
  for (int i = ch.stages - 1; i >= 0; --i) {
    const DefStage st = ch.s[i];
    lo += st.half;
    hi -= st.half;
    __syncthreads();
    if (st.kind == LIPASR_DEFENCE_FIR) {
      def_fir_stage<true>(a, b, kDefVjpLen / 4, lo, hi, base, nv, st.taps, st.arg, hs);
    } else {
      for (int idx = lo + (int)threadIdx.x; idx < hi; idx += kDefThreads) b[idx] = def_stage_adj_at(st, a + idx, route[i] + idx, base + idx, nv);
    }
    float* t = a;
    a = b;
    b = t;
  }
  __syncthreads();
  for (int t = t0 + threadIdx.x; t < tend; t += kDefThreads) orow[t] = a[t - base];
}

// ------------------------------------------------------------------------------------------------------------ checks
// The chain from its three host arrays; the taps themselves are not read.  g: the cotangent of the vjp (else null).
static int defence_check(const char* fn, const float* x, const float* g, bool vjp, const int* kinds, const int* args,
                         const float* const* taps, int stages, int clips, int n, const float* dst, DefChain* ch) {
  LP_CHECK_ARG(stages >= 1 && stages <= kDefMaxStages, "%s: %d stages; 1 to %d are supported", fn, stages, kDefMaxStages);
  LP_CHECK_ARG(kinds != nullptr && args != nullptr, "%s: a null pointer (kinds or args)", fn);
  LP_CHECK_ARG(clips >= 0 && n >= 0, "%s: bad shape %d x %d", fn, clips, n);
  LP_CHECK_ARG(n <= kDefMaxN, "%s: rows of %d elements; at most 2^30", fn, n);
  ch->stages = stages;
  ch->halo = ch->routed = 0;
  for (int i = 0; i < kDefMaxStages; ++i) ch->s[i] = DefStage{LIPASR_DEFENCE_QUANTIZE, 16, 0, nullptr};
  for (int i = 0; i < stages; ++i) {
    const int a = args[i];
    DefStage& s = ch->s[i];
    s.kind = kinds[i];
    s.arg = a;
    s.taps = nullptr;
    switch (kinds[i]) {
      case LIPASR_DEFENCE_MEDIAN:
        LP_CHECK_ARG(a >= 3 && a <= 15 && (a & 1), "%s: stage %d: a median of width %d; odd widths 3 to 15 are supported", fn, i, a);
        s.half = (a - 1) / 2;
        break;
      case LIPASR_DEFENCE_FIR:
        LP_CHECK_ARG(a >= 1 && a <= 255 && (a & 1), "%s: stage %d: %d taps; odd counts 1 to 255 are supported", fn, i, a);
        LP_CHECK_ARG(taps != nullptr && taps[i] != nullptr, "%s: stage %d: a null pointer (taps)", fn, i);
        s.half = (a - 1) / 2;
        s.taps = taps[i];
        break;
      case LIPASR_DEFENCE_QUANTIZE:
        LP_CHECK_ARG(a >= 2 && a <= 16, "%s: stage %d: %d bits; 2 to 16 are supported", fn, i, a);
        s.half = 0;
        break;
      default:
        LP_CHECK_ARG(false, "%s: stage %d: unknown kind %d", fn, i, kinds[i]);
    }
    ch->halo += s.half;
    if (s.kind != LIPASR_DEFENCE_FIR) ch->routed = i + 1;
  }
  LP_CHECK_ARG(ch->halo <= kDefMaxHalo, "%s: the half-widths of the chain sum to %d; the halo is at most %d", fn, ch->halo, kDefMaxHalo);
  if (clips == 0 || n == 0) return LIPASR_OK;
  LP_CHECK_ARG(x != nullptr && dst != nullptr && (!vjp || g != nullptr), "%s: a null pointer", fn);
  const size_t rb = (size_t)clips * n * 4;
  LP_CHECK_ARG(!spans_overlap(dst, rb, x, rb) && !(vjp && spans_overlap(dst, rb, g, rb)), "%s: the output overlaps an input", fn);
  for (int i = 0; i < stages; ++i)
    LP_CHECK_ARG(!spans_overlap(dst, rb, ch->s[i].taps, ch->s[i].taps ? (size_t)ch->s[i].arg * 4 : 0), "%s: the output overlaps the taps of stage %d",
                 fn, i);
  const long long wgs = (((long long)n + kDefTile - 1) / kDefTile) * clips;
  LP_CHECK_ARG(wgs <= 0x7fffffffLL, "%s: %lld workgroups; split the batch", fn, wgs);
  return LIPASR_OK;
}

// a row with kDefPad zeros on either side, so that every window of a stage lies inside it
constexpr int kDefPad = 128;
static_assert(kDefPad >= 127, "the widest half-width is 127");

static void defence_row_in(const float* row, int nv, int n, std::vector<float>& buf) {
  buf.assign((size_t)n + 2 * kDefPad, 0.0f);
  for (int p = 0; p < nv; ++p) buf[kDefPad + p] = row[p];
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

int lipasr_defence_apply(const float* x, const int* n_valid, const int* kinds, const int* args, const float* const* taps, int stages,
                         int clips, int n, float* out, lipasr_stream_t stream) {
  const char* fn = "lipasr_defence_apply";
  DefChain ch;
  if (int rc = defence_check(fn, x, nullptr, false, kinds, args, taps, stages, clips, n, out, &ch)) return rc;
  if (clips == 0 || n == 0) return LIPASR_OK;
  const int tiles = (n + kDefTile - 1) / kDefTile;
  hipLaunchKernelGGL(defence_apply_kernel, dim3((unsigned)tiles * (unsigned)clips), dim3(kDefThreads), 0, S(stream), x, n_valid, ch, n,
                     tiles, out);
  ++g_defence_launches[0];
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_defence_vjp(const float* x, const float* g, const int* n_valid, const int* kinds, const int* args, const float* const* taps,
                       int stages, int clips, int n, float* gx, lipasr_stream_t stream) {
  const char* fn = "lipasr_defence_vjp";
  DefChain ch;
  if (int rc = defence_check(fn, x, g, true, kinds, args, taps, stages, clips, n, gx, &ch)) return rc;
  if (clips == 0 || n == 0) return LIPASR_OK;
  const int tiles = (n + kDefTile - 1) / kDefTile;
  hipLaunchKernelGGL(defence_vjp_kernel, dim3((unsigned)tiles * (unsigned)clips), dim3(kDefThreads), 0, S(stream), x, g, n_valid, ch, n,
                     tiles, gx);
  ++g_defence_launches[1];
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_defence_apply_host(const float* x, const int* n_valid, const int* kinds, const int* args, const float* const* taps,
                              int stages, int clips, int n, float* out) {
  const char* fn = "lipasr_defence_apply_host";
  DefChain ch;
  if (int rc = defence_check(fn, x, nullptr, false, kinds, args, taps, stages, clips, n, out, &ch)) return rc;
  std::vector<float> cur, nxt;
  for (int b = 0; b < clips; ++b) {
    const int nv = row_valid(n_valid, b, n);
    defence_row_in(x + (size_t)b * n, nv, n, cur);
    for (int i = 0; i < ch.stages; ++i) {
      nxt.assign(cur.size(), 0.0f);
      signed char r;
      for (int p = 0; p < nv; ++p) nxt[kDefPad + p] = def_stage_at(ch.s[i], cur.data() + kDefPad + p, p, nv, r);
      cur.swap(nxt);
    }
    for (int p = 0; p < n; ++p) out[(size_t)b * n + p] = cur[kDefPad + p];
  }
  return LIPASR_OK;
}

int lipasr_defence_vjp_host(const float* x, const float* g, const int* n_valid, const int* kinds, const int* args,
                            const float* const* taps, int stages, int clips, int n, float* gx) {
  const char* fn = "lipasr_defence_vjp_host";
  DefChain ch;
  if (int rc = defence_check(fn, x, g, true, kinds, args, taps, stages, clips, n, gx, &ch)) return rc;
  std::vector<float> cur, nxt;
  std::vector<signed char> route[kDefMaxStages];
  for (int b = 0; b < clips; ++b) {
    const int nv = row_valid(n_valid, b, n);
    defence_row_in(x + (size_t)b * n, nv, n, cur);
    for (int i = 0; i < ch.stages; ++i) {
      nxt.assign(cur.size(), 0.0f);
      route[i].assign(cur.size(), ch.s[i].kind == LIPASR_DEFENCE_MEDIAN ? kDefDropped : 0);
      for (int p = 0; p < nv; ++p) nxt[kDefPad + p] = def_stage_at(ch.s[i], cur.data() + kDefPad + p, p, nv, route[i][kDefPad + p]);
      cur.swap(nxt);
    }
    defence_row_in(g + (size_t)b * n, nv, n, cur);
    for (int i = ch.stages - 1; i >= 0; --i) {
      nxt.assign(cur.size(), 0.0f);
      for (int s = 0; s < nv; ++s)
        nxt[kDefPad + s] = def_stage_adj_at(ch.s[i], cur.data() + kDefPad + s, route[i].data() + kDefPad + s, s, nv);
      cur.swap(nxt);
    }
    for (int p = 0; p < n; ++p) gx[(size_t)b * n + p] = cur[kDefPad + p];
  }
  return LIPASR_OK;
}

long lipasr_debug_defence_launches(int kernel) { return (kernel == 0 || kernel == 1) ? g_defence_launches[kernel] : -1; }

}  // extern "C"
