// K2: the host side of the dense classifier's GEMMs (gfx950): the knobs, the launch counters, the table of kernel instances, the
// choice of one for a problem (pick_gemm) and the launchers.  The interface is gemm.h.  This unit holds no device code: every tile
// family is a translation unit of its own that registers its kernels and their launch shapes in the GemmTable --
//   gemm_frag.hip        32x32 fragment tile (split-K, operands global/L2 -> VGPR), plain, exchange and grouped instances
//   gemm_lds.hip         64x64 LDS tile (gemm_lds_tile.h), plain, exchange and grouped instances
//   gemm_ring.hip        64x64 LDS-DMA ring tile (gemm_ring_tile.h), arithmetic mode 2
//   gemm_ring_group.hip  128x128 weight-gradient ring tiles and the grouped launch of arithmetic mode 2
//   gemm_ring2.hip       128x64 exchange ring tile of arithmetic mode 2
// with the device code they share in gemm_device.h.  The plan-level sequences that call these launchers are mlp_train.hip (the
// training step, with the BatchNorm / dropout kernels) and mlp_infer.hip (predict / attacks / class gradients, with the softmax kernels).
#include "gemm.h"
#include <algorithm>
#include <cstdint>

namespace lipasr {

// ---------------------------------------------------------------------------------------------
// Host side.  pick_gemm is the ONE place that decides which instance runs a problem; launch_gemm, gemm_row_tiles and
// exchange_fits all go through it or through the predicates it is written with.
// ---------------------------------------------------------------------------------------------
static GemmKnobs g_knobs;
const GemmKnobs& gemm_knobs() { return g_knobs; }
constexpr int kEpiCount = EPI_DH_BNX + 1;
// Test hooks (lipasr_debug_gemm_launches / lipasr_debug_group_launches): launches since load, counted from the GemmPick / group that
// is actually launched.  Plain host increments; the kernels see nothing of them.
static long g_gemm_launches[GK_KINDS][2][2][2][3][kEpiCount] = {};  // [kind][exchange][AMODE][BMODE][arithmetic][epilogue]
static long g_group_launches[3][3] = {};   // [0 fragment, 1 LDS, 2 ring tiles][arithmetic]: grouped weight-gradient launches
static long g_group_ring_problems[4] = {};  // problems inside ring launches by GemmArgs::ring (0: not ring-legal, on plain tiles)
static long g_group_ring_launches[4] = {};  // ring launches by the launch's ring tile (1 64 x 64, 2 128 x 128 split pass, 3 per fragment)

// arithmetic mode (GemmArgs::bf16: 0 exact fp32, 1 bf16 operands, 2 fp16 two-plane split) -> index
static int arith_index(int bf16) { return bf16 == 2 ? 2 : bf16 == 1 ? 1 : 0; }
// Every instantiated GEMM kernel with its launch shape (GemmTable: gemm.h), filled on first use.  A kernel's address is taken in the
// translation unit that instantiates it, so each tile family fills its own slice of the table (register_gemm_*).
static const GemmTable& gemm_table() { static const GemmTable t; return t; }

// the instance of a kind with its tile and launch shape
static GemmPick gemm_instance(int kind, bool exchange, int amode, int bmode, int ar) {
  const GemmTable& t = gemm_table();
  const GemmShape& s = t.shape[kind];
  return GemmPick{kind, s.tile_m, s.tile_n, s.threads, s.lds_bytes, t.fn[kind][exchange ? 1 : 0][amode][bmode][ar]};
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static bool ring_legal(int amode, int bmode, const GemmArgs& g) {
  if (g_knobs.no_ring || g.bf16 != 2 || g.M < 64 || g.N < 64 || g.K < 32) return false;
  if ((g.K & 31) && (!g.zeros || (g.K & 3))) return false;  // a K tail needs the zero source, and whole 16-byte chunks
  if ((g.lda & 3) || (g.ldb & 3) || !aligned16(g.A) || !aligned16(g.B)) return false;
  const int m_real = g.ones_row ? g.M - 1 : g.M;
  if (amode == 1 && ((m_real & 3) || m_real < 4)) return false;
  if (bmode == 1 && ((g.N & 3) || g.N < 4)) return false;
  return true;
}

// The 128 x 64 exchange tile (gemm_ring2_tile) pays where the 64 x 64 tiling would put two workgroups on (nearly) every CU of the
// plan's share: then it halves the workgroups and moves 3/4 of the bytes per CU; with fewer tiles than that it would leave CUs idle.
// One workgroup per CU (124 KB of LDS) and every workgroup resident (the exchange): at most `cus` tiles.
static bool use_ring2(int bmode, const GemmArgs& g, int cus) {
  if (!g_knobs.ring2 || g.bf16 != 2 || g.M < 128 || g.N < 64 || !ring_legal(0, bmode, g)) return false;
  const long tiles = (long)((g.M + 127) / 128) * ((g.N + 63) / 64);
  return 4 * tiles >= 3 * (long)cus && tiles <= (long)cus && (g.M + 127) / 128 <= g.xc_rt_max;
}

constexpr int kLdsMinTiles = 224;  // measured on MI355X (scratch/time_gemm.py): the LDS kernel wins from ~one tile per CU

static bool use_lds_gemm(int M, int N, int K, int min_tiles = 0) {
  if (g_knobs.gemm_mode == 1) return false;
  const bool legal = M >= 64 && N >= 64 && K >= 32;
  if (g_knobs.gemm_mode == 2) return legal;
  const long tiles = (long)((M + 63) / 64) * ((N + 63) / 64);
  return legal && tiles >= (min_tiles > 0 ? min_tiles : kLdsMinTiles);
}

int pick_gemm(int amode, int bmode, const GemmArgs& g, GemmPick* out) {
  if (g.M <= 0 || g.N <= 0 || g.K <= 0) { set_error("gemm: empty problem %dx%dx%d", g.M, g.N, g.K); return LIPASR_EINVAL; }
  const bool lds_k = use_lds_gemm(g.M, g.N, g.K, g.lds_min_tiles);
  const bool exchange = g.epi == EPI_BIAS_RELU_BNX || g.epi == EPI_DH_BNX;
  int kind;
  if (g.epi == EPI_BIAS_SOFTMAX_CE) {  // one 32-wide column tile, 4 wavefronts: the epilogue reduces along lanes
    if (g.N > 32) { set_error("gemm: the fused softmax epilogue needs N <= 32 (got %d)", g.N); return LIPASR_EINVAL; }
    if (amode != 0 || bmode != 1) { set_error("gemm: the fused softmax epilogue is a forward (NN) epilogue"); return LIPASR_EINVAL; }
    kind = GK_FRAG4;
  } else if (exchange) {  // the exchange epilogue: forward (NN) or input-gradient (NT) GEMMs only
    if (amode != 0) { set_error("gemm: the exchange epilogue needs a row-major A operand"); return LIPASR_EINVAL; }
    const int cus = g.cus > 0 ? g.cus : device_cus();
    if (use_ring2(bmode, g, cus)) kind = GK_RING2;  // 128 x 64 tiles, one workgroup per CU of the plan's share
    else if (lds_k && ring_legal(0, bmode, g))      // at most one workgroup per CU: the instance with loader wavefronts
      kind = (g_knobs.ring_x1 && (long)((g.N + 63) / 64) * ((g.M + 63) / 64) <= (long)cus) ? GK_RING_X1 : GK_RING;
    else kind = lds_k ? GK_LDS : GK_FRAG4;
  } else if (lds_k) {
    kind = ring_legal(amode, bmode, g) ? GK_RING : GK_LDS;
  } else {
    // Few output tiles and a long K (the dW GEMMs of the narrow layers, K = batch): 16 wavefronts split K so that
    // the serial chain of chunk loads per wavefront stays short.  Not for the *_STATS epilogues (never needed there).
    const long tiles = (long)((g.N + 31) / 32) * ((g.M + 31) / 32);
    const bool deep = tiles <= 192 && g.K >= 512 && g.epi != EPI_BIAS_RELU_STATS && g.epi != EPI_DH_STATS;
    kind = deep ? GK_FRAG16 : GK_FRAG4;
  }
  *out = gemm_instance(kind, exchange, amode ? 1 : 0, bmode ? 1 : 0, kind >= GK_RING ? 2 : arith_index(g.bf16));
  if (!out->fn) { set_error("gemm: no kernel instance for this problem"); return LIPASR_EINVAL; }  // (a hole in the table: a bug)
  return LIPASR_OK;
}

int launch_gemm(int amode, int bmode, const GemmArgs& g, hipStream_t st) {
  GemmPick p;
  const int rc = pick_gemm(amode, bmode, g, &p);
  if (rc != LIPASR_OK) return rc;
  if (g.epi >= 0 && g.epi < kEpiCount) {
    const bool exchange = g.epi == EPI_BIAS_RELU_BNX || g.epi == EPI_DH_BNX;
    ++g_gemm_launches[p.kind][exchange ? 1 : 0][amode ? 1 : 0][bmode ? 1 : 0][p.kind >= GK_RING ? 2 : arith_index(g.bf16)][g.epi];
  }
  (void)ensure_dyn_lds(p.fn, p.lds_bytes);
  void* args[] = {const_cast<GemmArgs*>(&g)};
  (void)hipLaunchKernel(p.fn, dim3((g.N + p.tile_n - 1) / p.tile_n, (g.M + p.tile_m - 1) / p.tile_m), dim3(p.threads), args, p.lds_bytes, st);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int gemm_row_tiles(int amode, int bmode, const GemmArgs& g) {
  GemmPick p;
  return pick_gemm(amode, bmode, g, &p) == LIPASR_OK ? (g.M + p.tile_m - 1) / p.tile_m : 0;
}

// The exchange epilogue (EPI_*_BNX) spins until every row tile of its column block has published: every workgroup of the launch
// must be able to be resident at the same time.  Workgroups per CU = the occupancy query capped by the SGPR admission rule,
// times the CUs the plan's stream may use.  The row tiles must also fit the granule regions.  Anything else takes the launch
// chain (GEMM + apply kernel).
static int blocks_per_cu(const GemmPick& p) {
  int occ = 0;
  // the query answers 0 for a dynamic LDS size the kernel has not been allowed yet (launch_gemm raises the limit at a kernel's FIRST
  // launch -- which, for the exchange instances, only happens once this function has said they fit: in a fresh process the first
  // mode-2 training step then took the launch chain for every LDS-tiled layer, found by the launch-count test hook)
  (void)ensure_dyn_lds(p.fn, p.lds_bytes);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, p.fn, p.threads, p.lds_bytes) != hipSuccess) { (void)hipGetLastError(); return 0; }
  // MI355X_MICROARCH.md (residency): the hardware admits 256-thread blocks up to floor(800 / (ceil(sgpr / 16) 16 + 16)) per CU,
  // which the query does not know about (it can be one high).  These kernels use 102-106 SGPRs (GemmArgs is a large by-value
  // argument): 800 / 128 = 6 blocks of four wavefronts = 24 wavefronts per CU.
  const int by_sgpr = 24 / (p.threads / 64);
  return std::min(occ, by_sgpr);
}

// This is DELIBERATELY the conservative bound, kept as it was when the fuse-or-chain decision was measured: it is asked before the
// launch's GemmArgs exist, so it counts 64 x 64 (or 32 x 32) tiles by pick_gemm's own use_lds_gemm although the 128 x 64 instance
// would make half as many, and takes the smaller occupancy of the LDS and the 64 x 64 ring instance although pick_gemm may take
// the loader instances (one workgroup per CU, and only where the tiles are at most the CUs: inside this bound).  A launch this
// admits is resident whichever instance runs it; tightening it changes which layers fuse and needs measurements of its own.
bool exchange_fits(int bmode, int arith, int M, int N, int K, int lds_min_tiles, int xc_rt_max, int cus) {
  const bool lds_k = use_lds_gemm(M, N, K, lds_min_tiles);
  const int ts = lds_k ? 64 : 32;
  const long row_tiles = (M + ts - 1) / ts, tiles = row_tiles * ((N + ts - 1) / ts);
  if (row_tiles > xc_rt_max || row_tiles > 64) return false;
  // [BMODE][fragment | LDS kernel][arithmetic] and the ring instance [BMODE], filled on first use (one device per process in
  // practice; the kernels' resource use does not depend on the device)
  static int per_cu[2][2][3] = {{{-1, -1, -1}, {-1, -1, -1}}, {{-1, -1, -1}, {-1, -1, -1}}}, ring_pc[2] = {-1, -1};
  const int b = bmode ? 1 : 0, ar = arith_index(arith);
  int& pc = per_cu[b][lds_k ? 1 : 0][ar];
  if (pc < 0) pc = blocks_per_cu(gemm_instance(lds_k ? GK_LDS : GK_FRAG4, true, 0, b, ar));
  int per = pc;
  if (ar == 2 && lds_k) {  // the launch may take the LDS-DMA ring instance (68 KB of LDS): the smaller of the two answers
    if (ring_pc[b] < 0) ring_pc[b] = blocks_per_cu(gemm_instance(GK_RING, true, 0, b, 2));
    per = std::min(per, ring_pc[b]);
  }
  return per > 0 && tiles <= (long)per * cus;
}

int launch_gemm_group_tn(const GemmArgs* gs, int n, hipStream_t st) {
  int done = 0;
  while (done < n) {
    GemmGroup grp;
    memset(&grp, 0, sizeof(grp));
    // 64x64 LDS tiles when the group is large enough to fill the chip with them (measured: bench config 3, batch 1024)
    long big = 0;
    for (int k = 0; k < kMaxGroup && done + k < n; ++k)
      big += (long)((gs[done + k].N + 63) / 64) * ((gs[done + k].M + 63) / 64);
    const bool lds_tiles = g_knobs.group_lds && big >= 128 && gs[done].K >= 64;
    const int ts = lds_tiles ? 64 : 32;
    const int ar = gs[done].bf16;
    // 128 x 128 tiles (one workgroup per CU, half the operand bytes per flop, two accumulators per wavefront).  A CU takes in ~32 GB/s
    // whatever asks (LDS-DMA or register loads), so a launch is as long as its busiest CU's bytes: one 128 x 128 tile = 1 MB, two 64 x 64
    // tiles per CU = 1 MB as well but four per CU 2 MB.  The reference's model makes 105 + 4 tiles: with the split pass and the loader
    // wavefronts 38-40 us on a 128-CU share (64 x 64 ring tiles: 77) and config 2's step 0.310 against 0.316 ms on all 256 CUs, where
    // they leave 150 CUs idle -- so: whenever the tiles cover 40 % of the CUs the launch may use.
    int ring_tile = g_knobs.ring_tile;
    if (ring_tile >= 2 && lds_tiles && ar == 2) {
      long n128 = 0;
      for (int q = 0; q < kMaxGroup && done + q < n; ++q)
        if (ring_legal(1, 1, gs[done + q])) n128 += (long)((gs[done + q].N + 127) / 128) * ((gs[done + q].M + 127) / 128);
      if (10 * n128 < 4 * (long)(gs[done].cus > 0 ? gs[done].cus : device_cus())) ring_tile = 1;
    }
    int k = 0, tiles = 0;
    bool any_ring = false;
    for (; k < kMaxGroup && done + k < n; ++k) {
      const GemmArgs& g = gs[done + k];
      if (g.M <= 0 || g.N <= 0 || g.K <= 0) { set_error("grouped gemm: empty problem"); return LIPASR_EINVAL; }
      grp.g[k] = g;
      // arithmetic mode 2: the 128 x 128 two-accumulator ring tile for every problem it can take (ring_tile 1: the 64 x 64 ring tile)
      if (lds_tiles && ar == 2 && ring_legal(1, 1, g)) { grp.g[k].ring = ring_tile; any_ring = true; }
      const int tp = grp.g[k].ring >= 2 ? 128 : ts;
      grp.tile_start[k] = tiles;
      tiles += ((g.N + tp - 1) / tp) * ((g.M + tp - 1) / tp);
    }
    grp.n = k;
    grp.tile_start[k] = tiles;
    const GemmTable& t = gemm_table();
    const void* fn = lds_tiles ? t.grouped_lds[arith_index(ar)] : t.grouped_frag[arith_index(ar)];
    int threads = (lds_tiles ? t.grouped_lds_shape : t.grouped_frag_shape).threads;
    size_t lds = (lds_tiles ? t.grouped_lds_shape : t.grouped_frag_shape).lds_bytes;
    if (any_ring) {
      fn = t.grouped_ring;
      // 160 KB of dynamic LDS (the split-pass tile: the whole CU) where the device grants it, else the tile that splits per fragment
      if (ring_tile == 2 && !ensure_dyn_lds(fn, t.grouped_ring_shape[2].lds_bytes)) {  // (never seen on gfx950)
        ring_tile = 3;
        for (int q = 0; q < k; ++q) if (grp.g[q].ring == 2) grp.g[q].ring = 3;
      }
      lds = t.grouped_ring_shape[ring_tile].lds_bytes;
      threads = t.grouped_ring_shape[ring_tile].threads;  // (loader wavefronts: the split-pass tile only)
      ++g_group_launches[2][2];
      ++g_group_ring_launches[ring_tile];
      for (int q = 0; q < k; ++q) ++g_group_ring_problems[grp.g[q].ring & 3];
    } else {
      ++g_group_launches[lds_tiles ? 1 : 0][arith_index(ar)];
    }
    (void)ensure_dyn_lds(fn, lds);
    void* args[] = {&grp};
    (void)hipLaunchKernel(fn, dim3(tiles), dim3(threads), args, lds, st);
    LP_LAUNCH_CHECK();
    done += k;
  }
  return LIPASR_OK;
}

GemmArgs gemm_args(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K, int epi) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.B = B; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.epi = epi;
  g.xcd_map = g_knobs.xcd_map;
  g.sa = g.sb = 1.0f;
  return g;
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

long lipasr_debug_gemm_launches(int kind, int exchange, int amode, int bmode, int arith, int epi) {
  if (kind < 0 || kind >= GK_KINDS || (exchange | amode | bmode) & ~1 || arith < 0 || arith > 2 || epi < -1 || epi >= kEpiCount) return -1;
  if (!gemm_table().fn[kind][exchange][amode][bmode][arith]) return -1;
  const long* c = g_gemm_launches[kind][exchange][amode][bmode][arith];
  if (epi >= 0) return c[epi];
  long n = 0;
  for (int e = 0; e < kEpiCount; ++e) n += c[e];
  return n;
}

long lipasr_debug_group_launches(int family, int arith, int variant) {
  if (family < 0 || family > 2 || arith < 0 || arith > 2) return -1;
  if (family < 2) return variant == -1 ? g_group_launches[family][arith] : -1;
  if (arith != 2 || variant < -1 || variant > 3) return -1;  // the ring kernel is a mode-2 kernel
  return variant == -1 ? g_group_launches[2][2] : g_group_ring_problems[variant];
}

long lipasr_debug_launch_count(int kind) {
  if (kind == 0) return lipasr_debug_gemm_launches(GK_RING2, 1, 0, 0, 2, -1) + lipasr_debug_gemm_launches(GK_RING2, 1, 0, 1, 2, -1);
  return kind == 1 ? g_group_ring_launches[2] : -1;
}

int lipasr_debug_gemm_mode(int mode) {  // the bits: GemmKnobs (gemm.h)
  GemmKnobs k;
  k.gemm_mode = mode & 3;
  k.split_dw0 = (mode >> 2) & 1;
  k.group_lds = !((mode >> 3) & 1);
  k.xcd_map = (mode >> 4) & 1;
  k.no_ring = (mode >> 5) & 1;
  k.ring_tile = ((mode >> 6) & 1) ? 1 : ((mode >> 7) & 1) ? 3 : 2;
  k.ring2 = !((mode >> 8) & 1);
  k.ring_x1 = !((mode >> 9) & 1);
  g_knobs = k;
  return LIPASR_OK;
}

// the stand-alone product in arithmetic `arith`: the checks and the launch of lipasr_gemm_f32 / _f16x2 / lipasr_debug_gemm (`fn` names
// the entry in the error text)
static int gemm_entry(const char* fn, lipasr_handle_t h, int arith, int transA, int transB, int M, int N, int K, const float* A, int lda,
                      const float* B, int ldb, float* C, int ldc, float scale_a, float scale_b, lipasr_stream_t stream) {
  LP_CHECK_ARG(h && A && B && C, "%s: null argument", fn);
  LP_CHECK_ARG(arith >= 0 && arith <= 2, "%s: arithmetic mode %d (0 = exact fp32, 1 = bf16 operands, 2 = fp16 two-plane split)", fn, arith);
  LP_CHECK_ARG(M > 0 && N > 0 && K > 0, "%s: empty problem %dx%dx%d", fn, M, N, K);
  LP_CHECK_ARG(lda >= (transA ? M : K) && ldb >= (transB ? K : N) && ldc >= N, "%s: leading dimension too small", fn);
  GemmArgs g = gemm_args(A, lda, B, ldb, C, ldc, M, N, K, EPI_STORE);
  g.bf16 = arith;
  if (arith == 2) {
    int ea = 0, eb = 0;
    LP_CHECK_ARG(scale_a > 0.0f && scale_b > 0.0f && frexpf(scale_a, &ea) == 0.5f && frexpf(scale_b, &eb) == 0.5f,
                 "%s: the scales must be powers of two (got %g, %g)", fn, (double)scale_a, (double)scale_b);
    g.sa = scale_a;
    g.sb = scale_b;
    g.zeros = h->zeros;
  }
  return launch_gemm(transA ? 1 : 0, transB ? 0 : 1, g, S(stream));
}

int lipasr_gemm_f32(lipasr_handle_t h, int transA, int transB, int M, int N, int K, const float* A, int lda,
                    const float* B, int ldb, float* C, int ldc, lipasr_stream_t stream) {
  return gemm_entry("lipasr_gemm_f32", h, 0, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, 1.0f, 1.0f, stream);
}

int lipasr_debug_gemm(lipasr_handle_t h, int arith, int transA, int transB, int M, int N, int K, const float* A, int lda, const float* B,
                      int ldb, float* C, int ldc, float scale_a, float scale_b, lipasr_stream_t stream) {
  return gemm_entry("lipasr_debug_gemm", h, arith, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, scale_a, scale_b, stream);
}

int lipasr_gemm_f16x2(lipasr_handle_t h, int transA, int transB, int M, int N, int K, const float* A, int lda, const float* B,
                      int ldb, float* C, int ldc, float scale_a, float scale_b, lipasr_stream_t stream) {
  return gemm_entry("lipasr_gemm_f16x2", h, 2, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, scale_a, scale_b, stream);
}

}  // extern "C"
