// K2, the 64x64 LDS tile's kernels (gemm_lds_tile.h): one problem per launch and the grouped weight-gradient launch, with their
// registration in the GemmTable.
#include "gemm_lds_tile.h"

namespace lipasr {

template <int AMODE, int BMODE, int BF = 0, int BK = kLdsBKMax, bool X = false>
__global__ __launch_bounds__(512) void gemm_lds_kernel(GemmArgs g) {
  int bx = blockIdx.x, by = blockIdx.y;
  if (g.xcd_map) xcd_tile(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x, gridDim.y, bx, by);
  gemm_lds_tile<AMODE, BMODE, BF, BK, X>(g, bx, by, gridDim.y);
}

// The grouped launch with 64x64 LDS tiles: the weight-gradient GEMMs read both operands k-major (lin[k][i], dz[k][j]), which
// is exactly the LDS image, so a tile is staged by plain float4 copies and every operand element leaves L2 once per 64x64
// tile -- half the L2 -> CU traffic of the 32x32 fragment kernel (410 MB per step at batch 1024), which is what bounded it.
template <int AMODE, int BMODE, int BF = 0>
__global__ __launch_bounds__(512) void gemm_lds_grouped_kernel(GemmGroup grp) {
  int p = 0;
  while (p + 1 < grp.n && (int)blockIdx.x >= grp.tile_start[p + 1]) ++p;
  const GemmArgs& g = grp.g[p];
  const int local = blockIdx.x - grp.tile_start[p];
  const int ntx = (g.N + 63) / 64, nty = (g.M + 63) / 64;
  int bx = local % ntx, by = local / ntx;
  if (g.xcd_map && (grp.tile_start[p] & 7) == 0) xcd_tile(local, ntx, nty, bx, by);
  gemm_lds_tile<AMODE, BMODE, BF, kLdsBKMax>(g, bx, by, nty);
}

template <int A, int B, int AR> static void reg_lds(GemmTable& t) {
  t.fn[GK_LDS][0][A][B][AR] = reinterpret_cast<const void*>(gemm_lds_kernel<A, B, AR>);
  if constexpr (A == 0) t.fn[GK_LDS][1][0][B][AR] = reinterpret_cast<const void*>(gemm_lds_kernel<0, B, AR, kLdsBKMax, true>);  // the exchange epilogue: AMODE 0 only
  if constexpr (A == 1 && B == 1) t.grouped_lds[AR] = reinterpret_cast<const void*>(gemm_lds_grouped_kernel<1, 1, AR>);
}
template <int AR> static void reg_lds_modes(GemmTable& t) {
  reg_lds<0, 0, AR>(t); reg_lds<0, 1, AR>(t); reg_lds<1, 0, AR>(t); reg_lds<1, 1, AR>(t);
}

void register_gemm_lds(GemmTable& t) {
  t.shape[GK_LDS] = {64, 64, 512, lds_gemm_bytes(kLdsBKMax)};
  t.grouped_lds_shape = t.shape[GK_LDS];
  reg_lds_modes<0>(t); reg_lds_modes<1>(t); reg_lds_modes<2>(t);
}

}  // namespace lipasr
