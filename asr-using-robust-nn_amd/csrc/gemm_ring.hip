// K2, the 64x64 LDS-DMA ring tile's kernels (gemm_ring_tile.h; arithmetic mode 2 only): the plain and exchange instances and the
// exchange instance with loader wavefronts, with their registration in the GemmTable.
#include "gemm_ring_tile.h"

namespace lipasr {

#ifndef LIPASR_RING_LOADERS
#define LIPASR_RING_LOADERS 0
#endif
constexpr int kRingLoaders = LIPASR_RING_LOADERS;  // 0, 1, 2 or 4 (with the exchange epilogue's 81 registers two workgroups of ten wavefronts still share a CU).
// Measured with 2 (same box, interleaved): config 3 0.3427 against 0.3422 ms, config 2 0.3117 against 0.3108 -- two workgroups per CU already
// overlap one's address-path time with the other's arithmetic; the loaders pay where ONE workgroup owns the CU (the tiles of gemm_ring_group.hip and gemm_ring2.hip).  Off.
template <int AMODE, int BMODE, bool X = false>
__global__ __launch_bounds__(512 + 64 * kRingLoaders) void gemm_ring_kernel(GemmArgs g) {
  int bx = blockIdx.x, by = blockIdx.y;
  if (g.xcd_map) xcd_tile(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x, gridDim.y, bx, by);
  gemm_ring_tile<AMODE, BMODE, X, kRingLoaders>(g, bx, by, gridDim.y);
}
// The exchange instance for launches of at most ONE workgroup per CU (layer 2 on a 128-CU share, layer 1 on the whole chip): four loader
// wavefronts.  Same box, interleaved, loaders on every exchange launch: config 2 0.3067 against 0.3098 ms (its 256-tile launches are one per
// CU); config 3 lost (two workgroups of twelve wavefronts no longer share a CU at 81 registers) -- hence per launch.
constexpr int kRingLoadersOnePerCu = 4;
template <int BMODE>
__global__ __launch_bounds__(512 + 64 * kRingLoadersOnePerCu) void gemm_ring_x1_kernel(GemmArgs g) {
  int bx = blockIdx.x, by = blockIdx.y;
  if (g.xcd_map) xcd_tile(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x, gridDim.y, bx, by);
  gemm_ring_tile<0, BMODE, true, kRingLoadersOnePerCu>(g, bx, by, gridDim.y);
}

template <int A, int B> static void reg_ring(GemmTable& t) {
  t.fn[GK_RING][0][A][B][2] = reinterpret_cast<const void*>(gemm_ring_kernel<A, B>);
  if constexpr (A == 0) {  // the exchange epilogue: AMODE 0 only
    t.fn[GK_RING][1][0][B][2] = reinterpret_cast<const void*>(gemm_ring_kernel<0, B, true>);
    t.fn[GK_RING_X1][1][0][B][2] = reinterpret_cast<const void*>(gemm_ring_x1_kernel<B>);
  }
}

void register_gemm_ring(GemmTable& t) {
  t.shape[GK_RING] = {64, 64, 512 + 64 * kRingLoaders, ring_gemm_bytes()};
  t.shape[GK_RING_X1] = {64, 64, 512 + 64 * kRingLoadersOnePerCu, ring_gemm_bytes()};
  reg_ring<0, 0>(t); reg_ring<0, 1>(t); reg_ring<1, 0>(t); reg_ring<1, 1>(t);
}

}  // namespace lipasr
