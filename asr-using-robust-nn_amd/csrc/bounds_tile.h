// The MFMA tile of the bound kernels, stated once: bounds_layer_kernel and bounds_back_kernel (bounds.hip), bg_wgrad_kernel and
// bg_back_kernel (bounds_grad.hip), cg_adjoint_kernel and cg_wgrad_kernel (bounds_crown_grad.hip).
//
// A block of kBdThreads = 256 threads makes a 32 x 128 tile of out[r][c] = sum_k a[r][k] w[k][c] on v_mfma_f32_32x32x2_f32, a
// wavefront per 32 columns, the reduction in chunks of 32.  Lane (li, h) of a wavefront feeds a step with row li of a and column
// li of w at k = 2 s + h, and holds in element e of its accumulator the row (e & 3) + 8 (e >> 2) + 4 h of column wave 32 + li.
// A chunk is a narrow operand (32 x 32, 4 elements a thread) and a wide one (32 x 128, 16 elements a thread); bt_pipeline keeps the
// next chunk's loads in flight in registers while the current one feeds the 16 MFMA steps from LDS.  A kernel states what is its
// own: how an element is formed (fetch, or stage where it is formed as it is stored), how many accumulators a step feeds, and the
// epilogue.  Elements out of range read as 0.  The MFMA is an fmaf chain in ascending k: steps and chunks run in ascending order.
#pragma once
#include "bounds.h"

namespace lipasr {

constexpr int kBtNarrow = 32 * 33;   // floats of a narrow image: the 32 x 32 block, rows padded to 33 so that both reads below
                                     // (a column of 32 rows, a row of 32 columns) touch 32 different banks
constexpr int kBtWideK = 32 * 128;  // floats of a wide image, k-major: rows of 128, no padding (a step reads along a row)
constexpr int kBtWideN = 128 * 33;  // floats of a wide image, n-major: padded like the narrow one, and for the same reason

struct BtThread {
  int tid, lane, wave, li, h;
  __device__ __forceinline__ BtThread() : tid(threadIdx.x), lane(tid & 63), wave(tid >> 6), li(lane & 31), h(lane >> 5) {}
  // where element e of an accumulator lies in the tile at (r0, c0); the row is the same for the 32 lanes of a half
  __device__ __forceinline__ int row(int r0, int e) const { return r0 + (e & 3) + 8 * (e >> 2) + 4 * h; }
  __device__ __forceinline__ int col(int c0) const { return c0 + wave * 32 + li; }
};

__device__ __forceinline__ bd_f32x16 bt_zero() {
  bd_f32x16 v;
#pragma unroll
  for (int e = 0; e < 16; ++e) v[e] = 0.0f;
  return v;
}

// f(q, i, j) for the Q elements of a thread in a chunk walked [.][1 << LOG], consecutive threads along j
template <int Q, int LOG, class F>
__device__ __forceinline__ void bt_each(int tid, const F& f) {
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int idx = tid + kBdThreads * q;
    f(q, idx >> LOG, idx & ((1 << LOG) - 1));
  }
}

// the narrow operand: f(q, i, j), image a[i * 33 + j].  by_row: i is the output row and j the k of the chunk (layer, back, adjoint);
// by_k: i is the k of the chunk and j the output row (the two weight-gradient kernels, whose operand is stored [k][rows])
template <class F>
__device__ __forceinline__ void bt_narrow_each(int tid, const F& f) { bt_each<4, 5>(tid, f); }
__device__ __forceinline__ int bt_narrow_at(int i, int j) { return i * 33 + j; }
__device__ __forceinline__ void bt_narrow_store(float* a, int tid, const float (&reg)[4]) {
  bt_narrow_each(tid, [&](int q, int i, int j) { a[bt_narrow_at(i, j)] = reg[q]; });
}
// the two reads of step s.  Each map is stated once, as the macro; the function is how a kernel reads, except bg_wgrad_kernel and
// bg_back_kernel, which expand the macros in place: through a function the compiler pairs the first one's reads of steps s and
// s + 1 into ds_read2 with folded offsets and issues the second one's reads in blocks ahead of its MFMAs; in place both keep the
// order of reads and MFMAs they were tuned and measured with (profiles/bounds_tile_timing.txt)
#define BT_NARROW_BY_ROW(a, t, s) (a)[(t).li * 33 + 2 * (s) + (t).h]
#define BT_NARROW_BY_K(a, t, s) (a)[(2 * (s) + (t).h) * 33 + (t).li]
__device__ __forceinline__ float bt_narrow_by_row(const float* a, const BtThread& t, int s) { return BT_NARROW_BY_ROW(a, t, s); }
__device__ __forceinline__ float bt_narrow_by_k(const float* a, const BtThread& t, int s) { return BT_NARROW_BY_K(a, t, s); }

// the wide operand stored [k][N]: f(q, k, col), image w[k * 128 + col] (kBtWideK floats)
template <class F>
__device__ __forceinline__ void bt_wide_k_each(int tid, const F& f) { bt_each<16, 7>(tid, f); }
__device__ __forceinline__ int bt_wide_k_at(int k, int col) { return k * 128 + col; }
__device__ __forceinline__ void bt_wide_k_store(float* w, int tid, const float (&reg)[16]) {
  bt_wide_k_each(tid, [&](int q, int k, int col) { w[bt_wide_k_at(k, col)] = reg[q]; });
}
#define BT_WIDE_K(w, t, s) (w)[(2 * (s) + (t).h) * 128 + (t).wave * 32 + (t).li]
__device__ __forceinline__ float bt_wide_k(const float* w, const BtThread& t, int s) { return BT_WIDE_K(w, t, s); }

// W stored [N][K]: f(q, n, k), image w[n * 33 + k] (kBtWideN floats)
template <class F>
__device__ __forceinline__ void bt_wide_n_each(int tid, const F& f) { bt_each<16, 5>(tid, f); }
__device__ __forceinline__ void bt_wide_n_store(float* w, int tid, const float (&reg)[16]) {
  bt_wide_n_each(tid, [&](int q, int n, int k) { w[n * 33 + k] = reg[q]; });
}
#define BT_WIDE_N(w, t, s) (w)[((t).wave * 32 + (t).li) * 33 + 2 * (s) + (t).h]
__device__ __forceinline__ float bt_wide_n(const float* w, const BtThread& t, int s) { return BT_WIDE_N(w, t, s); }

// the reduction over [begin, end) in chunks of 32.  fetch(k0): the chunk at k0 into registers; stage(): the registers into LDS;
// step(s): the MFMAs of k = 2 s + h from LDS
template <class Fetch, class Stage, class Step>
__device__ __forceinline__ void bt_pipeline(int begin, int end, const Fetch& fetch, const Stage& stage, const Step& step) {
  fetch(begin);
  for (int k0 = begin; k0 < end; k0 += 32) {
    __syncthreads();  // the previous chunk is read
    stage();
    __syncthreads();
    if (k0 + 32 < end) fetch(k0 + 32);  // in flight while this chunk feeds the MFMAs
#pragma unroll
    for (int s = 0; s < 16; ++s) step(s);
  }
}

}  // namespace lipasr
