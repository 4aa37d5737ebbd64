// Second stage of the deterministic column sums of the training kernels (T3a: LayerNorm dw / db, T3b: the layer-scale
// gradient).  Stage one leaves one row of partial sums per block in a workspace `ws` (nb, ncols); here column c becomes
// the sum of ws[0][c] .. ws[nb-1][c], the blocks in index order, associated as a balanced binary tree:
//   level 1: (0 + 1), (2 + 3), ...;  level 2: (0..1 + 2..3), (4..5 + 6..7), ...;  a range without a right neighbour waits.
// Every partial sum covers a contiguous range of block indices and is always the LEFT operand of the range that follows
// it.  (A left-to-right walk over 1024 blocks rounds 1024 times at the magnitude of the total; the tree does so once per
// level, which keeps the error below that of a library reduction: DESIGN section 5, T3.)
// No atomics: the result depends on (nb, ncols) and the partial sums only, never on the order in which blocks ran.
// A block stages its kColsumCols columns of every partial row in LDS and reduces them there.
#pragma once
#include "sea_common.h"

namespace sea {

constexpr int kColsumMaxBlocks = 1024;  // cap of a stage-one grid: bounds the LDS tile (32 KB)
constexpr int kColsumCols = 8;

// number of stage-one blocks for `groups` groups of rows (one group = the rows a block takes per grid stride)
static inline int colsum_blocks(int64_t groups) {
  return (int)(groups < 1 ? 1 : (groups > kColsumMaxBlocks ? kColsumMaxBlocks : groups));
}

// columns [0, split) go to out0, columns [split, ncols) to out1[c - split]
static __global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ ws, int nb, int ncols,
                                                            float* __restrict__ out0, float* __restrict__ out1, int split) {
  __shared__ float tile[kColsumMaxBlocks * kColsumCols];
  const int c0 = blockIdx.x * kColsumCols;
  for (int i = threadIdx.x; i < nb * kColsumCols; i += 256) {
    const int b = i / kColsumCols, c = c0 + i % kColsumCols;
    tile[i] = c < ncols ? ws[(int64_t)b * ncols + c] : 0.f;
  }
  __syncthreads();
  const int j = threadIdx.x % kColsumCols, q = threadIdx.x / kColsumCols;
  for (int step = 1; step < nb; step *= 2) {
    for (int b = q * 2 * step; b + step < nb; b += (256 / kColsumCols) * 2 * step)
      tile[b * kColsumCols + j] += tile[(b + step) * kColsumCols + j];
    __syncthreads();
  }
  const int c = c0 + threadIdx.x;
  if (threadIdx.x < kColsumCols && c < ncols) {
    if (c < split) out0[c] = tile[threadIdx.x];
    else out1[c - split] = tile[threadIdx.x];
  }
}

static inline void launch_colsum(const float* ws, int nb, int ncols, float* out0, float* out1, int split, hipStream_t st) {
  hipLaunchKernelGGL(colsum_kernel, dim3((ncols + kColsumCols - 1) / kColsumCols), dim3(256), 0, st, ws, nb, ncols, out0, out1,
                     split);
}

}  // namespace sea
