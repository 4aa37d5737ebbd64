// T3b (model side, training): the tail of a ConvNeXt block on dense NHWC rows -- layer scale, stochastic depth and the
// residual add (convnext_orig.py:75-86: `x = self.gamma * x`, `x = input + self.drop_path(x)`) -- as one streaming pass
// per direction instead of four element-wise ATen passes, and the layer-scale gradient without a transposed copy.
//   forward :  out[r,c] = x[r,c] + (y[r,c] * gamma[c]) * s[r / HW]
//   backward:  t = g[r,c] * s[r / HW];  gy[r,c] = t * gamma[c];  ggamma[c] = sum_r t * y[r,c];  (gx = g: no kernel)
// s (B): 0 or 1 / keep per image, NULL = no factor; gamma (C) or NULL = no factor.  A dropped image is not special-cased:
// s = 0 multiplies like the torch composition does (a non-finite y gives NaN there too).
//
// Arithmetic order (this unit is compiled with -ffp-contract=off: every product and sum below is one rounded fp32
// operation, as written, whatever the build): forward two products then the add, in the order of the formula; backward
// the product with s first, then the one with gamma.  ggamma, fixed by (rows, C) alone, no atomics:
//   1. a thread owns one float4 of channels and a row slot; it adds its rows in increasing row index
//      (r = block * RPB + slot, stepping by grid * RPB) by one explicit fma per row: acc = fma(t, y, acc);
//   2. the block's RPB row slots are combined through LDS in slot order 0, 1, ..., RPB - 1 -> one partial row per block;
//   3. colsum_kernel adds the blocks in index order, associated as a balanced binary tree (colsum.h).
//
// Layout: a block has RPB = 256 / NV row slots of NV = C / 4 lanes (NV * RPB <= 256 threads, all of them active); the
// RPB rows of a block are one contiguous run of 16-byte accesses.  rows < 2^31 (the image index is a FastDiv of the row).
#include "colsum.h"
#include "sea_common.h"

namespace sea {

__device__ __forceinline__ float4 mul4(const float4 a, const float4 b) {
  return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}
__device__ __forceinline__ float4 mul4(const float4 a, const float b) { return make_float4(a.x * b, a.y * b, a.z * b, a.w * b); }

__global__ __launch_bounds__(256) void block_tail_fwd_kernel(const float4* __restrict__ x, const float4* __restrict__ y,
                                                             const float4* __restrict__ gamma, const float* __restrict__ s,
                                                             float4* __restrict__ out, int rows, int NV, FastDiv hw) {
  const int rpb = blockDim.x / NV, slot = threadIdx.x / NV, lane = threadIdx.x % NV;
  float4 gm = make_float4(0.f, 0.f, 0.f, 0.f);
  if (gamma) gm = gamma[lane];
  for (int64_t r = (int64_t)blockIdx.x * rpb + slot; r < rows; r += (int64_t)gridDim.x * rpb) {
    const int64_t i = r * NV + lane;
    float4 t = y[i];
    const float4 xv = x[i];
    if (gamma) t = mul4(t, gm);
    if (s) t = mul4(t, s[fdiv((uint32_t)r, hw)]);
    out[i] = make_float4(xv.x + t.x, xv.y + t.y, xv.z + t.z, xv.w + t.w);
  }
}

// GAMMA_GRAD: also leave this block's partial sums of ggamma in ws (gridDim.x, NV) float4; gy may be NULL then
template <bool GAMMA_GRAD>
__global__ __launch_bounds__(256) void block_tail_bwd_kernel(const float4* __restrict__ g, const float4* __restrict__ y,
                                                             const float4* __restrict__ gamma, const float* __restrict__ s,
                                                             float4* __restrict__ gy, float4* __restrict__ ws, int rows,
                                                             int NV, FastDiv hw) {
  const int rpb = blockDim.x / NV, slot = threadIdx.x / NV, lane = threadIdx.x % NV;
  float4 gm = make_float4(0.f, 0.f, 0.f, 0.f), acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (gamma) gm = gamma[lane];
  for (int64_t r = (int64_t)blockIdx.x * rpb + slot; r < rows; r += (int64_t)gridDim.x * rpb) {
    const int64_t i = r * NV + lane;
    float4 t = g[i];
    if (s) t = mul4(t, s[fdiv((uint32_t)r, hw)]);
    if constexpr (GAMMA_GRAD) {
      const float4 yv = y[i];
      acc = make_float4(fmaf(t.x, yv.x, acc.x), fmaf(t.y, yv.y, acc.y), fmaf(t.z, yv.z, acc.z), fmaf(t.w, yv.w, acc.w));
    }
    if (gy) gy[i] = gamma ? mul4(t, gm) : t;
  }
  if constexpr (GAMMA_GRAD) {
    __shared__ float4 part[256];
    part[threadIdx.x] = acc;
    __syncthreads();
    if (slot == 0) {
      float4 a = acc;
      for (int sl = 1; sl < rpb; ++sl) {
        const float4 p = part[sl * NV + lane];
        a = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
      }
      ws[(int64_t)blockIdx.x * NV + lane] = a;
    }
  }
}

// the reduction grid (GAMMA_GRAD) is capped by colsum.h; the pure streams take the library's memory-bound grid
static inline int tail_threads(int C) { return (C / 4) * (256 / (C / 4)); }
static inline int64_t tail_groups(int64_t rows, int C) {
  const int rpb = 256 / (C / 4);
  return (rows + rpb - 1) / rpb;
}
static inline bool tail_shape_ok(int64_t rows, int HW, int C) {
  return rows > 0 && rows < (1ll << 31) && HW > 0 && (rows % HW) == 0 && C >= 4 && (C % 4) == 0 && C <= 1024;
}

}  // namespace sea

using namespace sea;

// out = x + (y * gamma) * s on (rows, C) dense fp32 rows, rows = B * HW; gamma (C) / s (B) may be NULL.  C % 4 == 0, C <= 1024.
extern "C" int sea_block_tail_fwd(const float* x, const float* y, const float* gamma, const float* s, float* out, int64_t rows,
                                  int HW, int C, void* stream) {
  SEA_CHECK_ARG(x && y && out && tail_shape_ok(rows, HW, C));
  SEA_CHECK_ARG(((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)gamma) | ((uintptr_t)out)) & 15) == 0);
  hipLaunchKernelGGL(block_tail_fwd_kernel, dim3(grid_for(tail_groups(rows, C), 1)), dim3(tail_threads(C)), 0,
                     (hipStream_t)stream, (const float4*)x, (const float4*)y, (const float4*)gamma, s, (float4*)out, (int)rows,
                     C / 4, fast_div((uint32_t)HW));
  SEA_RETURN_LAST();
}

// floats of workspace for sea_block_tail_bwd with ggamma: one partial row (C) per block of its grid
extern "C" int64_t sea_block_tail_bwd_workspace(int64_t rows, int C) {
  if (!tail_shape_ok(rows, 1, C)) return 0;
  return (int64_t)colsum_blocks(tail_groups(rows, C)) * C;
}

// gy = (g * s) * gamma and, when ggamma != NULL, ggamma (C) = sum_r (g * s) * y (y, ws required then; gy may be NULL)
extern "C" int sea_block_tail_bwd(const float* g, const float* y, const float* gamma, const float* s, float* gy, float* ggamma,
                                  float* ws, int64_t rows, int HW, int C, void* stream) {
  SEA_CHECK_ARG(g && (gy || ggamma) && tail_shape_ok(rows, HW, C) && (!ggamma || (y && ws)));
  SEA_CHECK_ARG(((((uintptr_t)g) | ((uintptr_t)y) | ((uintptr_t)gamma) | ((uintptr_t)gy) | ((uintptr_t)ws)) & 15) == 0);
  const hipStream_t st = (hipStream_t)stream;
  const FastDiv hw = fast_div((uint32_t)HW);
  if (ggamma) {
    const int blocks = colsum_blocks(tail_groups(rows, C));
    hipLaunchKernelGGL(block_tail_bwd_kernel<true>, dim3(blocks), dim3(tail_threads(C)), 0, st, (const float4*)g,
                       (const float4*)y, (const float4*)gamma, s, (float4*)gy, (float4*)ws, (int)rows, C / 4, hw);
    launch_colsum(ws, blocks, C, ggamma, (float*)nullptr, C, st);
  } else {
    hipLaunchKernelGGL(block_tail_bwd_kernel<false>, dim3(grid_for(tail_groups(rows, C), 1)), dim3(tail_threads(C)), 0, st,
                       (const float4*)g, (const float4*)y, (const float4*)gamma, s, (float4*)gy, (float4*)nullptr, (int)rows,
                       C / 4, hw);
  }
  SEA_RETURN_LAST();
}
