// What the two attention translation units share: csrc/attention.hip (M7, fp32 MFMA) and csrc/attention_bf16.hip (M7b, the
// same three kernels on the 16-bit matrix cores).  Launch geometry of every kernel: grid (ceil(T / 128), H, B), block 256,
// wave w owns rows [128 bx + 32 w, +32) and the block walks the other index in tiles of 64 rows.
#pragma once
#include "sea_common.h"

namespace sea {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kD = 64;     // head dimension (ViT-S/16: 384 / 6; mask transformer: 384 / 6)
constexpr int kTile = 64;  // keys (or queries) per LDS tile
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// row of a 32x32 accumulator tile that register `reg` of lane-half `half` holds
__device__ __forceinline__ int acc_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// v_exp_f32 itself (2^x, flushes results below 2^-126 to zero: irrelevant next to a soft-max sum >= 1)
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}

// 64 rows x 64 floats of a (row-strided) matrix -> registers; thread e = tid + 256 i holds row e >> 4, floats 4 (e & 15)..+3.
// Rows >= n_rows are clamped to the last valid row (their results are masked or never stored).
__device__ __forceinline__ void load_tile_regs(const float* __restrict__ base, int64_t row_stride, int row0, int n_rows,
                                               f32x4 (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = (int)threadIdx.x + 256 * i;  // float4 index in the tile
    int row = row0 + (e >> 4);
    row = row < n_rows ? row : n_rows - 1;
    r[i] = *reinterpret_cast<const f32x4*>(base + (int64_t)row * row_stride + 4 * (e & 15));
  }
}

// store a transposed accumulator pair (d-tile 0 and 1) of 32 rows: out[row][d] = t[d][row] * mul, 16-byte stores
__device__ __forceinline__ void store_rows_t(float* __restrict__ base, int64_t row_stride, int row, bool ok, int lane,
                                             const f32x16& t0, const f32x16& t1, float mul) {
  if (!ok) return;
  const int half = lane >> 5;
  float* p = base + (int64_t)row * row_stride;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    f32x4 a, b;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      a[k] = t0[4 * g + k] * mul;
      b[k] = t1[4 * g + k] * mul;
    }
    *reinterpret_cast<f32x4*>(p + 8 * g + 4 * half) = a;
    *reinterpret_cast<f32x4*>(p + 32 + 8 * g + 4 * half) = b;
  }
}

struct AttnPtrs {
  const float* q;  // element (b, h, t, d) at q + b*sb + h*sh + t*st + d   (same strides for k and v)
  const float* k;
  const float* v;
  int64_t sb, sh, st;
};

}  // namespace sea

// The split path (defined in csrc/attention_bf16.hip), called by the sea_attention_* entries of csrc/attention.hip.
// arith: 22 = fp16 x 2 (amax_ws = 4 B H device words of scratch, filled here), 3 / 2 = bf16 terms (amax_ws unused).
int sea_attention_fwd_split(const sea::AttnPtrs& p, int B, int H, int T, float scale, float* out, float* lse, int arith,
                            uint32_t* amax_ws, hipStream_t stream);
int sea_attention_bwd_split(const sea::AttnPtrs& p, int B, int H, int T, float scale, const float* grad_out, const float* lse,
                            const float* delta, float* dq, float* dk, float* dv, int64_t gsb, int64_t gsh, int64_t gst, int arith,
                            uint32_t* amax_ws, hipStream_t stream);
