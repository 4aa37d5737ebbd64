// DeepLabV3's ASPP (reference semseg/models/ddcat_psp.py:33-81): the three dilated 3x3 convolutions of the frozen eval
// forward / input gradient as "product first, shift second".
//
// A 3x3 convolution with dilation = padding = rate and frozen weights W[co][ci][ky][kx] is
//     Y[q][co] = sum_t sum_ci X[q + off_t][ci] W_t[co][ci],   off_t = ((ky - 1) rate, (kx - 1) rate),  t = 3 ky + kx,
// and the inner sum does not depend on where the row of X is read FOR: with Z_t = X . W_t^T computed once on the
// un-shifted map (one M8 product for every tap of every rate, N = R * 9 * Cb columns),
//     Y[q] = sum_t Z_t[q + off_t].
// No copy of the 2048-channel input is shifted, padded or split into phases; the shift happens on Cb = 256-channel rows.
//
// P5  sea_aspp_tap_sum: Y[b][y][x][r Cb + c] = max(acc + shift[r Cb + c], 0), acc = 0.f, then for t = 0 .. 8 in that order
//     acc += Z[b][y + (ky-1) rate_r][x + (kx-1) rate_r][z_col0 + (9 r + t) Cb + c]; a tap whose source pixel lies outside
//     the map is skipped (the convolution's zero padding).  The BatchNorm scale is folded into W, its shift is ``shift``.
//     Compiled with -ffp-contract=off: the bits are those of the written-out sum.  One float4 of channels per lane, lanes
//     along (pixel, branch, channel): every load is a run of Cb * 4 contiguous bytes, and every element of Z whose target
//     pixel exists is read exactly once.  Y is a channel slice (pixel stride ldy, first column y_col0) of the ASPP
//     concatenation; nothing outside the slice is written.
//     sea_aspp_tap_sum_backward: the adjoint as a gather, dZ[b][y'][x'][(9 r + t) Cb + c] = Y[q] > 0 ? dY[q] : 0 with
//     q = (y' - (ky-1) rate_r, x' - (kx-1) rate_r), and 0 where q lies outside the map.  Every element of dZ's branch
//     columns is written exactly once, zeros included (the product dX = dZ . W_all reads them all).  One term per
//     element: no atomics, no rounding.  The gate is the saved output Y, as in P3.
//     All element offsets are 64-bit: Z holds B H W * 27 * 256 floats (826 MB at B = 8, 473 x 473 inputs).
#include "sea_common.h"

namespace sea {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kAsppMaxBranches = 4;

struct AsppRates {
  int rate[kAsppMaxBranches];
};

// (a select chain, not an indexed read: the kernel-argument struct stays in scalar registers)
__device__ __forceinline__ int aspp_rate(const AsppRates& rt, int r) {
  return r == 0 ? rt.rate[0] : r == 1 ? rt.rate[1] : r == 2 ? rt.rate[2] : rt.rate[3];
}

// total = B * H * W * R * C4 lanes; i -> (pixel, r, c4)
__global__ __launch_bounds__(256) void aspp_tap_sum_kernel(const float* __restrict__ z, const float* __restrict__ shift,
                                                           float* __restrict__ y, int64_t total, int H, int W, int R,
                                                           int C4, int64_t ldz, int64_t z_col0, int64_t ldy,
                                                           int64_t y_col0, AsppRates rates) {
  const int Cb = 4 * C4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    const int64_t u = i / C4;
    const int r = (int)(u % R);
    const int64_t pix = u / R;                       // (b * H + py) * W + px
    const int px = (int)(pix % W);
    const int64_t rowid = pix / W;                   // b * H + py
    const int py = (int)(rowid % H);
    const int rate = aspp_rate(rates, r);
    const float* zc = z + z_col0 + (int64_t)(9 * r) * Cb + 4 * c4;
    f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int dy = (t / 3 - 1) * rate, dx = (t % 3 - 1) * rate;
      const int sy = py + dy, sx = px + dx;
      if (sy >= 0 && sy < H && sx >= 0 && sx < W) {
        const int64_t src = pix + (int64_t)dy * W + dx;
        acc += *(const f4*)(zc + src * ldz + (int64_t)t * Cb);
      }
    }
    const int col = r * Cb + 4 * c4;
    const f4 s = *(const f4*)(shift + col);
    const f4 v = acc + s;
    f4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = v[k] > 0.f ? v[k] : 0.f;
    *(f4*)(y + pix * ldy + y_col0 + col) = o;
  }
}

// total = B * H * W * R * 9 * C4 lanes; i -> (pixel, r, t, c4): the 9 * Cb floats of one (pixel, branch) are one run
__global__ __launch_bounds__(256) void aspp_tap_sum_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                               float* __restrict__ dz, int64_t total, int H, int W,
                                                               int R, int C4, int64_t lddy, int64_t dy_col0,
                                                               int64_t ldy, int64_t y_col0, int64_t ldz,
                                                               int64_t z_col0, AsppRates rates) {
  const int Cb = 4 * C4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    const int64_t u = i / C4;
    const int t = (int)(u % 9);
    const int64_t v = u / 9;
    const int r = (int)(v % R);
    const int64_t pix = v / R;
    const int px = (int)(pix % W);
    const int64_t rowid = pix / W;
    const int py = (int)(rowid % H);
    const int rate = aspp_rate(rates, r);
    const int oy = (t / 3 - 1) * rate, ox = (t % 3 - 1) * rate;
    const int qy = py - oy, qx = px - ox;
    f4 o = {0.f, 0.f, 0.f, 0.f};
    if (qy >= 0 && qy < H && qx >= 0 && qx < W) {
      const int64_t q = pix - (int64_t)oy * W - ox;
      const int col = r * Cb + 4 * c4;
      const f4 yv = *(const f4*)(y + q * ldy + y_col0 + col);
      const f4 gv = *(const f4*)(dy + q * lddy + dy_col0 + col);
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = yv[k] > 0.f ? gv[k] : 0.f;
    }
    *(f4*)(dz + pix * ldz + z_col0 + (int64_t)(9 * r + t) * Cb + 4 * c4) = o;
  }
}

}  // namespace sea

using namespace sea;

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// a (B, H, W, .) row tensor with pixel stride ld whose columns [col0, col0 + width) hold float4-aligned data
static bool aspp_slice_ok(const void* p, int64_t ld, int64_t col0, int64_t width) {
  return p && aligned16(p) && ld > 0 && (ld % 4) == 0 && col0 >= 0 && (col0 % 4) == 0 && col0 + width <= ld;
}

static bool aspp_shape_ok(int B, int H, int W, int R, int Cb, const int* rates, AsppRates* out) {
  if (!(B > 0 && H > 0 && W > 0 && R >= 1 && R <= kAsppMaxBranches && Cb > 0 && (Cb % 4) == 0 && rates)) return false;
  if ((int64_t)B * H * W >= (1ll << 31) || (int64_t)9 * R * Cb >= (1ll << 31) || H > (1 << 24) || W > (1 << 24)) return false;
  for (int r = 0; r < kAsppMaxBranches; ++r) {
    out->rate[r] = r < R ? rates[r] : 1;
    // (H, W <= 2^24 and rate <= 2^20: py + dy stays inside 32 bits, (ky - 1) * rate * W far inside 64)
    if (out->rate[r] < 1 || out->rate[r] > (1 << 20)) return false;
  }
  return true;
}

extern "C" int sea_aspp_tap_sum(const float* z, int64_t ldz, int64_t z_col0, const float* shift, float* y, int64_t ldy,
                                int64_t y_col0, int B, int H, int W, int R, int Cb, const int* rates, void* stream) {
  AsppRates rt;
  SEA_CHECK_ARG(aspp_shape_ok(B, H, W, R, Cb, rates, &rt));
  SEA_CHECK_ARG(aspp_slice_ok(z, ldz, z_col0, (int64_t)9 * R * Cb) && aspp_slice_ok(y, ldy, y_col0, (int64_t)R * Cb));
  SEA_CHECK_ARG(shift && aligned16(shift) && (const void*)z != (const void*)y);
  const int64_t total = (int64_t)B * H * W * R * (Cb / 4);
  hipLaunchKernelGGL(aspp_tap_sum_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, z, shift, y,
                     total, H, W, R, Cb / 4, ldz, z_col0, ldy, y_col0, rt);
  SEA_RETURN_LAST();
}

extern "C" int sea_aspp_tap_sum_backward(const float* dy, int64_t lddy, int64_t dy_col0, const float* y, int64_t ldy,
                                         int64_t y_col0, float* dz, int64_t ldz, int64_t z_col0, int B, int H, int W,
                                         int R, int Cb, const int* rates, void* stream) {
  AsppRates rt;
  SEA_CHECK_ARG(aspp_shape_ok(B, H, W, R, Cb, rates, &rt));
  SEA_CHECK_ARG(aspp_slice_ok(dy, lddy, dy_col0, (int64_t)R * Cb) && aspp_slice_ok(y, ldy, y_col0, (int64_t)R * Cb) &&
                aspp_slice_ok(dz, ldz, z_col0, (int64_t)9 * R * Cb));
  SEA_CHECK_ARG((const void*)dz != (const void*)y && (const void*)dz != (const void*)dy);
  const int64_t total = (int64_t)B * H * W * R * 9 * (Cb / 4);
  hipLaunchKernelGGL(aspp_tap_sum_bwd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, dy, y, dz,
                     total, H, W, R, Cb / 4, lddy, dy_col0, ldy, y_col0, ldz, z_col0, rt);
  SEA_RETURN_LAST();
}
