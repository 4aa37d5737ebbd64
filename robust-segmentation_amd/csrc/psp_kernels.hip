// PSPNet-ResNet50 (reference semseg/models/ddcat_psp.py:372-486, backbones/resnet_ddcat.py): the data-movement and
// element-wise steps of its frozen eval forward / input gradient.  The convolutions themselves run on the existing
// Winograd (M1) and operand-split GEMM (M8) paths.
//
// P1  polyphase split / merge (channels_last fp32, C % 4 == 0, one float4 per lane).  A 3x3 convolution with
//     dilation d and padding d equals, for every phase (py, px) in [0, d)^2, an ordinary 3x3 / pad-1 convolution of the
//     sub-image s[m][n] = x[py + d m][px + d n] (the reference's dilated conv2 of layer3 / layer4).  split writes the d*d
//     sub-images of every image as one batch (B*d*d, ceil(H/d), ceil(W/d), C), zero where py + d m >= H or px + d n >= W:
//     those zero tails stand for the convolution's zero padding, so the sub-image convolutions are exact.  merge is the
//     inverse on the valid positions and crops the tails.  Each is the other's adjoint, so the backward of a split is a
//     merge and vice versa.  first_only: phase (0, 0) alone = x[::d, ::d] (the stride-2 1x1 downsample of layer2), and its
//     adjoint, which writes zeros at every other position.
//     Grid: one block row per output row, lanes over (column, float4) of that row: every load and store is a run of
//     C*4 contiguous bytes.  Pure data movement: bytes = read + write of the larger side.
//
// P2  bilinear up-sampling with align_corners=True (the PPM branches, ddcat_psp.py:28, and the final logits,
//     ddcat_psp.py:467).  ATen's arithmetic (UpSampleBilinear2d.cu): scale = (in-1)/(out-1) in fp32 (0 for in == 1),
//     src = scale*dst, i0 = (int)src, i1 = i0 + (i0 < in-1), l1 = src - i0, l0 = 1 - l1,
//     out = l0_y*(l0_x*v00 + l1_x*v01) + l1_y*(l0_x*v10 + l1_x*v11), the same expression in the same order and with the
//     same fused multiply-adds as ATen's compiled kernel (lerp_ac): bitwise F.interpolate.
//     NCHW form: one output pixel of one plane per lane.  channels_last form: one float4 of channels per lane, written
//     into a channel slice of a wider tensor (pixel stride S): the PPM's 4096-channel concatenation is never assembled
//     by a copy.
//     Backward: a gather in two separable passes (first along W into a (rows, H_out, w_in) workspace, then along H),
//     each input pixel summing, in increasing output index, the outputs its weights feed.  Deterministic, no atomics.
//
// P3  residual add + ReLU of a bottleneck (resnet_ddcat.py:102-105): y = max(a + r, 0); backward g' = y > 0 ? g : 0,
//     the gradient of both a and r.  float4 per lane, grid-stride.
#include "bilinear_map.h"
#include "sea_common.h"

namespace sea {

typedef float f4 __attribute__((ext_vector_type(4)));

// ---- P1 ------------------------------------------------------------------------------------------------------------
// rows = B * P * Hs rows of y (P = d*d, or 1 with first_only); lanes over Ws * C4
__global__ __launch_bounds__(256) void psp_split_kernel(const f4* __restrict__ x, f4* __restrict__ y, int rows, int P,
                                                        int H, int W, int Hs, int Ws, int C4, int d) {
  const int rowlen = Ws * C4;
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {
    const int m = row % Hs;
    const int bp = row / Hs;
    const int p = bp % P, b = bp / P;
    const int py = p / d, px = p % d;
    const int h = py + d * m;
    f4* yr = y + (int64_t)row * rowlen;
    const f4* xr = x + ((int64_t)b * H + h) * W * C4;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rowlen; i += gridDim.x * blockDim.x) {
      const int n = i / C4, c = i - n * C4;
      const int w = px + d * n;
      f4 v = {0.f, 0.f, 0.f, 0.f};
      if (h < H && w < W) v = xr[(int64_t)w * C4 + c];
      yr[i] = v;
    }
  }
}

// rows = B * H rows of x; lanes over W * C4
__global__ __launch_bounds__(256) void psp_merge_kernel(const f4* __restrict__ y, f4* __restrict__ x, int rows, int P,
                                                        int H, int W, int Hs, int Ws, int C4, int d) {
  const int rowlen = W * C4;
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {
    const int h = row % H, b = row / H;
    const int py = h % d, m = h / d;
    f4* xr = x + (int64_t)row * rowlen;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rowlen; i += gridDim.x * blockDim.x) {
      const int w = i / C4, c = i - w * C4;
      const int px = w % d, n = w / d;
      const int p = py * d + px;
      f4 v = {0.f, 0.f, 0.f, 0.f};
      if (p < P) v = y[(((int64_t)b * P + p) * Hs + m) * Ws * C4 + (int64_t)n * C4 + c];
      xr[i] = v;
    }
  }
}

static void p1_grid(int rows, int rowlen, dim3& grid) {
  grid.x = (rowlen + 255) / 256;
  grid.y = rows < 65535 ? rows : 65535;
  grid.z = 1;
}

// ---- P2 ------------------------------------------------------------------------------------------------------------
// psp_ac_scale, ac_map and lerp_ac: bilinear_map.h (T2u-ac interpolates with the same definitions)
// weight of input index i in output index o (0 if o does not read i)
__device__ __forceinline__ float ac_weight(int o, int i, float scale, int n_in) {
  const AcMap a = ac_map(o, scale, n_in);
  float wgt = 0.f;
  if (a.i0 == i) wgt += a.l0;
  if (a.i0 + a.p == i) wgt += a.l1;
  return wgt;
}

// output indices [lo, hi] that may read input index i (a superset: ac_weight decides)
__device__ __forceinline__ void ac_range(int i, float scale, int n_in, int n_out, int& lo, int& hi) {
  if (n_in == 1 || scale <= 0.f) {
    lo = 0;
    hi = n_out - 1;
    return;
  }
  lo = (int)floorf((float)(i - 1) / scale) - 1;
  hi = (int)ceilf((float)(i + 1) / scale) + 1;
  if (lo < 0) lo = 0;
  if (hi > n_out - 1) hi = n_out - 1;
}

// NCHW forward: planes x (h, w) -> planes x (H, W)
__global__ __launch_bounds__(256) void psp_up_ac_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                        int64_t total, int h, int w, int H, int W, float sh, float sw) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int X = (int)(i % W);
    const int64_t t = i / W;
    const int Y = (int)(t % H);
    const int64_t plane = t / H;
    const AcMap my = ac_map(Y, sh, h), mx = ac_map(X, sw, w);
    const float* r0 = x + (plane * h + my.i0) * w;
    const float* r1 = r0 + (int64_t)my.p * w;
    y[i] = lerp_ac(r0[mx.i0], r0[mx.i0 + mx.p], r1[mx.i0], r1[mx.i0 + mx.p], mx, my);
  }
}

// NCHW backward pass 1 (along W): t[plane][Y][j] = sum_X wx(X, j) g[plane][Y][X]
__global__ __launch_bounds__(256) void psp_up_ac_bwd_w_kernel(const float* __restrict__ g, float* __restrict__ t,
                                                              int64_t total, int w, int H, int W, float sw) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % w);
    const int64_t rowY = i / w;                       // plane * H + Y
    const float* gr = g + rowY * W;
    int lo, hi;
    ac_range(j, sw, w, W, lo, hi);
    float acc = 0.f;
    for (int X = lo; X <= hi; ++X) {
      const float wx = ac_weight(X, j, sw, w);
      if (wx != 0.f) acc += wx * gr[X];
    }
    t[i] = acc;
  }
}

// NCHW backward pass 2 (along H): gx[plane][i][j] = sum_Y wy(Y, i) t[plane][Y][j]
__global__ __launch_bounds__(256) void psp_up_ac_bwd_h_kernel(const float* __restrict__ t, float* __restrict__ gx,
                                                              int64_t total, int h, int w, int H, float sh) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < total; k += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(k % w);
    const int64_t q = k / w;
    const int i = (int)(q % h);
    const int64_t plane = q / h;
    const float* tp = t + plane * H * w + j;
    int lo, hi;
    ac_range(i, sh, h, H, lo, hi);
    float acc = 0.f;
    for (int Y = lo; Y <= hi; ++Y) {
      const float wy = ac_weight(Y, i, sh, h);
      if (wy != 0.f) acc += wy * tp[(int64_t)Y * w];
    }
    gx[k] = acc;
  }
}

// channels_last forward: x dense (B, h, w, C) -> y (B, H, W, C) with pixel stride S (a channel slice of a wider tensor)
__global__ __launch_bounds__(256) void psp_up_ac_cl_kernel(const f4* __restrict__ x, float* __restrict__ y,
                                                           int64_t total, int C4, int h, int w, int H, int W, int S,
                                                           float sh, float sw) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4);
    const int64_t pix = i / C4;
    const int X = (int)(pix % W);
    const int64_t t = pix / W;
    const int Y = (int)(t % H);
    const int64_t b = t / H;
    const AcMap my = ac_map(Y, sh, h), mx = ac_map(X, sw, w);
    const f4* r0 = x + ((b * h + my.i0) * w) * C4 + c;
    const f4* r1 = r0 + (int64_t)my.p * w * C4;
    const f4 v00 = r0[(int64_t)mx.i0 * C4], v01 = r0[(int64_t)(mx.i0 + mx.p) * C4];
    const f4 v10 = r1[(int64_t)mx.i0 * C4], v11 = r1[(int64_t)(mx.i0 + mx.p) * C4];
    f4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = lerp_ac(v00[k], v01[k], v10[k], v11[k], mx, my);
    *(f4*)(y + pix * S + 4 * c) = o;
  }
}

// channels_last backward pass 1 (along W): t (B, H, w, C) dense from g (B, H, W, C) with pixel stride S
__global__ __launch_bounds__(256) void psp_up_ac_cl_bwd_w_kernel(const float* __restrict__ g, f4* __restrict__ t,
                                                                 int64_t total, int C4, int w, int W, int S, float sw) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4);
    const int64_t q = i / C4;
    const int j = (int)(q % w);
    const int64_t rowY = q / w;                       // b * H + Y
    const float* gr = g + rowY * W * S + 4 * c;
    int lo, hi;
    ac_range(j, sw, w, W, lo, hi);
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int X = lo; X <= hi; ++X) {
      const float wx = ac_weight(X, j, sw, w);
      if (wx != 0.f) acc += wx * *(const f4*)(gr + (int64_t)X * S);
    }
    t[i] = acc;
  }
}

// channels_last backward pass 2 (along H): gx (B, h, w, C) dense from t (B, H, w, C)
__global__ __launch_bounds__(256) void psp_up_ac_cl_bwd_h_kernel(const f4* __restrict__ t, f4* __restrict__ gx,
                                                                 int64_t total, int C4, int h, int w, int H, float sh) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < total; k += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(k % C4);
    const int64_t q = k / C4;
    const int j = (int)(q % w);
    const int64_t q2 = q / w;
    const int i = (int)(q2 % h);
    const int64_t b = q2 / h;
    const f4* tp = t + (b * H * w + j) * C4 + c;
    int lo, hi;
    ac_range(i, sh, h, H, lo, hi);
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int Y = lo; Y <= hi; ++Y) {
      const float wy = ac_weight(Y, i, sh, h);
      if (wy != 0.f) acc += wy * tp[(int64_t)Y * w * C4];
    }
    gx[k] = acc;
  }
}

// ---- P3 ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void psp_add_relu_kernel(const f4* __restrict__ a, const f4* __restrict__ r,
                                                           f4* __restrict__ y, int64_t n4) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const f4 s = a[i] + r[i];
    f4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = s[k] > 0.f ? s[k] : 0.f;
    y[i] = o;
  }
}

__global__ __launch_bounds__(256) void psp_add_relu_bwd_kernel(const f4* __restrict__ g, const f4* __restrict__ y,
                                                               f4* __restrict__ gx, int64_t n4) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const f4 gv = g[i], yv = y[i];
    f4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = yv[k] > 0.f ? gv[k] : 0.f;
    gx[i] = o;
  }
}

}  // namespace sea

using namespace sea;

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

extern "C" int sea_psp_polyphase_split(const float* x, float* y, int B, int H, int W, int C, int d, int first_only,
                                       void* stream) {
  SEA_CHECK_ARG(x && y && x != y && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && d >= 1 && d <= 16 &&
                aligned16(x) && aligned16(y));
  const int Hs = (H + d - 1) / d, Ws = (W + d - 1) / d, P = first_only ? 1 : d * d;
  SEA_CHECK_ARG((int64_t)B * P * Hs < (1ll << 31) && (int64_t)Ws * (C / 4) < (1ll << 31) &&
                (int64_t)W * (C / 4) < (1ll << 31));
  dim3 grid;
  p1_grid(B * P * Hs, Ws * (C / 4), grid);
  hipLaunchKernelGGL(psp_split_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const f4*)x, (f4*)y, B * P * Hs, P, H,
                     W, Hs, Ws, C / 4, d);
  SEA_RETURN_LAST();
}

extern "C" int sea_psp_polyphase_merge(const float* y, float* x, int B, int H, int W, int C, int d, int first_only,
                                       void* stream) {
  SEA_CHECK_ARG(x && y && x != y && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && d >= 1 && d <= 16 &&
                aligned16(x) && aligned16(y));
  const int Hs = (H + d - 1) / d, Ws = (W + d - 1) / d, P = first_only ? 1 : d * d;
  SEA_CHECK_ARG((int64_t)B * H < (1ll << 31) && (int64_t)W * (C / 4) < (1ll << 31) &&
                (int64_t)Ws * (C / 4) < (1ll << 31));
  dim3 grid;
  p1_grid(B * H, W * (C / 4), grid);
  hipLaunchKernelGGL(psp_merge_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const f4*)y, (f4*)x, B * H, P, H, W,
                     Hs, Ws, C / 4, d);
  SEA_RETURN_LAST();
}

extern "C" int sea_psp_upsample_ac(const float* x, float* y, int64_t planes, int h, int w, int H, int W,
                                   void* stream) {
  SEA_CHECK_ARG(x && y && x != y && planes > 0 && h > 0 && w > 0 && H > 0 && W > 0);
  const int64_t total = planes * H * W;
  hipLaunchKernelGGL(psp_up_ac_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, x, y, total, h,
                     w, H, W, psp_ac_scale(h, H), psp_ac_scale(w, W));
  SEA_RETURN_LAST();
}

extern "C" int sea_psp_upsample_ac_bwd(const float* gy, float* gx, float* work, int64_t planes, int h, int w, int H,
                                       int W, void* stream) {
  SEA_CHECK_ARG(gy && gx && work && gx != gy && work != gy && work != gx && planes > 0 && h > 0 && w > 0 && H > 0 &&
                W > 0);
  const hipStream_t s = (hipStream_t)stream;
  const int64_t t1 = planes * H * w, t2 = planes * h * w;
  hipLaunchKernelGGL(psp_up_ac_bwd_w_kernel, dim3(grid_for(t1, 256)), dim3(256), 0, s, gy, work, t1, w, H, W,
                     psp_ac_scale(w, W));
  hipLaunchKernelGGL(psp_up_ac_bwd_h_kernel, dim3(grid_for(t2, 256)), dim3(256), 0, s, work, gx, t2, h, w, H,
                     psp_ac_scale(h, H));
  SEA_RETURN_LAST();
}

extern "C" int sea_psp_upsample_ac_nhwc(const float* x, float* y, int B, int C, int h, int w, int H, int W, int S,
                                        void* stream) {
  SEA_CHECK_ARG(x && y && x != y && B > 0 && C > 0 && C % 4 == 0 && S >= C && S % 4 == 0 && h > 0 && w > 0 && H > 0 &&
                W > 0 && aligned16(x) && aligned16(y));
  const int64_t total = (int64_t)B * H * W * (C / 4);
  hipLaunchKernelGGL(psp_up_ac_cl_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, (const f4*)x,
                     y, total, C / 4, h, w, H, W, S, psp_ac_scale(h, H), psp_ac_scale(w, W));
  SEA_RETURN_LAST();
}

extern "C" int sea_psp_upsample_ac_nhwc_bwd(const float* gy, float* gx, float* work, int B, int C, int h, int w, int H,
                                            int W, int S, void* stream) {
  SEA_CHECK_ARG(gy && gx && work && gx != gy && work != gy && work != gx && B > 0 && C > 0 && C % 4 == 0 && S >= C &&
                S % 4 == 0 && h > 0 && w > 0 && H > 0 && W > 0 && aligned16(gy) && aligned16(gx) && aligned16(work));
  const hipStream_t s = (hipStream_t)stream;
  const int64_t t1 = (int64_t)B * H * w * (C / 4), t2 = (int64_t)B * h * w * (C / 4);
  hipLaunchKernelGGL(psp_up_ac_cl_bwd_w_kernel, dim3(grid_for(t1, 256)), dim3(256), 0, s, gy, (f4*)work, t1, C / 4, w,
                     W, S, psp_ac_scale(w, W));
  hipLaunchKernelGGL(psp_up_ac_cl_bwd_h_kernel, dim3(grid_for(t2, 256)), dim3(256), 0, s, (const f4*)work, (f4*)gx, t2,
                     C / 4, h, w, H, psp_ac_scale(h, H));
  SEA_RETURN_LAST();
}

extern "C" int sea_psp_add_relu(const float* a, const float* r, float* y, int64_t n, void* stream) {
  SEA_CHECK_ARG(a && r && y && n > 0 && n % 4 == 0 && aligned16(a) && aligned16(r) && aligned16(y));
  hipLaunchKernelGGL(psp_add_relu_kernel, dim3(grid_for(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, (const f4*)a,
                     (const f4*)r, (f4*)y, n / 4);
  SEA_RETURN_LAST();
}

extern "C" int sea_psp_add_relu_bwd(const float* gy, const float* y, float* gx, int64_t n, void* stream) {
  SEA_CHECK_ARG(gy && y && gx && n > 0 && n % 4 == 0 && aligned16(gy) && aligned16(y) && aligned16(gx));
  hipLaunchKernelGGL(psp_add_relu_bwd_kernel, dim3(grid_for(n / 4, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const f4*)gy, (const f4*)y, (f4*)gx, n / 4);
  SEA_RETURN_LAST();
}
