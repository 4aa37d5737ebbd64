// Multi-scale + flip evaluation (semseg.val.evaluate_msf, reference semseg/val.py:330-372): the two device steps of
// one (scale, flip) pass.
//
// K10a  input resize (+ flip): F.interpolate(images, (Hs, Ws), mode="bilinear", align_corners=True), optionally also
//      mirrored along W (torch.flip(dims=(3,))), both written in one pass.  ATen's arithmetic: scale = (in-1)/(out-1)
//      in fp32, src = scale*dst, i0 = (int)src clamped, lambda = src - i0 clamped to [0, 1], i1 = min(i0+1, in-1),
//      out = (1-ly)*((1-lx)*v00 + lx*v01) + ly*((1-lx)*v10 + lx*v11).  Built with -ffp-contract=off so that every
//      product and sum rounds separately, like the reference's CPU interpolation.
//
// K10b  accumulate: score[b, :, h, w] += softmax_C(resize_{align_corners=True}(flip?(logits)))[b, :, h, w].
//      Full-res mode: logits = model(x_s), (B, C, Hs, Ws).  Low-res mode: logits = forward_lowres(x_s), (B, C, hl, wl)
//      at 1/r of the scaled size; the model's own final up-sampling (align_corners=False, csrc/bilinear_map.h = M2) is
//      evaluated on the fly: each output pixel takes the 4 scaled-grid samples of the second resize, each from 2 x 2
//      low-res taps.  The (B, C, Hs, Ws) scaled-resolution logits never exist.  The flip is folded into the column
//      map: column c of the mirrored logits is column Ws-1-c of the model's output.
//      Softmax per pixel in fp32: max, sum of exps, divide.  Bytes per pass: score read + written once,
//      2*B*C*H*W*4, plus the logits (full-res mode: B*C*Hs*Ws*4; low-res mode r^2 times less).
//      Work split: a block owns consecutive pixels of one image; pixel = lane, so every load and store of a class
//      plane is a coalesced row segment.
//        C <= 32  (VOC): 128 pixels per block, one pixel per lane, 2 waves per pixel row take the even / odd classes
//                        (16 in registers each).  (One wave holding all 32 classes spilled 2 KB per lane to scratch.)
//        C <= 192 (ADE): 64 pixels per block, the 4 waves take classes q, q+4, ... (at most 48 in registers each).
//      The per-pixel max and sum are combined across the waves through LDS in a fixed order.
//      No atomics: every score element is read and written by one lane, results are bitwise reproducible.
#include <math.h>

#include "sea_common.h"
#include "bilinear_map.h"
#include "msf_map.h"

namespace sea {

// ---- K10a ----------------------------------------------------------------------------------------------------------
// one output pixel per lane, grid-stride over planes*H*W
__global__ __launch_bounds__(256) void msf_resize_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                         float* __restrict__ yf, int64_t total, int h, int w, int H,
                                                         int W, float sh, float sw) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int X = (int)(i % W);
    const int64_t t = i / W;
    const int Y = (int)(t % H);
    const int64_t plane = t / H;
    const AxisMapAC my = axis_map_ac(Y, sh, h), mx = axis_map_ac(X, sw, w);
    const float* p = x + plane * h * w;
    const float* r0 = p + (int64_t)my.i0 * w;
    const float* r1 = p + (int64_t)my.i1 * w;
    const float v = lerp2_ac(r0[mx.i0], r0[mx.i1], r1[mx.i0], r1[mx.i1], mx.lam, my.lam);
    if (y) y[i] = v;
    if (yf) yf[(plane * H + Y) * W + (W - 1 - X)] = v;
  }
}

// ---- K10b ----------------------------------------------------------------------------------------------------------
// (gather plan and sample: msf_map.h)
// NQ thread groups (256/NQ lanes each) split the classes (c = q + NQ*k, k < CPT); pixel = lane within the group, so a
// block covers 256/NQ consecutive pixels of image blockIdx.y.
template <int NQ, int CPT, bool LOWRES>
__global__ __launch_bounds__(256) void msf_accumulate_kernel(const float* __restrict__ logits,
                                                             float* __restrict__ score, int C, int hl, int wl, int Hs,
                                                             int Ws, int H, int W, int flip) {
  constexpr int PIX = 256 / NQ;
  __shared__ float red_m[NQ][PIX], red_s[NQ][PIX];
  const int lane = threadIdx.x % PIX, q = threadIdx.x / PIX;
  const int b = blockIdx.y;
  const int HW = H * W;
  const int pix = blockIdx.x * PIX + lane;
  const bool valid = pix < HW;
  const int64_t lplane = LOWRES ? (int64_t)hl * wl : (int64_t)Hs * Ws;
  const float* lb = logits + (int64_t)b * C * lplane;
  float* sb = score + (int64_t)b * C * HW + pix;
  float v[CPT];
  float m = -INFINITY;
  if (valid) {
    const MsfPlan pl = msf_plan<LOWRES>(pix / W, pix % W, Hs, Ws, hl, wl, H, W, flip);
    const float* pc = lb + q * lplane;
#pragma unroll
    for (int k = 0; k < CPT; ++k, pc += NQ * lplane) {
      if (q + NQ * k < C) {
        v[k] = msf_sample<LOWRES>(pc, pl, wl);
        m = fmaxf(m, v[k]);
      }
    }
  }
  if constexpr (NQ > 1) {
    red_m[q][lane] = m;
    __syncthreads();
    m = red_m[0][lane];
#pragma unroll
    for (int j = 1; j < NQ; ++j) m = fmaxf(m, red_m[j][lane]);
  }
  float s = 0.f;
  if (valid) {
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      if (q + NQ * k < C) {
        v[k] = expf(v[k] - m);
        s += v[k];
      }
    }
  }
  if constexpr (NQ > 1) {
    red_s[q][lane] = s;
    __syncthreads();
    s = red_s[0][lane];
#pragma unroll
    for (int j = 1; j < NQ; ++j) s += red_s[j][lane];
  }
  if (!valid) return;
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    const int c = q + NQ * k;
    if (c < C) {
      float* o = sb + (int64_t)c * HW;
      *o = *o + v[k] / s;
    }
  }
}

template <bool LOWRES>
static void launch_accumulate(const float* logits, float* score, int B, int C, int hl, int wl, int Hs, int Ws, int H,
                              int W, int flip, hipStream_t s) {
  const int HW = H * W;
  if (C <= 32) {
    const dim3 grid((HW + 127) / 128, B);
    hipLaunchKernelGGL((msf_accumulate_kernel<2, 16, LOWRES>), grid, dim3(256), 0, s, logits, score, C, hl, wl, Hs, Ws,
                       H, W, flip);
  } else {
    const dim3 grid((HW + 63) / 64, B);
    hipLaunchKernelGGL((msf_accumulate_kernel<4, 48, LOWRES>), grid, dim3(256), 0, s, logits, score, C, hl, wl, Hs, Ws,
                       H, W, flip);
  }
}

}  // namespace sea

using namespace sea;

extern "C" int sea_msf_resize_input(const float* x, float* y, float* y_flip, int64_t planes, int h, int w, int H, int W,
                                    void* stream) {
  SEA_CHECK_ARG(x && (y || y_flip) && planes > 0 && h > 0 && w > 0 && H > 0 && W > 0);
  const int64_t total = planes * H * W;
  const dim3 grid(grid_for(total, 256)), block(256);
  hipLaunchKernelGGL(msf_resize_kernel, grid, block, 0, (hipStream_t)stream, x, y, y_flip, total, h, w, H, W,
                     ac_scale(h, H), ac_scale(w, W));
  SEA_RETURN_LAST();
}

extern "C" int sea_msf_accumulate(const float* logits, float* score, int B, int C, int hl, int wl, int Hs, int Ws, int H,
                                  int W, int flip, void* stream) {
  SEA_CHECK_ARG(logits && score && B > 0 && B <= 65535 && C > 0 && C <= SEA_MSF_MAX_CLASSES && hl > 0 && wl > 0 &&
                hl <= Hs && wl <= Ws && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31) &&
                (int64_t)Hs * Ws < (1ll << 31));
  const hipStream_t s = (hipStream_t)stream;
  if (hl == Hs && wl == Ws)
    launch_accumulate<false>(logits, score, B, C, hl, wl, Hs, Ws, H, W, flip ? 1 : 0, s);
  else
    launch_accumulate<true>(logits, score, B, C, hl, wl, Hs, Ws, H, W, flip ? 1 : 0, s);
  SEA_RETURN_LAST();
}
