// The adjoints of the multi-scale + flip evaluation (K10, msf_kernels.hip), for the attack through the ensemble
// (semseg.utils.msf_model.MsfModel).  Every index and weight comes from the forward's own device functions (msf_map.h,
// bilinear_map.h); built with -ffp-contract=off like the forward, so every product and sum rounds separately.
//
// K10r' adjoint of the align_corners=True bilinear resize (h, w) -> (H, W), a gather with one lane per SOURCE element
//      (of 8 consecutive planes, whose maps are the same), lanes = consecutive source columns.  The destination rows
//      that reference source row i are those whose forward map has i0 in {i - 1, i}: the range
//      [first_dst_ge_msf(i - 1), first_dst_ge_msf(i + 1)), an estimate settled by evaluating axis_map_ac itself (no
//      second closed formula); columns alike.  Summation order of one element, fp32, from 0.f:
//          for Y ascending, for X ascending, row tap 0 (i0 == i, weight 1 - ly) before row tap 1 (i1 == i, weight ly),
//          inside a row tap column tap 0 (1 - lx) before column tap 1 (lx):   acc += (wy * wx) * g[p, Y, X]
//      A clamped border pixel (i1 == i0) contributes both of its terms, as in the forward; a tap of weight 0 (H == h)
//      still adds its 0.  A source element that no destination references is written 0.f.
//      Two sites.  K10a' (input): g is the gradient of the plain scaled image and / or g_flip that of the mirrored one
//      (the forward wrote yf[.., W-1-X] = y[.., X]); all plain terms first, then all mirrored ones in the same order of
//      (Y, X), reading g_flip[p, Y, W-1-X].  Phase B of K10b' (src_flip): the mirror is on the SOURCE columns, source
//      column c is index w-1-c of the map, as in msf_plan.
// K10g softmax backward at label resolution: per pixel the resized logits v_c as K10b computes them (msf_plan /
//      msf_sample, both modes, flip), p = softmax(v) with K10b's max, exps, sum and quotient, t = sum_c p_c * d_c and
//      G_c = p_c * (d_c - t) for d = dL/dscore.  K10b's work split (C <= 32: two groups of 128 pixels, C <= 192: four of
//      64; classes in registers).  t: every group adds its classes c = q, q + NQ, ... ascending from 0.f, then the
//      groups' partial sums are added in group order 0 .. NQ-1 through LDS (the order of K10b's sum of exps).
// The backward of one pass = K10g into the workspace G (B, C, H, W), then K10r' (src_flip = flip) onto the scaled grid.
// No atomics anywhere: every output element is written by one lane, results are bitwise reproducible.
#include <math.h>

#include "sea_common.h"
#include "bilinear_map.h"
#include "msf_map.h"

namespace sea {

// ---- K10r' ---------------------------------------------------------------------------------------------------------
// The maps depend on the source element (r, j) alone, not on the plane: a lane owns element (r, j) of kPlanesPerLane
// consecutive planes, computes ranges, taps and weights once and walks the planes innermost (independent loads in
// flight).  Every plane's sum still runs in the documented order.
constexpr int kPlanesPerLane = 8;

__device__ __forceinline__ void resize_bwd_terms(float (&acc)[kPlanesPerLane], const float* __restrict__ gp, int np,
                                                 int64_t HW, bool mirrored, int r, int jm, int y0, int y1, int x0,
                                                 int x1, int h, int w, int W, float sh, float sw) {
  for (int Y = y0; Y < y1; ++Y) {
    const AxisMapAC my = axis_map_ac(Y, sh, h);
    const bool r0 = my.i0 == r, r1 = my.i1 == r;
    const float wy0 = 1.f - my.lam, wy1 = my.lam;
    const float* row = gp + (int64_t)Y * W;
    for (int X = x0; X < x1; ++X) {
      const AxisMapAC mx = axis_map_ac(X, sw, w);
      const bool c0 = mx.i0 == jm, c1 = mx.i1 == jm;
      const float wx0 = 1.f - mx.lam, wx1 = mx.lam;
      const float w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;
      const float* px = row + (mirrored ? W - 1 - X : X);
#pragma unroll
      for (int p = 0; p < kPlanesPerLane; ++p) {
        if (p < np) {
          const float gv = px[p * HW];
          if (r0 && c0) acc[p] += w00 * gv;
          if (r0 && c1) acc[p] += w01 * gv;
          if (r1 && c0) acc[p] += w10 * gv;
          if (r1 && c1) acc[p] += w11 * gv;
        }
      }
    }
  }
}

// grid.x covers the h*w source elements of a plane (lanes = consecutive source columns), grid.y strides over the groups of
// kPlanesPerLane planes
__global__ __launch_bounds__(256) void msf_resize_bwd_kernel(const float* __restrict__ g, const float* __restrict__ gf,
                                                             float* __restrict__ dsrc, int64_t planes, int h, int w,
                                                             int H, int W, float sh, float sw, int src_flip) {
  const int64_t hw = (int64_t)h * w, HW = (int64_t)H * W;
  const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (idx >= hw) return;
  const int j = (int)(idx % w), r = (int)(idx / w);
  const int jm = src_flip ? w - 1 - j : j;
  const int y0 = first_dst_ge_msf(r - 1, sh, h, H), y1 = first_dst_ge_msf(r + 1, sh, h, H);
  const int x0 = first_dst_ge_msf(jm - 1, sw, w, W), x1 = first_dst_ge_msf(jm + 1, sw, w, W);
  for (int64_t p0 = (int64_t)blockIdx.y * kPlanesPerLane; p0 < planes; p0 += (int64_t)gridDim.y * kPlanesPerLane) {
    const int np = planes - p0 < kPlanesPerLane ? (int)(planes - p0) : kPlanesPerLane;
    float acc[kPlanesPerLane];
#pragma unroll
    for (int p = 0; p < kPlanesPerLane; ++p) acc[p] = 0.f;
    if (g) resize_bwd_terms(acc, g + p0 * HW, np, HW, false, r, jm, y0, y1, x0, x1, h, w, W, sh, sw);
    if (gf) resize_bwd_terms(acc, gf + p0 * HW, np, HW, true, r, jm, y0, y1, x0, x1, h, w, W, sh, sw);
    float* out = dsrc + p0 * hw + idx;
#pragma unroll
    for (int p = 0; p < kPlanesPerLane; ++p)
      if (p < np) out[p * hw] = acc[p];
  }
}

static void launch_resize_bwd(const float* g, const float* gf, float* dsrc, int64_t planes, int h, int w, int H, int W,
                              int src_flip, hipStream_t s) {
  const int64_t hw = (int64_t)h * w, groups = (planes + kPlanesPerLane - 1) / kPlanesPerLane;
  const dim3 grid((unsigned)((hw + 255) / 256), (unsigned)(groups < 65535 ? groups : 65535));
  hipLaunchKernelGGL(msf_resize_bwd_kernel, grid, dim3(256), 0, s, g, gf, dsrc, planes, h, w, H, W, ac_scale(h, H),
                     ac_scale(w, W), src_flip);
}

// ---- K10g ----------------------------------------------------------------------------------------------------------
// NQ thread groups (256/NQ lanes each) split the classes (c = q + NQ*k, k < CPT); pixel = lane within the group, so a
// block covers 256/NQ consecutive pixels of image blockIdx.y (msf_accumulate_kernel's split).
template <int NQ, int CPT, bool LOWRES>
__global__ __launch_bounds__(256) void msf_softmax_bwd_kernel(const float* __restrict__ logits,
                                                              const float* __restrict__ dscore, float* __restrict__ G,
                                                              int C, int hl, int wl, int Hs, int Ws, int H, int W,
                                                              int flip) {
  constexpr int PIX = 256 / NQ;
  __shared__ float red_m[NQ][PIX], red_s[NQ][PIX], red_t[NQ][PIX];
  const int lane = threadIdx.x % PIX, q = threadIdx.x / PIX;
  const int b = blockIdx.y;
  const int HW = H * W;
  const int pix = blockIdx.x * PIX + lane;
  const bool valid = pix < HW;
  const int64_t lplane = LOWRES ? (int64_t)hl * wl : (int64_t)Hs * Ws;
  const float* lb = logits + (int64_t)b * C * lplane;
  const float* db = dscore + (int64_t)b * C * HW + pix;
  float* gb = G + (int64_t)b * C * HW + pix;
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
  red_m[q][lane] = m;
  __syncthreads();
  m = red_m[0][lane];
#pragma unroll
  for (int j = 1; j < NQ; ++j) m = fmaxf(m, red_m[j][lane]);
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
  red_s[q][lane] = s;
  __syncthreads();
  s = red_s[0][lane];
#pragma unroll
  for (int j = 1; j < NQ; ++j) s += red_s[j][lane];
  float t = 0.f;
  if (valid) {
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      const int c = q + NQ * k;
      if (c < C) {
        v[k] = v[k] / s;                                  // p_c, K10b's quotient
        t += v[k] * db[(int64_t)c * HW];
      }
    }
  }
  red_t[q][lane] = t;
  __syncthreads();
  t = red_t[0][lane];
#pragma unroll
  for (int j = 1; j < NQ; ++j) t += red_t[j][lane];
  if (!valid) return;
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    const int c = q + NQ * k;
    if (c < C) gb[(int64_t)c * HW] = v[k] * (db[(int64_t)c * HW] - t);     // d is read again (L2) instead of kept
  }
}

template <bool LOWRES>
static void launch_softmax_bwd(const float* logits, const float* dscore, float* G, int B, int C, int hl, int wl, int Hs,
                               int Ws, int H, int W, int flip, hipStream_t s) {
  const int HW = H * W;
  if (C <= 32) {
    const dim3 grid((HW + 127) / 128, B);
    hipLaunchKernelGGL((msf_softmax_bwd_kernel<2, 16, LOWRES>), grid, dim3(256), 0, s, logits, dscore, G, C, hl, wl, Hs,
                       Ws, H, W, flip);
  } else {
    const dim3 grid((HW + 63) / 64, B);
    hipLaunchKernelGGL((msf_softmax_bwd_kernel<4, 48, LOWRES>), grid, dim3(256), 0, s, logits, dscore, G, C, hl, wl, Hs,
                       Ws, H, W, flip);
  }
}

}  // namespace sea

using namespace sea;

extern "C" int sea_msf_resize_bwd(const float* g, const float* g_flip, float* dsrc, int64_t planes, int h, int w, int H,
                                  int W, int src_flip, void* stream) {
  SEA_CHECK_ARG((g || g_flip) && dsrc && dsrc != g && dsrc != g_flip && planes > 0 && h > 0 && w > 0 && H > 0 && W > 0 &&
                (int64_t)h * w < (1ll << 31) && (int64_t)H * W < (1ll << 31));
  launch_resize_bwd(g, g_flip, dsrc, planes, h, w, H, W, src_flip ? 1 : 0, (hipStream_t)stream);
  SEA_RETURN_LAST();
}

extern "C" int sea_msf_accumulate_bwd(const float* logits, const float* dscore, float* G, float* dscaled, int B, int C,
                                      int hl, int wl, int Hs, int Ws, int H, int W, int flip, void* stream) {
  SEA_CHECK_ARG(logits && dscore && G && dscaled && B > 0 && B <= 65535 && C > 0 && C <= SEA_MSF_MAX_CLASSES && hl > 0 &&
                wl > 0 && hl <= Hs && wl <= Ws && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31) &&
                (int64_t)Hs * Ws < (1ll << 31));
  SEA_CHECK_ARG(G != logits && G != dscore && dscaled != logits && dscaled != dscore && dscaled != G);
  const hipStream_t s = (hipStream_t)stream;
  if (hl == Hs && wl == Ws)
    launch_softmax_bwd<false>(logits, dscore, G, B, C, hl, wl, Hs, Ws, H, W, flip ? 1 : 0, s);
  else
    launch_softmax_bwd<true>(logits, dscore, G, B, C, hl, wl, Hs, Ws, H, W, flip ? 1 : 0, s);
  launch_resize_bwd(G, nullptr, dscaled, (int64_t)B * C, Hs, Ws, H, W, flip ? 1 : 0, s);
  SEA_RETURN_LAST();
}
