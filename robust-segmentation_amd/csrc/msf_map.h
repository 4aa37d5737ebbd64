// The index maps of the multi-scale + flip evaluation (K10), shared by its forward (msf_kernels.hip) and its adjoints
// (msf_grad.hip): ATen's align_corners=True rule, the per-pixel gather plan of K10b and the resized logit it samples.
// Inline, so every includer contracts them under its own flags; both users are built with -ffp-contract=off.
#pragma once
#include <math.h>

#include "bilinear_map.h"

namespace sea {

struct AxisMapAC {
  int i0, i1;
  float lam;
};

// ATen's align_corners=True source index (area_pixel_compute_source_index + guard_index_and_lambda)
__device__ __forceinline__ AxisMapAC axis_map_ac(int dst, float scale, int n_in) {
  const float src = scale * (float)dst;
  AxisMapAC m;
  m.i0 = (int)src;                                   // src >= 0: truncation == floor
  if (m.i0 > n_in - 1) m.i0 = n_in - 1;
  float l = src - (float)m.i0;
  m.lam = l < 0.f ? 0.f : (l > 1.f ? 1.f : l);
  m.i1 = m.i0 + ((m.i0 < n_in - 1) ? 1 : 0);
  return m;
}

__host__ __device__ __forceinline__ float ac_scale(int n_in, int n_out) {
  return n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f;
}

__device__ __forceinline__ float lerp2_ac(float v00, float v01, float v10, float v11, float lx, float ly) {
  const float top = (1.f - lx) * v00 + lx * v01;
  const float bot = (1.f - lx) * v10 + lx * v11;
  return (1.f - ly) * top + ly * bot;
}

// first destination index whose axis_map_ac(.).i0 is >= t (n_out if none).  i0 does not decrease with dst (a float
// product with a non-negative constant is monotone, and so are truncation and the clamp), so the two loops make the
// estimate exact with respect to axis_map_ac whatever the rounding of scale * dst; scale 0 (n_out == 1 or n_in == 1)
// maps every index to 0.
__device__ __forceinline__ int first_dst_ge_msf(int t, float scale, int n_in, int n_out) {
  if (t <= 0) return 0;
  if (t > n_in - 1 || !(scale > 0.f)) return n_out;
  const float est = ceilf((float)t / scale);
  int d = est < (float)n_out ? (int)est : n_out;
  d = d < 0 ? 0 : d;
  while (d > 0 && axis_map_ac(d - 1, scale, n_in).i0 >= t) --d;
  while (d < n_out && axis_map_ac(d, scale, n_in).i0 < t) ++d;
  return d;
}

// ---- K10b ----------------------------------------------------------------------------------------------------------
// Per-pixel gather plan: the 2 scaled rows / 2 (mirrored) scaled columns of the align_corners=True resize and, in
// low-res mode, the M2 map of each of them onto the low-res grid.
struct MsfPlan {
  int64_t o00, o01, o10, o11;          // full-res mode: offsets of the 4 samples in a class plane
  int rr[4], cc[4];                    // low-res mode: rows (of scaled rows a0, a1) x cols (of scaled cols c0, c1)
  float rl0, rl1, cl0, cl1;            // M2 lambdas of those rows / cols
  float lx, ly;                        // lambdas of the align_corners=True resize
};

template <bool LOWRES>
__device__ __forceinline__ MsfPlan msf_plan(int oy, int ox, int Hs, int Ws, int hl, int wl, int H, int W, int flip) {
  MsfPlan pl;
  const AxisMapAC my = axis_map_ac(oy, ac_scale(Hs, H), Hs), mx = axis_map_ac(ox, ac_scale(Ws, W), Ws);
  const int c0 = flip ? Ws - 1 - mx.i0 : mx.i0, c1 = flip ? Ws - 1 - mx.i1 : mx.i1;
  pl.lx = mx.lam;
  pl.ly = my.lam;
  if constexpr (LOWRES) {
    const float rh = (float)hl / (float)Hs, rw = (float)wl / (float)Ws;    // = sea_upsample_bilinear_fwd
    const AxisMapU a0 = axis_map_u(my.i0, rh, hl), a1 = axis_map_u(my.i1, rh, hl);
    const AxisMapU b0 = axis_map_u(c0, rw, wl), b1 = axis_map_u(c1, rw, wl);
    pl.rr[0] = a0.i0; pl.rr[1] = a0.i1; pl.rr[2] = a1.i0; pl.rr[3] = a1.i1;
    pl.cc[0] = b0.i0; pl.cc[1] = b0.i1; pl.cc[2] = b1.i0; pl.cc[3] = b1.i1;
    pl.rl0 = a0.lam; pl.rl1 = a1.lam; pl.cl0 = b0.lam; pl.cl1 = b1.lam;
  } else {
    pl.o00 = (int64_t)my.i0 * Ws + c0;
    pl.o01 = (int64_t)my.i0 * Ws + c1;
    pl.o10 = (int64_t)my.i1 * Ws + c0;
    pl.o11 = (int64_t)my.i1 * Ws + c1;
  }
  return pl;
}

// the resized (and mirrored) logit of one class plane at the planned pixel
template <bool LOWRES>
__device__ __forceinline__ float msf_sample(const float* __restrict__ p, const MsfPlan& pl, int wl) {
  if constexpr (LOWRES) {
    // M2's value at a scaled-grid point: (1-ly)*((1-lx)*v00 + lx*v01) + ly*((1-lx)*v10 + lx*v11)
    const float* ra = p + (int64_t)pl.rr[0] * wl;
    const float* rb = p + (int64_t)pl.rr[1] * wl;
    const float* rc = p + (int64_t)pl.rr[2] * wl;
    const float* rd = p + (int64_t)pl.rr[3] * wl;
    const float s00 = lerp2_ac(ra[pl.cc[0]], ra[pl.cc[1]], rb[pl.cc[0]], rb[pl.cc[1]], pl.cl0, pl.rl0);
    const float s01 = lerp2_ac(ra[pl.cc[2]], ra[pl.cc[3]], rb[pl.cc[2]], rb[pl.cc[3]], pl.cl1, pl.rl0);
    const float s10 = lerp2_ac(rc[pl.cc[0]], rc[pl.cc[1]], rd[pl.cc[0]], rd[pl.cc[1]], pl.cl0, pl.rl1);
    const float s11 = lerp2_ac(rc[pl.cc[2]], rc[pl.cc[3]], rd[pl.cc[2]], rd[pl.cc[3]], pl.cl1, pl.rl1);
    return lerp2_ac(s00, s01, s10, s11, pl.lx, pl.ly);
  } else {
    return lerp2_ac(p[pl.o00], p[pl.o01], p[pl.o10], p[pl.o11], pl.lx, pl.ly);
  }
}

}  // namespace sea
