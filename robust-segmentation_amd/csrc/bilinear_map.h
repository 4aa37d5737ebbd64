// ATen's bilinear source-index rules.  align_corners=False: shared by the up-sampling kernels (M2), the fused
// FPN-bottleneck kernels (M6) and the fused criteria (K2u, T2u).  align_corners=True (at the end): shared by PSPNet's
// up-sampling (P2, psp_kernels.hip) and the criterion fused with it (T2u-ac, train_loss_up.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace sea {

struct AxisMapU {
  int i0, i1;
  float lam;
};

__device__ __forceinline__ AxisMapU axis_map_u(int dst, float r, int n_in) {
  float src = r * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  AxisMapU m;
  m.i0 = (int)src;
  if (m.i0 > n_in - 1) m.i0 = n_in - 1;
  m.i1 = m.i0 + ((m.i0 < n_in - 1) ? 1 : 0);
  m.lam = src - (float)m.i0;
  return m;
}

__device__ __forceinline__ int first_dst_ge(int t, float r, int n_in, int n_out) {
  if (t <= 0) return 0;
  if (t > n_in - 1) return n_out;
  int d = (int)ceilf(((float)t + 0.5f) / r - 0.5f);
  d = d < 0 ? 0 : (d > n_out ? n_out : d);
  while (d > 0 && axis_map_u(d - 1, r, n_in).i0 >= t) --d;
  while (d < n_out && axis_map_u(d, r, n_in).i0 < t) ++d;
  return d;
}

// Power-of-two factor S in this axis (n_out = S * n_in): with t = dst + S/2 the source pair is i0 = (t >> log2 S) - 1
// (negative: clamped to 0 with lambda = 0, exactly what the clamp of src does) and lambda = ((t & (S-1)) + 0.5) / S.
// r = 1/S and every intermediate of axis_map_u are exact in float for such factors: identical results, integer ops only.
// S = 0 selects the general float rule.
template <int S>
struct Pow2 {
  static constexpr int LOG = S == 2 ? 1 : S == 4 ? 2 : S == 8 ? 3 : 4;
  static_assert(S == 2 || S == 4 || S == 8 || S == 16, "supported factors");
};

template <int S>
__device__ __forceinline__ AxisMapU axis_map_p2(int dst, float r, int n_in) {
  if constexpr (S == 0) {
    return axis_map_u(dst, r, n_in);
  } else {
    constexpr int LOG = Pow2<S>::LOG;
    const int t = dst + S / 2;
    AxisMapU m;
    m.i0 = (t >> LOG) - 1;
    m.lam = ((float)(t & (S - 1)) + 0.5f) * (1.f / (float)S);
    if (m.i0 < 0) {
      m.i0 = 0;
      m.lam = 0.f;
    }
    m.i1 = min(m.i0 + 1, n_in - 1);
    return m;
  }
}

// weight of source index `src` in the interpolation of destination index `dst`
__device__ __forceinline__ float axis_coef(int dst, int src, float r, int n_in) {
  const AxisMapU m = axis_map_u(dst, r, n_in);
  return ((m.i0 == src) ? (1.f - m.lam) : 0.f) + ((m.i1 == src) ? m.lam : 0.f);
}

// ATen's expression tree of the four-tap sum (K2u, T2u): with it the fused criteria see F.interpolate's logits bit for bit.
// Inline, so it is contracted under its includer's flags; both users are built with the default ones.
__device__ __forceinline__ float lerp2(float v00, float v01, float v10, float v11, float lx, float ly) {
  const float top = (1.f - lx) * v00 + lx * v01;
  const float bot = (1.f - lx) * v10 + lx * v11;
  return (1.f - ly) * top + ly * bot;
}

// ---- align_corners=True (ATen's UpSampleBilinear2d.cu): scale = (in-1)/(out-1) in fp32 (0 for out == 1),
// src = scale*dst, i0 = (int)src, i1 = i0 + (i0 < in-1), l1 = src - i0, l0 = 1 - l1
__host__ __device__ __forceinline__ float psp_ac_scale(int n_in, int n_out) {
  return n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f;
}

struct AcMap {
  int i0, p;           // taps i0 and i0 + p
  float l0, l1;
};

__device__ __forceinline__ AcMap ac_map(int dst, float scale, int n_in) {
  const float src = scale * (float)dst;
  AcMap a;
  a.i0 = (int)src;
  a.p = (a.i0 < n_in - 1) ? 1 : 0;
  a.l1 = src - (float)a.i0;
  a.l0 = 1.f - a.l1;
  return a;
}

// l0y*(l0x*v00 + l1x*v01) + l1y*(l0x*v10 + l1x*v11) rounded exactly as ATen's compiled kernel rounds it (measured on
// MI355X against F.interpolate: each sum's FIRST product is fused, the second rounded on its own); written with explicit
// fmaf so that the result does not depend on how this translation unit's contraction happens to pair the terms
__device__ __forceinline__ float lerp_ac(float v00, float v01, float v10, float v11, const AcMap& mx, const AcMap& my) {
  const float t0 = fmaf(mx.l0, v00, mx.l1 * v01);
  const float t1 = fmaf(mx.l0, v10, mx.l1 * v11);
  return fmaf(my.l0, t0, my.l1 * t1);
}

// first destination index whose i0 is >= t (n_out if none): the inverse of ac_map, as first_dst_ge is of axis_map_u.
// i0 does not decrease with dst (a float product with a non-negative constant is monotone), so the two loops make the
// estimate exact with respect to ac_map whatever the rounding of scale * dst; scale 0 (n_in == 1) maps every index to 0.
__device__ __forceinline__ int first_dst_ge_ac(int t, float scale, int n_in, int n_out) {
  if (t <= 0) return 0;
  if (t > n_in - 1 || !(scale > 0.f)) return n_out;
  int d = (int)ceilf((float)t / scale);
  d = d < 0 ? 0 : (d > n_out ? n_out : d);
  while (d > 0 && ac_map(d - 1, scale, n_in).i0 >= t) --d;
  while (d < n_out && ac_map(d, scale, n_in).i0 < t) ++d;
  return d;
}

}  // namespace sea
