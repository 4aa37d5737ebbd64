// M6 (model side): the FPN bottleneck of the UperNet head without up-sampling its coarse inputs
// (semseg/models/uperforseg.py:255-262:  fpn_bottleneck(cat([f0, up(f1), up(f2), up(f3)]))).
//
// A 3x3 convolution is  sum_taps Shift_tap o W_tap  with W_tap a pure channel mixing, and channel mixing commutes
// with bilinear up-sampling:  W_tap up(f) = up(W_tap f).  For an input that is an x4 / x8 up-sampling the nine
// channel mixings therefore run at the COARSE resolution (one GEMM, 16x / 64x fewer rows than at the output
// resolution, 4x / 16x fewer multiplications than even Winograd F(4x4,3x3)), and what is left at the output
// resolution is HBM-bound:
//   forward :  extra[b,Y,X,:] (+)= sum_{a,b in 3x3, (Y+a-1, X+b-1) inside} bilinear(G[..., tap(a,b), :])(Y+a-1, X+b-1)
//              G = f @ W  laid out (B,h,w,9,C); `extra` enters the Winograd output transform as an addend
//   backward:  dG[b,y,x,tap,:] = sum over the bilinear footprint (P,Q) of (y,x) of wy(P,y) wx(Q,x) gz[b,P-a+1,Q-b+1,:]
//              then df = dG @ W^T at the coarse resolution
// Lanes run along channels (float4): every access is coalesced; the 9 taps share one pass over the footprint window.
#include "sea_common.h"
#include <utility>
#include "bilinear_map.h"
#include "upsample_plan.h"

namespace sea {

// One lane = (4x4 block of output pixels, 4 channels).  For an up-sampling factor >= 3 the four sample positions
// of one tap row / column touch at most 3 coarse rows / columns, so per tap a 3x3 coarse window (9 loads) feeds all
// 16 outputs through separable weights: 81 loads per 16 outputs instead of 36 per output (the plain gather was
// bound by L2 bandwidth at 16 TB/s of corner re-reads).
constexpr int kTB = kTapBlock;  // (upsample_plan.h: the plan counts the blocks)

// ---- interior blocks of a power-of-two factor: every weight is a compile-time constant ----------------------------------
// For S = 4 / 8 the sample rows P = Y0 + q + a - 1 of a 4 x 4 block (Y0 a multiple of 4, phase Y0 mod S) map to
// i0 = cy + (u >> log2 S) - 1, lambda = ((u & (S - 1)) + 0.5) / S with u = phase + q + a - 1 + S / 2 (axis_map_p2; cy = Y0 / S):
// away from the borders nothing depends on the block but cy.  The general loop above evaluates 24 weights per tap and lane
// (compares and selects around the float maps: as many VALU instructions as the interpolation itself) and multiplies by the
// third of them that is zero; here the two live weights per sample are immediates and the dead products are not issued:
// 208 -> us for the 16 x 16 -> 128 x 128 level (profiles/r6_tap_gather_ab.log).  Rounding differs from the general path in
// the last bit (the tap's contribution goes into the accumulator term by term instead of as one sum).
typedef float tg_f4 __attribute__((ext_vector_type(4)));

template <int N, typename F, int... I>
__device__ __forceinline__ void tg_static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void tg_static_for(F&& f) {
  tg_static_for_impl<N>(f, std::make_integer_sequence<int, N>{});
}

template <int S>
struct TgAxis {   // one axis of one tap: u0 = phase + a - 1 + S / 2
  static constexpr int LOG = Pow2<S>::LOG;
  static constexpr int base(int u0) { return (u0 >> LOG) - 1; }                               // ib - c
  static constexpr int k(int u0, int q) { return ((u0 + q) >> LOG) - (u0 >> LOG); }          // i0 - ib: 0 or 1
  static constexpr float lam(int u0, int q) { return ((float)((u0 + q) & (S - 1)) + 0.5f) / (float)S; }
};

template <int S, int PHY, int PHX>
__device__ __forceinline__ void tap_gather_inner(const float4* __restrict__ Gb, int cy, int cx, int w, int CG, tg_f4 (&acc)[kTB][kTB]) {
  using AX = TgAxis<S>;
  tg_static_for<9>([&](auto T) {
    constexpr int tap = decltype(T)::value;
    constexpr int a = tap / 3, bq = tap % 3;
    constexpr int uy = PHY + a - 1 + S / 2, ux = PHX + bq - 1 + S / 2;
    constexpr int NR = AX::k(uy, kTB - 1) + 2, NC = AX::k(ux, kTB - 1) + 2;                   // coarse rows / columns in use
    const int ib = cy + AX::base(uy), jb = cx + AX::base(ux);
    tg_f4 g[NR][NC];
#pragma unroll
    for (int k = 0; k < NR; ++k)
#pragma unroll
      for (int l = 0; l < NC; ++l) g[k][l] = *(const tg_f4*)(Gb + (uint32_t)((((ib + k) * w + jb + l) * 9 + tap) * CG));
#pragma unroll
    for (int py = 0; py < kTB; ++py) {
      const int ky = AX::k(uy, py);
      const float ly = AX::lam(uy, py);
      tg_f4 t[NC];
#pragma unroll
      for (int l = 0; l < NC; ++l) t[l] = __builtin_elementwise_fma(tg_f4{ly, ly, ly, ly}, g[ky + 1][l], (1.f - ly) * g[ky][l]);
#pragma unroll
      for (int px = 0; px < kTB; ++px) {
        const int kx = AX::k(ux, px);
        const float lx = AX::lam(ux, px);
        acc[py][px] = __builtin_elementwise_fma(tg_f4{1.f - lx, 1.f - lx, 1.f - lx, 1.f - lx}, t[kx], acc[py][px]);
        acc[py][px] = __builtin_elementwise_fma(tg_f4{lx, lx, lx, lx}, t[kx + 1], acc[py][px]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);     // (one tap's loads at a time, as in the general loop)
  });
}

template <int S>  // S = 4 / 8: that power-of-two factor in both axes (integer source map), 0: any factor >= 3
__global__ __launch_bounds__(256) void tap_gather_fwd_kernel(const float4* __restrict__ G, float4* __restrict__ extra,
                                                             int accumulate, int CG, int h, int w, int H, int W, float rh,
                                                             float rw, int nBh, int nBw, int64_t total, int xcd,
                                                             Divs3 dv, int inner_ok) {
  const IndexRange rg = xcd_range(total, xcd);
  const bool fast = total < kFastIndexLimit;
  for (int64_t i = rg.begin; i < rg.end; i += rg.stride) {
    const Index4 ix = split_index(i, dv, fast);  // (cg, bx, by, b)
    const int cg = ix.c0, bx = ix.c1, by = ix.c2;
    const int b = (int)ix.c3;
    const int Y0 = by * kTB, X0 = bx * kTB;
    float4 acc[kTB][kTB];
    float4* eb = extra + (int64_t)b * H * W * CG + cg;
#pragma unroll
    for (int py = 0; py < kTB; ++py)
#pragma unroll
      for (int px = 0; px < kTB; ++px)
        acc[py][px] = (accumulate && Y0 + py < H && X0 + px < W) ? eb[(uint32_t)(((Y0 + py) * W + X0 + px) * CG)]
                                                                 : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4* Gb = G + (int64_t)b * h * w * 9 * CG + cg;
    if constexpr (S == 4 || S == 8) {
      if (inner_ok && Y0 - 1 >= S / 2 && Y0 + kTB + S / 2 < H && X0 - 1 >= S / 2 && X0 + kTB + S / 2 < W) {
        tg_f4 (&va)[kTB][kTB] = reinterpret_cast<tg_f4 (&)[kTB][kTB]>(acc);
        const int cy = Y0 / S, cx = X0 / S;
        if constexpr (S == 4) {
          tap_gather_inner<4, 0, 0>(Gb, cy, cx, w, CG, va);
        } else {
          const int ph = ((Y0 >> 2) & 1) * 2 + ((X0 >> 2) & 1);
          if (ph == 0) tap_gather_inner<8, 0, 0>(Gb, cy, cx, w, CG, va);
          else if (ph == 1) tap_gather_inner<8, 0, 4>(Gb, cy, cx, w, CG, va);
          else if (ph == 2) tap_gather_inner<8, 4, 0>(Gb, cy, cx, w, CG, va);
          else tap_gather_inner<8, 4, 4>(Gb, cy, cx, w, CG, va);
        }
#pragma unroll
        for (int py = 0; py < kTB; ++py)
#pragma unroll
          for (int px = 0; px < kTB; ++px) eb[(uint32_t)(((Y0 + py) * W + X0 + px) * CG)] = acc[py][px];
        continue;
      }
    }
#pragma unroll 1  // one tap at a time: 9 loads in flight, ~150 VGPRs (fully unrolled the 81 loads spill)
    for (int tap = 0; tap < 9; ++tap) {
      const int a = tap / 3, bq = tap - a * 3;
      // wy[py][k] = weight of coarse row ib + k for the sample row P = Y0+py+a-1 (0 outside the image); same for columns
      const int ib = axis_map_p2<S>(min(max(Y0 + a - 1, 0), H - 1), rh, h).i0;
      const int jb = axis_map_p2<S>(min(max(X0 + bq - 1, 0), W - 1), rw, w).i0;
      float wy[kTB][3], wx[kTB][3];
#pragma unroll
      for (int q = 0; q < kTB; ++q) {
        const int P = Y0 + q + a - 1, Q = X0 + q + bq - 1;
        const bool oky = P >= 0 && P < H, okx = Q >= 0 && Q < W;
        const AxisMapU mp = axis_map_p2<S>(P, rh, h), mq = axis_map_p2<S>(Q, rw, w);  // one map per sample row / column
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float cy = ((mp.i0 == ib + k) ? (1.f - mp.lam) : 0.f) + ((mp.i1 == ib + k) ? mp.lam : 0.f);
          const float cx = ((mq.i0 == jb + k) ? (1.f - mq.lam) : 0.f) + ((mq.i1 == jb + k) ? mq.lam : 0.f);
          wy[q][k] = oky ? cy : 0.f;
          wx[q][k] = okx ? cx : 0.f;
        }
      }
      float4 g[3][3];
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int l = 0; l < 3; ++l)
          g[k][l] = Gb[(uint32_t)(((min(ib + k, h - 1) * w + min(jb + l, w - 1)) * 9 + tap) * CG)];
#pragma unroll
      for (int py = 0; py < kTB; ++py) {
        float4 t[3];
#pragma unroll
        for (int l = 0; l < 3; ++l) {
          t[l].x = wy[py][0] * g[0][l].x + wy[py][1] * g[1][l].x + wy[py][2] * g[2][l].x;
          t[l].y = wy[py][0] * g[0][l].y + wy[py][1] * g[1][l].y + wy[py][2] * g[2][l].y;
          t[l].z = wy[py][0] * g[0][l].z + wy[py][1] * g[1][l].z + wy[py][2] * g[2][l].z;
          t[l].w = wy[py][0] * g[0][l].w + wy[py][1] * g[1][l].w + wy[py][2] * g[2][l].w;
        }
#pragma unroll
        for (int px = 0; px < kTB; ++px) {
          const float c0 = wx[px][0], c1 = wx[px][1], c2 = wx[px][2];
          acc[py][px].x += c0 * t[0].x + c1 * t[1].x + c2 * t[2].x;
          acc[py][px].y += c0 * t[0].y + c1 * t[1].y + c2 * t[2].y;
          acc[py][px].z += c0 * t[0].z + c1 * t[1].z + c2 * t[2].z;
          acc[py][px].w += c0 * t[0].w + c1 * t[1].w + c2 * t[2].w;
        }
      }
    }
#pragma unroll
    for (int py = 0; py < kTB; ++py)
#pragma unroll
      for (int px = 0; px < kTB; ++px)
        if (Y0 + py < H && X0 + px < W) eb[(uint32_t)(((Y0 + py) * W + X0 + px) * CG)] = acc[py][px];
  }
}

// one lane = (coarse pixel, 4 channels): a single pass over the (footprint + 1 ring) window of gz feeds all 9 taps
__global__ __launch_bounds__(256) void tap_gather_bwd_kernel(const float4* __restrict__ gz, float4* __restrict__ dG, int CG,
                                                             int h, int w, int H, int W, float rh, float rw,
                                                             int64_t total, int xcd, Divs3 dv) {
  const IndexRange rg = xcd_range(total, xcd);
  const bool fast = total < kFastIndexLimit;
  for (int64_t i = rg.begin; i < rg.end; i += rg.stride) {
    const Index4 ix = split_index(i, dv, fast);  // (cg, xq, yq, b)
    const int cg = ix.c0, xq = ix.c1, yq = ix.c2;
    const int b = (int)ix.c3;
    const int Plo = first_dst_ge(yq - 1, rh, h, H), Phi = first_dst_ge(yq + 1, rh, h, H);
    const int Qlo = first_dst_ge(xq - 1, rw, w, W), Qhi = first_dst_ge(xq + 1, rw, w, W);
    const int R0 = max(Plo - 1, 0), R1 = min(Phi + 1, H), S0 = max(Qlo - 1, 0), S1 = min(Qhi + 1, W);
    const float4* gb = gz + (int64_t)b * H * W * CG + cg;
    float4 acc[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int bq = 0; bq < 3; ++bq) acc[a][bq] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int R = R0; R < R1; ++R) {
      float wya[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int P = R + a - 1;  // the tap-a source row that reads gz row R
        wya[a] = (P >= Plo && P < Phi) ? axis_coef(P, yq, rh, h) : 0.f;
      }
      if (wya[0] == 0.f && wya[1] == 0.f && wya[2] == 0.f) continue;
      float4 rb[3];
#pragma unroll
      for (int bq = 0; bq < 3; ++bq) rb[bq] = make_float4(0.f, 0.f, 0.f, 0.f);
      // sliding column coefficients: c[bq] = weight of Q = S + bq - 1
      float c0 = (S0 - 1 >= Qlo && S0 - 1 < Qhi) ? axis_coef(S0 - 1, xq, rw, w) : 0.f;
      float c1 = (S0 >= Qlo && S0 < Qhi) ? axis_coef(S0, xq, rw, w) : 0.f;
      for (int S = S0; S < S1; ++S) {
        const float c2 = (S + 1 >= Qlo && S + 1 < Qhi) ? axis_coef(S + 1, xq, rw, w) : 0.f;
        const float4 g = gb[((int64_t)R * W + S) * CG];
        rb[0].x = fmaf(c0, g.x, rb[0].x); rb[0].y = fmaf(c0, g.y, rb[0].y); rb[0].z = fmaf(c0, g.z, rb[0].z); rb[0].w = fmaf(c0, g.w, rb[0].w);
        rb[1].x = fmaf(c1, g.x, rb[1].x); rb[1].y = fmaf(c1, g.y, rb[1].y); rb[1].z = fmaf(c1, g.z, rb[1].z); rb[1].w = fmaf(c1, g.w, rb[1].w);
        rb[2].x = fmaf(c2, g.x, rb[2].x); rb[2].y = fmaf(c2, g.y, rb[2].y); rb[2].z = fmaf(c2, g.z, rb[2].z); rb[2].w = fmaf(c2, g.w, rb[2].w);
        c0 = c1;
        c1 = c2;
      }
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int bq = 0; bq < 3; ++bq) {
          acc[a][bq].x = fmaf(wya[a], rb[bq].x, acc[a][bq].x);
          acc[a][bq].y = fmaf(wya[a], rb[bq].y, acc[a][bq].y);
          acc[a][bq].z = fmaf(wya[a], rb[bq].z, acc[a][bq].z);
          acc[a][bq].w = fmaf(wya[a], rb[bq].w, acc[a][bq].w);
        }
    }
    float4* out = dG + (((int64_t)b * h + yq) * w + xq) * 9 * CG + cg;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int bq = 0; bq < 3; ++bq) out[(a * 3 + bq) * CG] = acc[a][bq];
  }
}

// Power-of-two factor S (x4 and x8 in UperNet): the footprint of coarse pixel (yq, xq) is the 2S x 2S window at
// (S*yq - S/2, S*xq - S/2) with constant separable weights (upsample_kernels.hip: upsample_bwd_pow2_kernel), so the
// window + ring of gz is (2S+2)^2: a row is 2S+2 independent 16-byte loads and 3 x 2S fused multiply-adds per channel
// with compile-time weights, instead of one dependent load and three float source-index evaluations per element.
template <int S>
__device__ __forceinline__ float pow2_tap_weight(int t, bool e_lo, bool e_hi) {
  // weight of window position t in [0, 2S) (0 outside); e_lo / e_hi: the coarse pixel is the first / last of its axis
  if (t < 0 || t >= 2 * S) return 0.f;
  constexpr float inv = 1.f / (float)S;
  const float c = (t < S) ? ((float)t + 0.5f) * inv : ((float)(2 * S - t) - 0.5f) * inv;
  if (t < S / 2) return e_lo ? 0.f : c;
  if (t < S) return e_lo ? 1.f : c;
  if (t < 3 * S / 2) return e_hi ? 1.f : c;
  return e_hi ? 0.f : c;
}

template <int S>
__global__ __launch_bounds__(256) void tap_gather_bwd_pow2_kernel(const float4* __restrict__ gz, float4* __restrict__ dG,
                                                                  int CG, int h, int w, int64_t total, int xcd,
                                                                  Divs3 dv) {
  constexpr int T = 2 * S, TW = T + 2;
  const int H = h * S, W = w * S;
  const IndexRange rg = xcd_range(total, xcd);
  const bool fast = total < kFastIndexLimit;
  for (int64_t i = rg.begin; i < rg.end; i += rg.stride) {
    const Index4 ix = split_index(i, dv, fast);  // (cg, xq, yq, b)
    const int cg = ix.c0, xq = ix.c1, yq = ix.c2;
    const int b = (int)ix.c3;
    const bool eL = xq == 0, eR = xq == w - 1, eT = yq == 0, eB = yq == h - 1;
    const int Q0 = S * xq - S / 2 - 1, R0 = S * yq - S / 2 - 1;  // window + ring origin
    float wxe[T];
#pragma unroll
    for (int t = 0; t < T; ++t) wxe[t] = pow2_tap_weight<S>(t, eL, eR);
    const float4* gb = gz + ((int64_t)b * H * W + Q0) * CG + cg;
    float4 acc[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int bq = 0; bq < 3; ++bq) acc[a][bq] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
    for (int u = 0; u < TW; ++u) {
      const int R = R0 + u;
      if (R < 0 || R >= H) continue;
      // tap a reads gz row R as sample row P = R + a - 1, window position t = u + a - 2
      const float wy0 = pow2_tap_weight<S>(u - 2, eT, eB), wy1 = pow2_tap_weight<S>(u - 1, eT, eB),
                  wy2 = pow2_tap_weight<S>(u, eT, eB);
      const float4* row = gb + (int64_t)R * W * CG;
      float4 g[TW];
#pragma unroll
      for (int v = 0; v < TW; ++v) {
        const int Q = Q0 + v;
        g[v] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (Q >= 0 && Q < W) g[v] = row[(int64_t)v * CG];
      }
      float4 rb[3];
#pragma unroll
      for (int bq = 0; bq < 3; ++bq) {
        rb[bq] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int t = 0; t < T; ++t) {  // sample column Q' = window position t reads gz column v = t + 2 - bq
          const int v = t + 2 - bq;
          rb[bq].x = fmaf(wxe[t], g[v].x, rb[bq].x);
          rb[bq].y = fmaf(wxe[t], g[v].y, rb[bq].y);
          rb[bq].z = fmaf(wxe[t], g[v].z, rb[bq].z);
          rb[bq].w = fmaf(wxe[t], g[v].w, rb[bq].w);
        }
      }
#pragma unroll
      for (int bq = 0; bq < 3; ++bq) {
        acc[0][bq].x = fmaf(wy0, rb[bq].x, acc[0][bq].x);
        acc[0][bq].y = fmaf(wy0, rb[bq].y, acc[0][bq].y);
        acc[0][bq].z = fmaf(wy0, rb[bq].z, acc[0][bq].z);
        acc[0][bq].w = fmaf(wy0, rb[bq].w, acc[0][bq].w);
        acc[1][bq].x = fmaf(wy1, rb[bq].x, acc[1][bq].x);
        acc[1][bq].y = fmaf(wy1, rb[bq].y, acc[1][bq].y);
        acc[1][bq].z = fmaf(wy1, rb[bq].z, acc[1][bq].z);
        acc[1][bq].w = fmaf(wy1, rb[bq].w, acc[1][bq].w);
        acc[2][bq].x = fmaf(wy2, rb[bq].x, acc[2][bq].x);
        acc[2][bq].y = fmaf(wy2, rb[bq].y, acc[2][bq].y);
        acc[2][bq].z = fmaf(wy2, rb[bq].z, acc[2][bq].z);
        acc[2][bq].w = fmaf(wy2, rb[bq].w, acc[2][bq].w);
      }
    }
    float4* out = dG + (((int64_t)b * h + yq) * w + xq) * 9 * CG + cg;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int bq = 0; bq < 3; ++bq) out[(a * 3 + bq) * CG] = acc[a][bq];
  }
}

// out = gate > 0 ? g * scale[c] : 0   (backward of y = relu(scale * z + shift) w.r.t. z, NHWC dense)
__global__ __launch_bounds__(256) void gate_scale_kernel(const float4* __restrict__ g, const float4* __restrict__ gate,
                                                         const float4* __restrict__ scale, float4* __restrict__ out, int CG,
                                                         int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 s = scale[i % CG], gv = g[i], t = gate[i];
    out[i] = make_float4(t.x > 0.f ? gv.x * s.x : 0.f, t.y > 0.f ? gv.y * s.y : 0.f, t.z > 0.f ? gv.z * s.z : 0.f,
                         t.w > 0.f ? gv.w * s.w : 0.f);
  }
}

}  // namespace sea

using namespace sea;

// The two tap-gather entries choose by the same rule as M2's: pointers, query, plan (upsample_plan.h), launch.
// G (B,h,w,9,C) coarse per-tap maps -> extra (B,H,W,C) (+)= sum over the 3x3 taps of the shifted up-samplings
// inner: 0 switches the compile-time-weight path of interior blocks off (A/B; the shipped value is 1)
extern "C" int sea_tap_gather_fwd(const float* G, float* extra, int accumulate, int B, int C, int h, int w, int H, int W,
                                  int inner, void* stream) {
  SEA_CHECK_ARG(G && extra);
  UpsamplePlan pl;
  SEA_CHECK_ARG(upsample_plan(UpsampleQuery{SEA_UP_TAP_FWD, B, C, h, w, H, W, 0, (uintptr_t)G, (uintptr_t)extra,
                                            process_config().upsample_general != 0, process_config().xcd_order}, &pl) == 0);
  dispatch_s<0, 4, 8>(pl.S, [&](auto S) {
    launch_planned(tap_gather_fwd_kernel<decltype(S)::value>, pl, 1, stream, (const float4*)G, (float4*)extra, accumulate, C / 4,
                   h, w, H, W, (float)h / (float)H, (float)w / (float)W, pl.nbh, pl.nbw, pl.total, pl.xo,
                   divs3(C / 4, pl.nbw, pl.nbh), inner ? 1 : 0);
  });
  SEA_RETURN_LAST();
}

// gz (B,H,W,C) gradient at the convolution output -> dG (B,h,w,9,C)
extern "C" int sea_tap_gather_bwd(const float* gz, float* dG, int B, int C, int h, int w, int H, int W, void* stream) {
  SEA_CHECK_ARG(gz && dG);
  UpsamplePlan pl;
  SEA_CHECK_ARG(upsample_plan(UpsampleQuery{SEA_UP_TAP_BWD, B, C, h, w, H, W, 0, (uintptr_t)gz, (uintptr_t)dG,
                                            process_config().upsample_general != 0, process_config().xcd_order}, &pl) == 0);
  if (pl.kernel == UPK_TAP_BWD_POW2)
    dispatch_s<4, 8>(pl.S, [&](auto S) {
      launch_planned(tap_gather_bwd_pow2_kernel<decltype(S)::value>, pl, 1, stream, (const float4*)gz, (float4*)dG, C / 4, h, w,
                     pl.total, pl.xo, divs3(C / 4, w, h));
    });
  else
    launch_planned(tap_gather_bwd_kernel, pl, 1, stream, (const float4*)gz, (float4*)dG, C / 4, h, w, H, W, (float)h / (float)H,
                   (float)w / (float)W, pl.total, pl.xo, divs3(C / 4, w, h));
  SEA_RETURN_LAST();
}

extern "C" int sea_gate_scale(const float* g, const float* gate, const float* scale, float* out, int64_t pixels, int C,
                              void* stream) {
  SEA_CHECK_ARG(g && gate && scale && out && pixels > 0 && C > 0 && (C % 4) == 0);
  SEA_CHECK_ARG(((((uintptr_t)g) | ((uintptr_t)gate) | ((uintptr_t)scale) | ((uintptr_t)out)) & 15) == 0);
  const int64_t total = pixels * (C / 4);
  hipLaunchKernelGGL(gate_scale_kernel, dim3(grid_for(total, 256 * 2)), dim3(256), 0, (hipStream_t)stream,
                     (const float4*)g, (const float4*)gate, (const float4*)scale, (float4*)out, C / 4, total);
  SEA_RETURN_LAST();
}
