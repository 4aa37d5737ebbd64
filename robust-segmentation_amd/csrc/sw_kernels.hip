// Sliding-window evaluation (semseg.utils.segmenter_eval, reference semseg/utils/segmenter_eval.py:51-92): the merge of
// the window logits and the final resize + softmax, as gathers.
//
// K11a  merge: the reference adds every window's (C, ws, ws) logits into a zero (C, H, W) sum at its anchor, counts the
//      covering windows, divides, resizes to the original size and takes softmax_C.  Here every merged pixel gathers
//      instead: the windows that cover a coordinate are a contiguous range of the ascending anchor list (anchors are at
//      most ws apart), found per axis from the list's first step plus a fix-up walk (one or no iteration for the
//      reference's lists, correct for any list the entry accepts).  sum = sequential fp32 adds from 0.f in the
//      reference's order (ha outer, wa inner), avg = sum / (float)count: the same correctly rounded operations in the
//      same order, built with -ffp-contract=off, so the averaged logits are the reference's bits.
//      Full-res mode: logits = model(window), (B*n_win, C, ws, ws).  Low-res mode: logits = forward_lowres(window),
//      (B*n_win, C, hl, wl); the model's own final up-sampling (align_corners=False, csrc/bilinear_map.h = M2) is
//      evaluated at the window-local coordinate (y - ha, x - wa) with M2's rounding (sw_lerp_m2 below), 4 taps per
//      covering window.  The (B*n_win, C, ws, ws) window logits never exist.
//      Epilogue (i): out = avg.  Epilogue (ii): out (+)= softmax_C(avg), the column mirrored when flip (output column x
//      takes merged column W-1-x); the averaged logits are never written.
//      Bytes: full-res mode reads B*n_win*C*ws^2*4 (every window value once), low-res mode r^2 times less; both write
//      B*C*H*W*4 once (epilogue ii with accumulate also reads it once).
//
// K11b  finish: score (+)= softmax_C(flip?(F.interpolate(avg, (Ho, Wo), "bilinear", align_corners=False))) for an
//      original size that differs from the merged one; axis_map_u with r = in/out is ATen's rule up and down.
//
// K11c / K11c' / K11a'  the window cut, its adjoint and the adjoint of the merge, for attacks through the windows
//      (semseg.utils.segmenter_eval.SlidingWindowModel): described at their kernels below.
//
// Work split of both = K10b (msf_kernels.hip): a block owns consecutive pixels of one image, pixel = lane;
//        C <= 32 : 128 pixels per block, 2 lane groups take the even / odd classes (16 in registers each);
//        C <= 192:  64 pixels per block, 4 lane groups take classes q, q+4, ... (at most 48 each).
//      Max and sum are combined across the groups through LDS in a fixed order; one lane reads and writes each output
//      element: no atomics, bitwise reproducible.
#include <math.h>

#include "sea_common.h"
#include "bilinear_map.h"

namespace sea {

// the anchor lists travel by value in the kernel arguments: no device allocation, nothing to free
struct SwAnchors {
  int h[SEA_SW_MAX_ANCHORS];
  int w[SEA_SW_MAX_ANCHORS];
  int n_h, n_w;
};

// [lo, hi]: the anchors a with a <= p < a + ws.  a[] ascends strictly from 0, consecutive anchors are at most ws apart and
// the last one covers the end of the axis (checked by the entry), so hi = the last anchor <= p always covers p.
// `step` = a[1] - a[0] (1 for a single anchor): the reference's lists are k*stride except the last entry, so p / step
// is hi itself or one past it.
__device__ __forceinline__ void sw_cover(const int* a, int n, int step, int ws, int p, int& lo, int& hi) {
  int j = p / step;
  if (j > n - 1) j = n - 1;
  while (j + 1 < n && a[j + 1] <= p) ++j;
  while (j > 0 && a[j] > p) --j;
  hi = j;
  while (j > 0 && a[j - 1] + ws > p) --j;
  lo = j;
}

// M2 as sea_upsample_bilinear_fwd rounds it.  That unit is built with contraction on: the source coordinate is ONE
// fma, r*(dst+0.5) - 0.5, and in (1-ly)*((1-lx)*v00 + lx*v01) + ly*((1-lx)*v10 + lx*v11) the FIRST product of every sum is
// fused into the add while the second is rounded on its own.  Explicit fmaf here, since this unit is built with
// -ffp-contract=off.  (For power-of-two factors every intermediate of the map is exact either way.)
__device__ __forceinline__ AxisMapU sw_axis_map_m2(int dst, float r, int n_in) {
  float src = fmaf(r, (float)dst + 0.5f, -0.5f);
  src = src < 0.f ? 0.f : src;
  AxisMapU m;
  m.i0 = (int)src;
  if (m.i0 > n_in - 1) m.i0 = n_in - 1;
  m.i1 = m.i0 + ((m.i0 < n_in - 1) ? 1 : 0);
  m.lam = src - (float)m.i0;
  return m;
}

__device__ __forceinline__ float sw_lerp_m2(float v00, float v01, float v10, float v11, float lx, float ly) {
  const float top = fmaf(1.f - lx, v00, lx * v01);
  const float bot = fmaf(1.f - lx, v10, lx * v11);
  return fmaf(1.f - ly, top, ly * bot);
}

// ATen's align_corners=False interpolation, every product and sum rounded on its own
__device__ __forceinline__ float sw_lerp(float v00, float v01, float v10, float v11, float lx, float ly) {
  const float top = (1.f - lx) * v00 + lx * v01;
  const float bot = (1.f - lx) * v10 + lx * v11;
  return (1.f - ly) * top + ly * bot;
}

// softmax over the classes of one pixel, spread over NQ lane groups (v[k] = class q + NQ*k), written or added to
// o[c * HW].  Called by every thread of the block (two barriers); `valid` lanes own a pixel.
template <int NQ, int CPT>
__device__ __forceinline__ void sw_softmax_store(float (&v)[CPT], bool valid, int q, int lane, int C, float* o, int HW,
                                                 int accumulate, float (*red_m)[256 / NQ], float (*red_s)[256 / NQ]) {
  float m = -INFINITY;
  if (valid) {
#pragma unroll
    for (int k = 0; k < CPT; ++k)
      if (q + NQ * k < C) m = fmaxf(m, v[k]);
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
  if (!valid) return;
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    const int c = q + NQ * k;
    if (c < C) {
      float* p = o + (int64_t)c * HW;
      const float r = v[k] / s;
      *p = accumulate ? *p + r : r;
    }
  }
}

// ---- K11a ----------------------------------------------------------------------------------------------------------
// grid = (ceil(H*W / PIX), B); block 256 = NQ groups of PIX = 256/NQ lanes
template <int NQ, int CPT, bool LOWRES>
__global__ __launch_bounds__(256) void sw_merge_kernel(const float* __restrict__ logits, float* __restrict__ out,
                                                       const SwAnchors an, int C, int hl, int wl, int ws, int H, int W,
                                                       int flip, int softmax, int accumulate) {
  constexpr int PIX = 256 / NQ;
  __shared__ float red_m[NQ][PIX], red_s[NQ][PIX];
  __shared__ int a_h[SEA_SW_MAX_ANCHORS], a_w[SEA_SW_MAX_ANCHORS];
  if (threadIdx.x < SEA_SW_MAX_ANCHORS)
    a_h[threadIdx.x] = an.h[threadIdx.x];
  else if (threadIdx.x < 2 * SEA_SW_MAX_ANCHORS)
    a_w[threadIdx.x - SEA_SW_MAX_ANCHORS] = an.w[threadIdx.x - SEA_SW_MAX_ANCHORS];
  __syncthreads();
  const int lane = threadIdx.x % PIX, q = threadIdx.x / PIX;
  const int b = blockIdx.y;
  const int HW = H * W;
  const int pix = blockIdx.x * PIX + lane;
  const bool valid = pix < HW;
  const int n_h = an.n_h, n_w = an.n_w;
  const int64_t lplane = (int64_t)hl * wl;                       // full-res mode: hl == wl == ws
  float v[CPT];
#pragma unroll
  for (int k = 0; k < CPT; ++k) v[k] = 0.f;
  if (valid) {
    const int y = pix / W, xo = pix % W;
    const int x = flip ? W - 1 - xo : xo;                        // the merged column this output column takes
    int h_lo, h_hi, w_lo, w_hi;
    sw_cover(a_h, n_h, n_h > 1 ? a_h[1] - a_h[0] : 1, ws, y, h_lo, h_hi);
    sw_cover(a_w, n_w, n_w > 1 ? a_w[1] - a_w[0] : 1, ws, x, w_lo, w_hi);
    const float rh = (float)hl / (float)ws, rw = (float)wl / (float)ws;    // = sea_upsample_bilinear_fwd
    for (int ih = h_lo; ih <= h_hi; ++ih) {
      const int ly = y - a_h[ih];
      const AxisMapU my = sw_axis_map_m2(ly, rh, hl);
      for (int iw = w_lo; iw <= w_hi; ++iw) {
        const int lx = x - a_w[iw];
        const float* pc = logits + (((int64_t)b * n_h + ih) * n_w + iw) * C * lplane + q * lplane;
        if constexpr (LOWRES) {
          const AxisMapU mx = sw_axis_map_m2(lx, rw, wl);
          const int o00 = my.i0 * wl + mx.i0, o01 = my.i0 * wl + mx.i1;
          const int o10 = my.i1 * wl + mx.i0, o11 = my.i1 * wl + mx.i1;
#pragma unroll
          for (int k = 0; k < CPT; ++k, pc += NQ * lplane)
            if (q + NQ * k < C) v[k] = v[k] + sw_lerp_m2(pc[o00], pc[o01], pc[o10], pc[o11], mx.lam, my.lam);
        } else {
          const int o = ly * ws + lx;
#pragma unroll
          for (int k = 0; k < CPT; ++k, pc += NQ * lplane)
            if (q + NQ * k < C) v[k] = v[k] + pc[o];
        }
      }
    }
    const float count = (float)((h_hi - h_lo + 1) * (w_hi - w_lo + 1));
#pragma unroll
    for (int k = 0; k < CPT; ++k) v[k] = v[k] / count;
  }
  float* ob = out + (int64_t)b * C * HW + pix;
  if (!softmax) {                                                // block-uniform: no lane skips a barrier
    if (!valid) return;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      const int c = q + NQ * k;
      if (c < C) ob[(int64_t)c * HW] = v[k];
    }
    return;
  }
  sw_softmax_store<NQ, CPT>(v, valid, q, lane, C, ob, HW, accumulate, red_m, red_s);
}

// ---- K11b ----------------------------------------------------------------------------------------------------------
// grid = (ceil(Ho*Wo / PIX), B)
template <int NQ, int CPT>
__global__ __launch_bounds__(256) void sw_finish_kernel(const float* __restrict__ avg, float* __restrict__ score, int C,
                                                        int H, int W, int Ho, int Wo, int flip, int accumulate) {
  constexpr int PIX = 256 / NQ;
  __shared__ float red_m[NQ][PIX], red_s[NQ][PIX];
  const int lane = threadIdx.x % PIX, q = threadIdx.x / PIX;
  const int b = blockIdx.y;
  const int HWo = Ho * Wo;
  const int pix = blockIdx.x * PIX + lane;
  const bool valid = pix < HWo;
  const int64_t plane = (int64_t)H * W;
  float v[CPT];
#pragma unroll
  for (int k = 0; k < CPT; ++k) v[k] = 0.f;
  if (valid) {
    const int oy = pix / Wo, ox = pix % Wo;
    const AxisMapU my = axis_map_u(oy, (float)H / (float)Ho, H);
    const AxisMapU mx = axis_map_u(flip ? Wo - 1 - ox : ox, (float)W / (float)Wo, W);
    const int64_t o00 = (int64_t)my.i0 * W + mx.i0, o01 = (int64_t)my.i0 * W + mx.i1;
    const int64_t o10 = (int64_t)my.i1 * W + mx.i0, o11 = (int64_t)my.i1 * W + mx.i1;
    const float* pc = avg + ((int64_t)b * C + q) * plane;
#pragma unroll
    for (int k = 0; k < CPT; ++k, pc += NQ * plane)
      if (q + NQ * k < C) v[k] = sw_lerp(pc[o00], pc[o01], pc[o10], pc[o11], mx.lam, my.lam);
  }
  sw_softmax_store<NQ, CPT>(v, valid, q, lane, C, score + (int64_t)b * C * HWo + pix, HWo, accumulate, red_m, red_s);
}

// ==== the attack through the windows (SlidingWindowModel): the cut and the adjoints of cut and merge ==================
// All three are gathers with one lane per output element and a fixed summation order: no atomics, bitwise reproducible.

// stage the anchor lists in LDS (every thread of a 256-thread block calls this; one barrier)
__device__ __forceinline__ void sw_stage_anchors(const SwAnchors& an, int* a_h, int* a_w) {
  if (threadIdx.x < SEA_SW_MAX_ANCHORS)
    a_h[threadIdx.x] = an.h[threadIdx.x];
  else if (threadIdx.x < 2 * SEA_SW_MAX_ANCHORS)
    a_w[threadIdx.x - SEA_SW_MAX_ANCHORS] = an.w[threadIdx.x - SEA_SW_MAX_ANCHORS];
  __syncthreads();
}

// ---- K11c ----------------------------------------------------------------------------------------------------------
// window cut: crops[(b * n_win + ih * n_w + iw), c, i, j] = x[b, c, a_h[ih] + i, a_w[iw] + j], the torch.stack of slices
// of segmenter_eval.inference as one copy.  Bytes: reads x once per covering window, writes B*n_win*Cx*ws^2*4.
// grid-stride over the crop elements (consecutive lanes = consecutive columns of one window row)
__global__ __launch_bounds__(256) void sw_cut_kernel(const float* __restrict__ x, float* __restrict__ crops,
                                                     const SwAnchors an, int Cx, int ws, int H, int W, int64_t total) {
  __shared__ int a_h[SEA_SW_MAX_ANCHORS], a_w[SEA_SW_MAX_ANCHORS];
  sw_stage_anchors(an, a_h, a_w);
  const int n_w = an.n_w, n_win = an.n_h * an.n_w;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int j = (int)(e % ws);
    int64_t r = e / ws;
    const int i = (int)(r % ws);
    r /= ws;
    const int c = (int)(r % Cx);
    r /= Cx;
    const int k = (int)(r % n_win);
    const int64_t b = r / n_win;
    crops[e] = x[((b * Cx + c) * H + a_h[k / n_w] + i) * W + a_w[k % n_w] + j];
  }
}

// ---- K11c' ---------------------------------------------------------------------------------------------------------
// adjoint of the cut: dx[b, c, y, x] = the fp32 sum from 0.f of dcrops[b, k, c, y - ha, x - wa] over the windows that
// cover (y, x), ha outer, wa inner (sw_cover's [lo, hi] per axis).  Bytes: reads every crop gradient once, writes dx once.
__global__ __launch_bounds__(256) void sw_cut_bwd_kernel(const float* __restrict__ dcrops, float* __restrict__ dx,
                                                         const SwAnchors an, int Cx, int ws, int H, int W, int64_t total) {
  __shared__ int a_h[SEA_SW_MAX_ANCHORS], a_w[SEA_SW_MAX_ANCHORS];
  sw_stage_anchors(an, a_h, a_w);
  const int n_h = an.n_h, n_w = an.n_w;
  const int step_h = n_h > 1 ? a_h[1] - a_h[0] : 1, step_w = n_w > 1 ? a_w[1] - a_w[0] : 1;
  const int64_t wplane = (int64_t)ws * ws;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int xx = (int)(e % W);
    int64_t r = e / W;
    const int y = (int)(r % H);
    r /= H;
    const int c = (int)(r % Cx);
    const int64_t b = r / Cx;
    int h_lo, h_hi, w_lo, w_hi;
    sw_cover(a_h, n_h, step_h, ws, y, h_lo, h_hi);
    sw_cover(a_w, n_w, step_w, ws, xx, w_lo, w_hi);
    float s = 0.f;
    for (int ih = h_lo; ih <= h_hi; ++ih)
      for (int iw = w_lo; iw <= w_hi; ++iw)
        s = s + dcrops[(((b * n_h + ih) * n_w + iw) * Cx + c) * wplane + (int64_t)(y - a_h[ih]) * ws + (xx - a_w[iw])];
    dx[e] = s;
  }
}

// ---- K11a' ---------------------------------------------------------------------------------------------------------
// adjoint of the merge (epilogue i): g (B, C, H, W) -> dlogits (B*n_win, C, hl, wl).
//      Full-res mode (hl == wl == ws): dlogits[b, k, c, i, j] = g[b, c, ha + i, wa + j] / (float)count(ha + i, wa + j),
//      one correctly rounded division = autograd through the reference's logit / count.
//      Low-res mode: the adjoint of K11a's in-kernel M2 applied to g / count restricted to the window.  A low-res element
//      (i, j) gathers the window pixels whose taps touch it, rows [first(i-1), first(i+1)) x columns likewise, row-major:
//      a row's sum first (fma with the column weight, from 0.f, ascending column), then the rows (fma with the row weight,
//      ascending row), the separable order of M2's backward.  The weights are the forward's: sw_axis_map_m2's taps and
//      lambda, (1 - lam) on i0 and lam on i1 (both when they coincide at the clamped edge).  Neither g / count nor the
//      (B*n_win, C, ws, ws) gradient is written.
//      Bytes: reads g once per covering window (B*n_win*C*ws^2*4; low-res mode re-reads within a wave's cache lines, every
//      window pixel feeds at most 4 low-res elements); writes B*n_win*C*ws^2*4 in full-res mode, (ws/hl)^2 times less in
//      low-res mode.
//      Work split = K11a: a block owns consecutive elements of one window's (hl, wl) plane, element = lane, classes over
//      the lane groups (full-res mode: in registers as in K11a; low-res mode: see that kernel).
__device__ __forceinline__ int sw_first_dst_ge_m2(int t, float r, int n_in, int n_out) {
  if (t <= 0) return 0;
  if (t > n_in - 1) return n_out;
  int d = (int)ceilf(((float)t + 0.5f) / r - 0.5f);
  d = d < 0 ? 0 : (d > n_out ? n_out : d);
  while (d > 0 && sw_axis_map_m2(d - 1, r, n_in).i0 >= t) --d;
  while (d < n_out && sw_axis_map_m2(d, r, n_in).i0 < t) ++d;
  return d;
}

__device__ __forceinline__ float sw_coef_m2(int dst, int src, float r, int n_in) {
  const AxisMapU m = sw_axis_map_m2(dst, r, n_in);
  return ((m.i0 == src) ? (1.f - m.lam) : 0.f) + ((m.i1 == src) ? m.lam : 0.f);
}

// full-res mode.  grid = (ceil(ws*ws / PIX), B * n_win); block 256 = NQ class groups of PIX = 256/NQ lanes
template <int NQ, int CPT>
__global__ __launch_bounds__(256) void sw_merge_bwd_kernel(const float* __restrict__ g, float* __restrict__ dlogits,
                                                           const SwAnchors an, int C, int ws, int H, int W) {
  constexpr int PIX = 256 / NQ;
  __shared__ int a_h[SEA_SW_MAX_ANCHORS], a_w[SEA_SW_MAX_ANCHORS];
  sw_stage_anchors(an, a_h, a_w);
  const int lane = threadIdx.x % PIX, q = threadIdx.x / PIX;
  const int n_h = an.n_h, n_w = an.n_w;
  const int b = blockIdx.y / (n_h * n_w), k = blockIdx.y % (n_h * n_w);
  const int lplane = ws * ws;
  const int el = blockIdx.x * PIX + lane;
  if (el >= lplane) return;
  const int y = a_h[k / n_w] + el / ws, x = a_w[k % n_w] + el % ws;
  int lo, hi;
  sw_cover(a_h, n_h, n_h > 1 ? a_h[1] - a_h[0] : 1, ws, y, lo, hi);
  const int cnt = hi - lo + 1;
  sw_cover(a_w, n_w, n_w > 1 ? a_w[1] - a_w[0] : 1, ws, x, lo, hi);
  const float count = (float)(cnt * (hi - lo + 1));
  const int64_t HW = (int64_t)H * W;
  const float* gp = g + ((int64_t)b * C + q) * HW + (int64_t)y * W + x;
  float* o = dlogits + ((int64_t)blockIdx.y * C + q) * lplane + el;
#pragma unroll
  for (int kk = 0; kk < CPT; ++kk)
    if (q + NQ * kk < C) o[(int64_t)NQ * kk * lplane] = gp[(int64_t)NQ * kk * HW] / count;
}

// low-res mode.  grid = (ceil(hl*wl / 64), B * n_win); block 256 = 4 class groups of 64 lanes, lane = low-res element,
// group q takes the classes q, q + 4, ... one after the other, so that the taps of a lane (consecutive columns of a row)
// and of its neighbours stay in the L1 while they are read.  What a window column needs is computed once per block into a
// table in LDS: its covering count on the w axis, its left tap and lambda.  Entry X lives at X + (X >> pad_shift), with
// 2^pad_shift the up-sampling factor rounded down: lanes read columns one factor apart, the padding puts them on distinct
// banks.  Dynamic LDS = sw_bwd_low_lds_bytes(ws, pad_shift), at most 48 KB (checked by the entry).
struct SwColumn {
  int tap;             // i0 | (count on the w axis << 16)
  float lam;
};

static inline size_t sw_bwd_low_lds_bytes(int ws, int pad_shift) {
  return (size_t)2 * SEA_SW_MAX_ANCHORS * sizeof(int) + ((size_t)ws + (ws >> pad_shift) + 1) * sizeof(SwColumn);
}

__global__ __launch_bounds__(256) void sw_merge_bwd_low_kernel(const float* __restrict__ g, float* __restrict__ dlogits,
                                                               const SwAnchors an, int C, int hl, int wl, int ws, int H,
                                                               int W, int pad_shift) {
  extern __shared__ __attribute__((aligned(16))) int sw_lds[];
  int* a_h = sw_lds;
  int* a_w = sw_lds + SEA_SW_MAX_ANCHORS;
  SwColumn* col = reinterpret_cast<SwColumn*>(sw_lds + 2 * SEA_SW_MAX_ANCHORS);
  sw_stage_anchors(an, a_h, a_w);
  const int n_h = an.n_h, n_w = an.n_w;
  const int b = blockIdx.y / (n_h * n_w), k = blockIdx.y % (n_h * n_w);
  const int ha = a_h[k / n_w], wa = a_w[k % n_w];
  const int step_h = n_h > 1 ? a_h[1] - a_h[0] : 1, step_w = n_w > 1 ? a_w[1] - a_w[0] : 1;
  const float rh = (float)hl / (float)ws, rw = (float)wl / (float)ws;
  int lo, hi;
  for (int X = threadIdx.x; X < ws; X += 256) {
    sw_cover(a_w, n_w, step_w, ws, wa + X, lo, hi);
    const AxisMapU m = sw_axis_map_m2(X, rw, wl);
    SwColumn cx;
    cx.tap = m.i0 | ((hi - lo + 1) << 16);
    cx.lam = m.lam;
    col[X + (X >> pad_shift)] = cx;
  }
  __syncthreads();
  const int lane = threadIdx.x % 64, q = threadIdx.x / 64;
  const int lplane = hl * wl;
  const int el = blockIdx.x * 64 + lane;
  if (el >= lplane) return;
  const int i = el / wl, j = el % wl;
  const int Y0 = sw_first_dst_ge_m2(i - 1, rh, hl, ws), Y1 = sw_first_dst_ge_m2(i + 1, rh, hl, ws);
  const int X0 = sw_first_dst_ge_m2(j - 1, rw, wl, ws), X1 = sw_first_dst_ge_m2(j + 1, rw, wl, ws);
  const int64_t HW = (int64_t)H * W;
  for (int c = q; c < C; c += 4) {
    const float* gc = g + ((int64_t)b * C + c) * HW + (int64_t)ha * W + wa;
    float acc = 0.f;
    for (int Y = Y0; Y < Y1; ++Y) {
      const float wy = sw_coef_m2(Y, i, rh, hl);
      sw_cover(a_h, n_h, step_h, ws, ha + Y, lo, hi);
      const int cnt_y = hi - lo + 1;
      const float* gr = gc + (int64_t)Y * W;
      float row = 0.f;
      for (int X = X0; X < X1; ++X) {
        const SwColumn cx = col[X + (X >> pad_shift)];
        const int i0 = cx.tap & 0xffff;
        const int i1 = i0 + ((i0 < wl - 1) ? 1 : 0);
        const float wx = ((i0 == j) ? (1.f - cx.lam) : 0.f) + ((i1 == j) ? cx.lam : 0.f);
        const float count = (float)(cnt_y * (cx.tap >> 16));
        row = fmaf(wx, gr[X] / count, row);
      }
      acc = fmaf(wy, row, acc);
    }
    dlogits[((int64_t)blockIdx.y * C + c) * lplane + el] = acc;
  }
}

// one axis of the argument checks: 1 .. SEA_SW_MAX_ANCHORS anchors ascending strictly from 0 to n - ws, at most ws apart
static bool sw_axis_ok(const int* a, int n_a, int n, int ws) {
  if (!a || n_a < 1 || n_a > SEA_SW_MAX_ANCHORS || ws < 1 || ws > n) return false;
  if (a[0] != 0 || a[n_a - 1] != n - ws) return false;
  for (int i = 1; i < n_a; ++i)
    if (a[i] <= a[i - 1] || a[i] - a[i - 1] > ws || a[i] > n - ws) return false;
  return true;
}

}  // namespace sea

using namespace sea;

extern "C" int sea_sw_merge(const float* logits, float* out, int B, int C, int hl, int wl, int ws, const int* h_anchors,
                            int n_h, const int* w_anchors, int n_w, int H, int W, int flip, int softmax, int accumulate,
                            void* stream) {
  SEA_CHECK_ARG(logits && out && logits != out && B > 0 && C > 0 && C <= SEA_MSF_MAX_CLASSES && H > 0 && W > 0 &&
                (int64_t)H * W < (1ll << 31));
  SEA_CHECK_ARG(sw_axis_ok(h_anchors, n_h, H, ws) && sw_axis_ok(w_anchors, n_w, W, ws));
  SEA_CHECK_ARG(hl > 0 && wl > 0 && hl <= ws && wl <= ws && (int64_t)B * n_h * n_w <= 65535);
  SEA_CHECK_ARG(softmax || (!flip && !accumulate));     // the mirror and the sum belong to the step that writes scores
  SwAnchors an;
  for (int i = 0; i < SEA_SW_MAX_ANCHORS; ++i) {
    an.h[i] = i < n_h ? h_anchors[i] : 0;
    an.w[i] = i < n_w ? w_anchors[i] : 0;
  }
  an.n_h = n_h;
  an.n_w = n_w;
  const hipStream_t s = (hipStream_t)stream;
  const int HW = H * W, f = flip ? 1 : 0, sm = softmax ? 1 : 0, acc = accumulate ? 1 : 0;
  const bool full = hl == ws && wl == ws;
  if (C <= 32) {
    const dim3 grid((HW + 127) / 128, B);
    if (full)
      hipLaunchKernelGGL((sw_merge_kernel<2, 16, false>), grid, dim3(256), 0, s, logits, out, an, C, hl, wl, ws, H, W, f,
                         sm, acc);
    else
      hipLaunchKernelGGL((sw_merge_kernel<2, 16, true>), grid, dim3(256), 0, s, logits, out, an, C, hl, wl, ws, H, W, f,
                         sm, acc);
  } else {
    const dim3 grid((HW + 63) / 64, B);
    if (full)
      hipLaunchKernelGGL((sw_merge_kernel<4, 48, false>), grid, dim3(256), 0, s, logits, out, an, C, hl, wl, ws, H, W, f,
                         sm, acc);
    else
      hipLaunchKernelGGL((sw_merge_kernel<4, 48, true>), grid, dim3(256), 0, s, logits, out, an, C, hl, wl, ws, H, W, f,
                         sm, acc);
  }
  SEA_RETURN_LAST();
}

extern "C" int sea_sw_finish(const float* avg, float* score, int B, int C, int H, int W, int Ho, int Wo, int flip,
                             int accumulate, void* stream) {
  SEA_CHECK_ARG(avg && score && avg != score && B > 0 && B <= 65535 && C > 0 && C <= SEA_MSF_MAX_CLASSES && H > 0 &&
                W > 0 && Ho > 0 && Wo > 0 && (int64_t)H * W < (1ll << 31) && (int64_t)Ho * Wo < (1ll << 31));
  const hipStream_t s = (hipStream_t)stream;
  const int HWo = Ho * Wo, f = flip ? 1 : 0, acc = accumulate ? 1 : 0;
  if (C <= 32) {
    const dim3 grid((HWo + 127) / 128, B);
    hipLaunchKernelGGL((sw_finish_kernel<2, 16>), grid, dim3(256), 0, s, avg, score, C, H, W, Ho, Wo, f, acc);
  } else {
    const dim3 grid((HWo + 63) / 64, B);
    hipLaunchKernelGGL((sw_finish_kernel<4, 48>), grid, dim3(256), 0, s, avg, score, C, H, W, Ho, Wo, f, acc);
  }
  SEA_RETURN_LAST();
}

// the anchor lists of a call, checked, by value
static bool sw_make_anchors(SwAnchors& an, const int* h_anchors, int n_h, const int* w_anchors, int n_w, int H, int W,
                            int ws) {
  if (!(sw_axis_ok(h_anchors, n_h, H, ws) && sw_axis_ok(w_anchors, n_w, W, ws))) return false;
  for (int i = 0; i < SEA_SW_MAX_ANCHORS; ++i) {
    an.h[i] = i < n_h ? h_anchors[i] : 0;
    an.w[i] = i < n_w ? w_anchors[i] : 0;
  }
  an.n_h = n_h;
  an.n_w = n_w;
  return true;
}

static int sw_stride_grid(int64_t total) {
  const int64_t blocks = (total + 255) / 256;
  return (int)(blocks < 8192 ? blocks : 8192);
}

extern "C" int sea_sw_cut(const float* x, float* crops, int B, int Cx, int ws, const int* h_anchors, int n_h,
                          const int* w_anchors, int n_w, int H, int W, void* stream) {
  SEA_CHECK_ARG(x && crops && x != crops && B > 0 && Cx > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31));
  SwAnchors an;
  SEA_CHECK_ARG(sw_make_anchors(an, h_anchors, n_h, w_anchors, n_w, H, W, ws));
  SEA_CHECK_ARG((int64_t)B * n_h * n_w <= 65535);
  const int64_t total = (int64_t)B * n_h * n_w * Cx * ws * ws;
  hipLaunchKernelGGL(sw_cut_kernel, dim3(sw_stride_grid(total)), dim3(256), 0, (hipStream_t)stream, x, crops, an, Cx, ws,
                     H, W, total);
  SEA_RETURN_LAST();
}

extern "C" int sea_sw_cut_bwd(const float* dcrops, float* dx, int B, int Cx, int ws, const int* h_anchors, int n_h,
                              const int* w_anchors, int n_w, int H, int W, void* stream) {
  SEA_CHECK_ARG(dcrops && dx && dcrops != dx && B > 0 && Cx > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31));
  SwAnchors an;
  SEA_CHECK_ARG(sw_make_anchors(an, h_anchors, n_h, w_anchors, n_w, H, W, ws));
  SEA_CHECK_ARG((int64_t)B * n_h * n_w <= 65535);
  const int64_t total = (int64_t)B * Cx * H * W;
  hipLaunchKernelGGL(sw_cut_bwd_kernel, dim3(sw_stride_grid(total)), dim3(256), 0, (hipStream_t)stream, dcrops, dx, an,
                     Cx, ws, H, W, total);
  SEA_RETURN_LAST();
}

extern "C" int sea_sw_merge_bwd(const float* g, float* dlogits, int B, int C, int hl, int wl, int ws, const int* h_anchors,
                                int n_h, const int* w_anchors, int n_w, int H, int W, void* stream) {
  SEA_CHECK_ARG(g && dlogits && g != dlogits && B > 0 && C > 0 && C <= SEA_MSF_MAX_CLASSES && H > 0 && W > 0 &&
                (int64_t)H * W < (1ll << 31));
  SwAnchors an;
  SEA_CHECK_ARG(sw_make_anchors(an, h_anchors, n_h, w_anchors, n_w, H, W, ws));
  SEA_CHECK_ARG(hl > 0 && wl > 0 && hl <= ws && wl <= ws && (int64_t)B * n_h * n_w <= 65535);
  const hipStream_t s = (hipStream_t)stream;
  const int n_win = B * n_h * n_w;
  if (hl == ws && wl == ws) {
    if (C <= 32)
      hipLaunchKernelGGL((sw_merge_bwd_kernel<2, 16>), dim3((ws * ws + 127) / 128, n_win), dim3(256), 0, s, g, dlogits, an, C,
                         ws, H, W);
    else
      hipLaunchKernelGGL((sw_merge_bwd_kernel<4, 48>), dim3((ws * ws + 63) / 64, n_win), dim3(256), 0, s, g, dlogits, an, C,
                         ws, H, W);
  } else {
    int pad_shift = 0;
    while ((2 << pad_shift) <= ws / wl) ++pad_shift;     // 2^pad_shift <= ws / wl < 2^(pad_shift + 1)
    const size_t lds = sw_bwd_low_lds_bytes(ws, pad_shift);
    SEA_CHECK_ARG(ws < 65536 && lds <= 48 * 1024);       // the column table: ws <= 3000 at x2 and above
    hipLaunchKernelGGL(sw_merge_bwd_low_kernel, dim3((hl * wl + 63) / 64, n_win), dim3(256), lds, s, g, dlogits, an, C, hl,
                       wl, ws, H, W, pad_shift);
  }
  SEA_RETURN_LAST();
}
