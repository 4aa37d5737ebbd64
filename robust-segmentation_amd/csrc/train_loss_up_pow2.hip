// T2u for power-of-two ratios: CrossEntropyLoss(weight, ignore_index, reduction="mean") on
// F.interpolate(low, (H, W), mode="bilinear", align_corners=False), forward AND gradient in one pass, for H = r h,
// W = r w with r = 4 (UperNet's main head, uperforseg.py:416-418) or r = 16 (UperNet's auxiliary head,
// uperforseg.py:432-434; Segmenter, segmenter.py:228).
//
// The gather kernels of train_loss_up.hip need two launches because the backward's normalisation is known only after the
// whole forward, and they interpolate and exponentiate every (pixel, class) three times or more.  With mean reduction the
// gradient is g * (1 / sum w[y]) * raw, where raw[b,c,i,j] = sum over the valid pixels whose footprint touches (i, j) of
// (bilinear weight) * w[y] * (softmax(z)_c - [c == y]) does not depend on the two scalars: the forward can write raw (at LOW
// resolution, in double: see below) and the backward is one scale pass.  OHEM cannot do this (its selection needs every pixel's loss before any gradient) and keeps
// the gather kernels.
//
// The main kernel is K2u's power-of-two kernel (loss_upsampled.hip) with T2's criterion in it:
//   * lanes = CLASSES (c = lane + 64 slot, up to three slots); a lane keeps its classes' four corner logits of a CELL (the
//     S x S pixels that interpolate between the same four low-resolution pixels) in registers;
//   * a wave walks a SEGMENT of one cell row left to right (8 cells at x4, 2 at x16), carrying the shared corners and their
//     accumulators; per pixel it interpolates (ATen's expression tree, lerp2; the source cell and lambda of a pixel are
//     integer arithmetic and exact in fp32 for these ratios, as axis_map_p2 in bilinear_map.h), takes max and sum over the
//     classes by one wave reduction each, and scatters d z_c = w[y] (e_c / sum - [c == y]) into the four corner accumulators
//     with the four bilinear weights: every exponential is computed once;
//   * a pixel that is ignored or out of range costs one scalar compare: it skips everything;
//   * the loss terms of a group of 16 pixels are finished in one pass with lanes = pixels;
//   * top / bottom partial vectors are flushed per low-resolution column of a cell row; a second kernel adds the (at most
//     eight) partials of a low-resolution pixel in a fixed order and transposes to NCHW through LDS.  No float atomics,
//     one wave per (image, cell row, segment): the bits of raw[b] depend on image b alone.
//   * one TrainRecord per wave; train_reduce_k (train_loss_common.h) sums them in double in a fixed order into T2's words.
// No LDS and no barrier in the main kernel.
//
// Arithmetic, chosen so that T2's accuracy rule (error against float64 at most twice the unfused device path's, or the
// fp32 floor) holds with margin rather than for speed:
//   * accurate expf, as T2 / T2u (the hardware exponential's argument scaling costs |x| 2^-24 relative, several ulps in
//     the tail classes whose sum matters at C = 151);
//   * the class sum is a float tree over at most 192 non-negative terms (three per lane, DPP rows of 16, four rows):
//     at most nine roundings, every term <= 1, no cancellation; T2's double sum would double the reduction's cost for a
//     relative 5e-7 at worst that the per-pixel rounding of the loss to float already has;
//   * the per-pixel loss is T2's: (float)(log((double)sum) - ((double)z_y - (double)max)), once per pixel, lanes = pixels;
//   * the corner accumulators are DOUBLE: a low-resolution element collects up to 4 S^2 = 1024 signed terms at x16 whose sum
//     cancels (sum_c (p_c - [c == y]) = 0), the one place where fp32 accumulation would cost more than an ulp of the largest
//     element.  The bilinear weights are multiples of 1/1024, so each product is exact in double.  The per-pixel term
//     d z_c = K e_c / sum - K [c == y] is formed in double too (1 / sum: the float quotient plus one Newton step);
//   * the partial vectors, the combine kernel's sum (at most eight terms) and raw itself are DOUBLE, and the scale pass
//     multiplies in double by g / sum w[y] (the words' double sum, not their float coef): the gradient is rounded to float
//     ONCE.  A float raw costs a second rounding, and half an ulp of raw is up to a whole ulp of the product when raw sits
//     low in its binade and the product high in its own: 1.5 ulp at worst against the rule's floor of 1.  Measured with
//     float partials and float raw: 1.5 ulp of the largest element (C = 65, x4); with double partials and float raw: 1.02
//     ulp (C = 21, one row), where the unfused path has 0.4.  The price is 8 instead of 4 bytes per element of raw between
//     forward and backward: 10 MB at x16 and 158 MB at x4 for B = 8, C = 151, 512 x 512, where the full-resolution logits
//     alone are 1.27 GB.
#include "bilinear_map.h"
#include "train_loss_common.h"

namespace sea {

constexpr int kUp2MinClasses = 2, kUp2MaxClasses = 192;

__device__ __forceinline__ float up2_lerp2(float v00, float v01, float v10, float v11, float lx, float ly) {
  const float top = (1.f - lx) * v00 + lx * v01;
  const float bot = (1.f - lx) * v10 + lx * v11;
  return (1.f - ly) * top + ly * bot;
}

// wave reductions that leave ONE value for the whole wave in a fixed order (K2u's: DPP within rows of 16 lanes, the four
// rows added as scalars)
#define SEA_UP2_DPP(v, ctrl) \
  __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xF, 0xF, true))
__device__ __forceinline__ float up2_lane(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ float up2_wave_max(float v) {
  v = fmaxf(v, SEA_UP2_DPP(v, 0xB1));   // quad_perm [1,0,3,2]
  v = fmaxf(v, SEA_UP2_DPP(v, 0x4E));   // quad_perm [2,3,0,1]
  v = fmaxf(v, SEA_UP2_DPP(v, 0x141));  // row_half_mirror
  v = fmaxf(v, SEA_UP2_DPP(v, 0x140));  // row_mirror
  return fmaxf(fmaxf(up2_lane(v, 0), up2_lane(v, 16)), fmaxf(up2_lane(v, 32), up2_lane(v, 48)));
}
__device__ __forceinline__ float up2_wave_sum(float v) {
  v += SEA_UP2_DPP(v, 0xB1);
  v += SEA_UP2_DPP(v, 0x4E);
  v += SEA_UP2_DPP(v, 0x141);
  v += SEA_UP2_DPP(v, 0x140);
  return (up2_lane(v, 0) + up2_lane(v, 16)) + (up2_lane(v, 32) + up2_lane(v, 48));
}
#undef SEA_UP2_DPP

constexpr int up2_seg_cells(int S) { return S == 4 ? 8 : 2; }  // cells per wave (a segment of a cell row)
constexpr int kUp2CombineCols = 16;  // low-resolution columns per block of the combine kernel: 26 KB of LDS at C = 192

struct Up2Args {
  const float* low;
  const long long* y;
  const float* w;
  long long ignore;
  double* main_part;  // [B][2 roles][h + 1][wl][C]
  double* lead_part;  // [B][2 roles][h + 1][nseg][C]
  TrainRecord* rec;  // one record per wave: [B][h + 1][nseg]
  TrainWords* words;
  int C, h, wl, nseg, B;
};

template <int S, int NS>
__global__ __launch_bounds__(256) void train_ce_up_pow2_k(const Up2Args p) {
  constexpr int SEGC = up2_seg_cells(S);
  const int lane = threadIdx.x & 63;
  const int C = p.C, h = p.h, wl = p.wl, H = h * S, W = wl * S;
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // one wave = one (image, cell row, segment)
  const int per_img = (h + 1) * p.nseg;
  if (wid >= (int64_t)p.B * per_img) return;
  const int b = (int)(wid / per_img), rem = (int)(wid - (int64_t)b * per_img);
  const int ci_idx = rem / p.nseg, seg = rem - ci_idx * p.nseg;
  const int ci = ci_idx - 1;  // cell row: source rows (ci, ci + 1), clamped into the map
  const int r0 = ci < 0 ? 0 : ci, r1 = ci + 1 > h - 1 ? h - 1 : ci + 1;
  const int py_lo = ci < 0 ? S / 2 : 0, py_hi = ci == h - 1 ? S / 2 : S;
  const int cj_a = seg * SEGC - 1;
  int cj_b = cj_a + SEGC;
  cj_b = cj_b > wl ? wl : cj_b;  // cells cj_a .. cj_b - 1 of [-1, wl - 1]

  bool cv[NS];
  const float* pl0[NS];
  const float* pl1[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int c = lane + 64 * s;
    cv[s] = c < C;
    const int cc = cv[s] ? c : C - 1;
    pl0[s] = p.low + (((int64_t)b * C + cc) * h + r0) * wl;
    pl1[s] = p.low + (((int64_t)b * C + cc) * h + r1) * wl;
  }
  float v00[NS], v10[NS], v01[NS], v11[NS], n01[NS], n11[NS];
  double accT[NS], accB[NS];
  {
    const int c0 = cj_a < 0 ? 0 : cj_a;
    const int c1 = cj_a + 1 > wl - 1 ? wl - 1 : cj_a + 1;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      v00[s] = pl0[s][c0];
      v10[s] = pl1[s][c0];
      n01[s] = pl0[s][c1];  // (the right corners of the NEXT cell are fetched while this cell is computed)
      n11[s] = pl1[s][c1];
      accT[s] = 0.0;
      accB[s] = 0.0;
    }
  }
  const int64_t row_part = (int64_t)b * 2 * (h + 1) + ci_idx;  // role 0 (top); role 1 (bottom) is h + 1 rows further
  double* const mainT = p.main_part + row_part * wl * C;
  double* const mainB = p.main_part + (row_part + (h + 1)) * wl * C;
  double* const leadT = p.lead_part + (row_part * p.nseg + seg) * C;
  double* const leadB = p.lead_part + ((row_part + (h + 1)) * p.nseg + seg) * C;
  bool leading = true;  // the next flush is the segment's first column
  auto flush = [&](int col) __attribute__((always_inline)) {
    double* const t = leading ? leadT : mainT + (int64_t)col * C;
    double* const bo = leading ? leadB : mainB + (int64_t)col * C;
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (cv[s]) {
        t[lane + 64 * s] = accT[s];
        bo[lane + 64 * s] = accB[s];
      }
    leading = false;
  };

  double lsum = 0.0, wsum = 0.0;  // lanes 0-15: the sums of "their" pixels of every group
  int nvalid = 0;
  bool anybad = false;
  for (int cj = cj_a; cj < cj_b; ++cj) {
    const int c0 = cj < 0 ? 0 : cj, c1 = cj + 1 > wl - 1 ? wl - 1 : cj + 1;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      v01[s] = n01[s];
      v11[s] = n11[s];
    }
    if (cj + 1 < cj_b) {
      const int c2 = cj + 2 > wl - 1 ? wl - 1 : cj + 2;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        n01[s] = pl0[s][c2];
        n11[s] = pl1[s][c2];
      }
    }
    const int px_lo = cj < 0 ? S / 2 : 0, px_hi = cj == wl - 1 ? S / 2 : S;
    const int X0 = S * cj + S / 2;  // X = X0 + px, Y = Y0 + py
    const int Y0 = S * ci + S / 2;
    double nT[NS], nB[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      nT[s] = 0.0;
      nB[s] = 0.0;
    }
    // A GROUP of 4 x 4 pixels at (by, bx) of the cell (x4: the cell), lane q = (py & 3) * 4 + (px & 3) holds pixel q's label:
    //   1  per valid pixel (lanes = classes): logits, max, exponentials, sum, z_y; the gradient is scattered at once; the
    //      three statistics go into LANE q of three registers;
    //   2  once per group (lanes = pixels): the loss terms in double.
    auto group = [&](int by, int bx) __attribute__((always_inline)) {
      const int lpy = by + (lane >> 2), lpx = bx + (lane & 3);
      const bool in = lane < 16 && lpy >= py_lo && lpy < py_hi && lpx >= px_lo && lpx < px_hi;
      int labv = -1;
      if (in) {
        bool counted, bad;
        labv = train_label(p.y[((int64_t)b * H + (Y0 + lpy)) * W + (X0 + lpx)], p.ignore, C, counted, bad);
        nvalid += counted ? 1 : 0;
        anybad = anybad || bad;
      }
      float Mv = 0.f, Sv = 1.f, Zv = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int lab = __builtin_amdgcn_readlane(labv, q);
        if (lab < 0) continue;  // (wave-uniform) outside the image's part of the cell, ignored or out of range
        const float lx = cj < 0 ? 0.f : ((float)(bx + (q & 3)) + 0.5f) * (1.f / (float)S);
        const float ly = ci < 0 ? 0.f : ((float)(by + (q >> 2)) + 0.5f) * (1.f / (float)S);
        float z[NS], e[NS];
        float mloc = -INFINITY;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          z[s] = up2_lerp2(v00[s], v01[s], v10[s], v11[s], lx, ly);
          if (!cv[s]) z[s] = -INFINITY;
          mloc = fmaxf(mloc, z[s]);
        }
        float m = up2_wave_max(mloc);
        m = (m == -INFINITY) ? -3.0e38f : m;  // T2: exp(-inf - -inf) must not become NaN
        float sloc = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          e[s] = expf(z[s] - m);  // exp(-inf) = 0 for the padding lanes
          sloc += e[s];
        }
        const float ssum = up2_wave_sum(sloc);
        float zy = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s)
          if ((lab >> 6) == s) zy = up2_lane(z[s], lab & 63);
        const bool mine = lane == q;
        Mv = mine ? m : Mv;
        Sv = mine ? ssum : Sv;
        Zv = mine ? zy : Zv;
        // the gradient of this pixel: a e_c, minus K at the label, in double
        const float K = (p.w != nullptr) ? p.w[lab] : 1.f;
        const float rf = 1.f / ssum;  // sum >= 1 (the maximum's own term) unless every logit is -inf
        double r = (double)rf;
        r = r * fma(-(double)ssum, r, 2.0);  // one Newton step: the float quotient's 2^-24 squared
        const double a = (double)K * r, Kd = (double)K;
        const double w00 = (double)((1.f - ly) * (1.f - lx)), w01 = (double)((1.f - ly) * lx);
        const double w10 = (double)(ly * (1.f - lx)), w11 = (double)(ly * lx);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          double dz = a * (double)e[s];
          if ((lab >> 6) == s && lane == (lab & 63)) dz -= Kd;
          accT[s] = fma(w00, dz, accT[s]);
          nT[s] = fma(w01, dz, nT[s]);
          accB[s] = fma(w10, dz, accB[s]);
          nB[s] = fma(w11, dz, nB[s]);
        }
        __builtin_amdgcn_sched_barrier(0);  // (pixels one after the other: interleaved they multiply the live registers)
      }
      if (labv >= 0) {
        // -log_softmax(z)[y] = log(sum exp(z - m)) - (z_y - m), rounded to float once (T2)
        const float ce = (float)(log((double)Sv) - ((double)Zv - (double)Mv));
        const float wy = (p.w != nullptr) ? p.w[labv] : 1.f;
        lsum += (double)(wy * ce);
        wsum += (double)wy;
      }
    };
    if constexpr (S == 4) {
      group(0, 0);
    } else {
#pragma clang loop unroll(disable)
      for (int g16 = 0; g16 < 16; ++g16) {
        const int by = 4 * (g16 >> 2), bx = 4 * (g16 & 3);
        if (by + 4 <= py_lo || by >= py_hi || bx + 4 <= px_lo || bx >= px_hi) continue;
        group(by, bx);
      }
    }
    if (c1 == c0) {  // a clamped border cell: both columns are the same low-resolution pixel
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        accT[s] += nT[s];
        accB[s] += nB[s];
      }
    } else {
      flush(c0);
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        accT[s] = nT[s];
        accB[s] = nB[s];
        v00[s] = v01[s];
        v10[s] = v11[s];
      }
    }
  }
  {
    const int last = cj_b - 1;
    flush(last + 1 > wl - 1 ? wl - 1 : last + 1);
  }
  if (anybad) p.words->err = 1;  // every writer stores the same value
  lsum = wave_sum_d(lsum);
  wsum = wave_sum_d(wsum);
  nvalid = wave_sum_i(nvalid);
  if (lane == 0) {
    TrainRecord r;
    r.loss = lsum;
    r.w = wsum;
    r.hard = 0.0;
    r.n_valid = nvalid;
    r.n_hard = 0;
    p.rec[wid] = r;
  }
}

// raw[b][c][i][j] = sum, in a fixed order, of the partial vectors that belong to low-resolution pixel (i, j):
//   top of cell row -1 (i = 0 only), bottom of cell row i - 1, top of cell row i, bottom of cell row h - 1 (i = h - 1 only);
//   each = the main partial of column j (j > 0) + the leading partial of the segment that starts at column j
template <int S>
__global__ __launch_bounds__(256) void train_ce_up_pow2_combine_k(const double* __restrict__ main_part,
                                                                  const double* __restrict__ lead_part, int C, int h,
                                                                  int wl, int nseg, double* __restrict__ raw) {
  constexpr int SEGC = up2_seg_cells(S);
  constexpr int TJ = kUp2CombineCols;
  extern __shared__ double tile[];  // [C][TJ + 1]
  const int jt = blockIdx.x * TJ, i = blockIdx.y, b = blockIdx.z;
  auto term = [&](int role, int ci_idx, int j, int c) -> double {
    const int64_t row = ((int64_t)b * 2 + role) * (h + 1) + ci_idx;
    double v = 0.0;
    if (j > 0) v = main_part[(row * wl + j) * C + c];
    // column j leads segment g when j == max(g SEGC - 1, 0)
    const int g = (j + 1) / SEGC;
    if (j == 0 || ((j + 1) % SEGC == 0 && g < nseg)) v += lead_part[(row * nseg + (j == 0 ? 0 : g)) * C + c];
    return v;
  };
  for (int idx = threadIdx.x; idx < TJ * C; idx += 256) {
    const int jl = idx / C, c = idx - jl * C, j = jt + jl;
    if (j >= wl) continue;
    double v = 0.0;
    if (i == 0) v += term(0, 0, j, c);      // top of cell row -1
    v += term(1, i, j, c);                  // bottom of cell row i - 1  (index i)
    v += term(0, i + 1, j, c);              // top of cell row i        (index i + 1)
    if (i == h - 1) v += term(1, h, j, c);  // bottom of cell row h - 1
    tile[c * (TJ + 1) + jl] = v;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < TJ * C; idx += 256) {
    const int c = idx / TJ, jl = idx - c * TJ, j = jt + jl;
    if (j < wl) raw[(((int64_t)b * C + c) * h + i) * wl + j] = tile[c * (TJ + 1) + jl];
  }
}

// dlow = (g / sum w[y]) * raw in double, rounded once.  An element whose raw is zero stays zero: with every
// label ignored the factor is g / 0.
__global__ __launch_bounds__(256) void train_ce_up_pow2_scale_k(const double* __restrict__ raw, const float* __restrict__ g,
                                                                const TrainWords* __restrict__ words,
                                                                float* __restrict__ dlow, int64_t n) {
  const double gc = (double)g[0] / words->sum_w;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double v = raw[i];
    dlow[i] = (v == 0.0) ? 0.f : (float)(gc * v);
  }
}

static int up2_scale(int C, int h, int wl, int H, int W) {
  if (C < kUp2MinClasses || C > kUp2MaxClasses || h < 1 || wl < 1) return 0;
  if (h > (1 << 20) || wl > (1 << 20)) return 0;
  if (H == 4 * h && W == 4 * wl) return 4;
  if (H == 16 * h && W == 16 * wl) return 16;
  return 0;
}
static int up2_nseg(int wl, int S) { return (wl + 1 + up2_seg_cells(S) - 1) / up2_seg_cells(S); }
// workspace: [wave records][main partials][leading partials]
static size_t up2_rec_bytes(int B, int h, int wl, int S) {
  return ((size_t)B * (h + 1) * up2_nseg(wl, S) * sizeof(TrainRecord) + 255) / 256 * 256;
}
static size_t up2_main_bytes(int B, int C, int h, int wl) { return ((size_t)B * 2 * (h + 1) * wl * C * 8 + 255) / 256 * 256; }
static size_t up2_lead_bytes(int B, int C, int h, int wl, int S) {
  return (size_t)B * 2 * (h + 1) * up2_nseg(wl, S) * C * 8;
}

template <int S, int NS>
static void up2_launch(const Up2Args& a, double* raw, hipStream_t s) {
  const int64_t waves = (int64_t)a.B * (a.h + 1) * a.nseg;
  hipLaunchKernelGGL((train_ce_up_pow2_k<S, NS>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, a);
  hipLaunchKernelGGL((train_ce_up_pow2_combine_k<S>), dim3((a.wl + kUp2CombineCols - 1) / kUp2CombineCols, a.h, a.B),
                     dim3(256), (size_t)a.C * (kUp2CombineCols + 1) * sizeof(double), s, a.main_part, a.lead_part, a.C, a.h, a.wl, a.nseg, raw);
}

}  // namespace sea

using namespace sea;

extern "C" int sea_train_ce_up_pow2_supported(int C, int h, int w, int H, int W) {
  return up2_scale(C, h, w, H, W) != 0 ? 1 : 0;
}

extern "C" size_t sea_train_ce_up_pow2_workspace_bytes(int B, int C, int h, int w, int H, int W) {
  const int S = up2_scale(C, h, w, H, W);
  if (B <= 0 || !S) return 0;
  return up2_rec_bytes(B, h, w, S) + up2_main_bytes(B, C, h, w) + up2_lead_bytes(B, C, h, w, S);
}

extern "C" int sea_train_ce_up_pow2_fwd(const float* low, const int64_t* y, const float* wgt, int64_t ignore_label, int B,
                                        int C, int h, int w, int H, int W, double* raw, void* workspace,
                                        size_t workspace_bytes, void* words, void* stream) {
  SEA_CHECK_ARG(low && y && raw && workspace && words);
  const int S = up2_scale(C, h, w, H, W);
  SEA_CHECK_ARG(S != 0 && B > 0 && B <= 65535 && h <= 65535);
  SEA_CHECK_ARG((int64_t)B * H * W < ((int64_t)1 << 31) && (int64_t)B * C * h * w < ((int64_t)1 << 31));
  SEA_CHECK_ARG((int64_t)B * (h + 1) * up2_nseg(w, S) < ((int64_t)1 << 31));
  SEA_CHECK_ARG(workspace_bytes >= sea_train_ce_up_pow2_workspace_bytes(B, C, h, w, H, W));
  SEA_CHECK_ARG((((uintptr_t)workspace) % 16) == 0 && (((uintptr_t)words) % 8) == 0 && (((uintptr_t)y) % 8) == 0 &&
                (((uintptr_t)low) % 4) == 0 && (((uintptr_t)raw) % 8) == 0);
  Up2Args a;
  a.low = low;
  a.y = (const long long*)y;
  a.w = wgt;
  a.ignore = (long long)ignore_label;
  a.C = C;
  a.h = h;
  a.wl = w;
  a.B = B;
  a.nseg = up2_nseg(w, S);
  char* base = (char*)workspace;
  a.rec = (TrainRecord*)base;
  a.main_part = (double*)(base + up2_rec_bytes(B, h, w, S));
  a.lead_part = (double*)(base + up2_rec_bytes(B, h, w, S) + up2_main_bytes(B, C, h, w));
  a.words = (TrainWords*)words;
  const hipStream_t st = (hipStream_t)stream;
  const int NS = (C + 63) / 64;
#define SEA_T2U_POW2(SS)                        \
  do {                                          \
    if (NS == 1)                                \
      up2_launch<SS, 1>(a, raw, st);            \
    else if (NS == 2)                           \
      up2_launch<SS, 2>(a, raw, st);            \
    else                                        \
      up2_launch<SS, 3>(a, raw, st);            \
  } while (0)
  if (S == 4)
    SEA_T2U_POW2(4);
  else
    SEA_T2U_POW2(16);
#undef SEA_T2U_POW2
  hipLaunchKernelGGL(train_reduce_k, dim3(1), dim3(256), 0, st, (const TrainRecord*)a.rec, B * (h + 1) * a.nseg, 0, 0.f,
                     (int*)nullptr, (TrainWords*)words);  // (no histogram: that is the OHEM select's)
  SEA_RETURN_LAST();
}

extern "C" int sea_train_ce_up_pow2_scale(const double* raw, const float* g, const void* words, float* dlow, int64_t n,
                                          void* stream) {
  SEA_CHECK_ARG(raw && g && words && dlow && n > 0 && n < ((int64_t)1 << 31));
  SEA_CHECK_ARG((((uintptr_t)words) % 8) == 0 && (((uintptr_t)raw) % 8) == 0 && (((uintptr_t)dlow) % 4) == 0);
  hipLaunchKernelGGL(train_ce_up_pow2_scale_k, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, raw, g,
                     (const TrainWords*)words, dlow, n);
  SEA_RETURN_LAST();
}
