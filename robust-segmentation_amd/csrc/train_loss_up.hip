// T2u: the training criteria (T2, train_loss.hip) fused with the model's final bilinear up-sampling, the way K2u
// (loss_upsampled.hip) fuses it into the attack's loss.
//
// UperNet computes its main and auxiliary logits at 1/4 resolution and up-samples both to the input size only to hand them
// to F.cross_entropy (semseg/models/convnext_upernet.py, the end of forward).  These kernels take the LOW-resolution logits
// (B, C, h, w), interpolate on the fly out of LDS, and return the gradient of the low-resolution tensor: the (B, C, H, W)
// logits, their log-soft-max and both gradients never exist.  Between forward and backward only the full-resolution loss
// plane (B*H*W floats, what sea_train_ohem_select works on) and the 64 bytes of device words live.
//
// Two launches, unlike K2u's one: the backward's normalisation (1 / sum w[y], or 1 / n_sel after the OHEM select) is known
// only after the whole forward.
//
// Ownership (K2u's general kernel): a workgroup owns a TL x TL tile of low-resolution pixels.  It stages the tile plus a
// one-pixel halo in LDS.  In the forward it owns the full-resolution pixels whose top-left source index (i0, j0) falls
// into the tile: it alone writes their loss and counts them in its record.  In the backward it alone writes the gradient
// of its low-resolution pixels; for that it recomputes the soft-max statistics of the full-resolution pixels with
// (i0, j0) in the tile or in the halo row / column above / left of it (every pixel whose footprint touches the tile) and
// GATHERS per (low-resolution pixel, class) over the four source cells around the pixel, rows then columns, in double:
// one owner per element, a fixed summation order, no float atomics => bitwise reproducible.
//
// Arithmetic is T2's: accurate expf, the soft-max denominator summed in double, the per-pixel log taken in double, the
// records reduced wave -> block -> train_reduce_k in a fixed order in double.  The interpolation is ATen's
// upsample_bilinear2d (align_corners=False) with K2u's expressions: axis_map_u (bilinear_map.h) and lerp2.
//
// LDS: 4*(C*(TL+2)^2 + 6*RMAX + 2*(TL+3)) bytes in both kernels plus 16*RMAX^2 (four statistics planes of the region) in
// the backward, RMAX = (TL+1)*ratio + 4.  TL is the largest edge <= 8 that keeps the backward within 64 KB (two
// workgroups per CU) and RMAX within 72: x4 gives TL = 8 up to C = 95 and TL = 6 at C = 151 (55 KB); x16 gives TL = 2.
//
// T2u-ac: PSPNet up-samples its two heads with align_corners=True (P2, psp_kernels.hip).  The kernels are templates on the
// interpolation rule (MapHalfPixel / MapCorners below): the axis map, its inverse, the expression tree of the four-tap
// sum and the plan's region bound are the rule's, everything else (ownership, LDS layout, summation order, records,
// workspace) is shared source.  The align_corners=False instantiation is the code it was before the template.  With
// align_corners=True, src = scale * dst with scale = (h-1)/(H-1): x8 (PSPNet's 60 -> 473) gives TL = 6 at C = 21 (RMAX 60, 63 KB) and
// TL = 4 at C = 151.
#include "bilinear_map.h"
#include "train_loss_common.h"

namespace sea {

constexpr int kUpMinClasses = 2, kUpMaxClasses = 192;  // K2u's ceiling (and MSF_MAX_CLASSES)
constexpr size_t kUpLdsBudget = 64 * 1024;
constexpr int kUpMaxRegion = 72;

// The two interpolation rules the kernels are instantiated for.  map: source pair and weight of a destination index;
// first_ge: its inverse (first destination index whose i0 is >= t); lerp: the rule's expression tree; scale: the float
// the launcher passes as rh / rw.
struct MapHalfPixel {  // align_corners=False: ATen's area_pixel_compute_scale, axis_map_u, lerp2
  static float scale(int n_in, int n_out) { return (float)n_in / (float)n_out; }
  // TL + 1 source cells of at most ceil(ratio) pixels each, plus slack for the clamped border cells
  static double region(int TL, int n_in, int n_out) { return (TL + 1) * ((double)n_out / n_in) + 4.0; }
  __device__ static __forceinline__ AxisMapU map(int dst, float r, int n_in) { return axis_map_u(dst, r, n_in); }
  __device__ static __forceinline__ int first_ge(int t, float r, int n_in, int n_out) {
    return first_dst_ge(t, r, n_in, n_out);
  }
  __device__ static __forceinline__ float lerp(float v00, float v01, float v10, float v11, float lx, float ly) {
    return lerp2(v00, v01, v10, v11, lx, ly);
  }
};

struct MapCorners {  // align_corners=True: P2's psp_ac_scale, ac_map, lerp_ac (l0 = 1 - l1, as ac_map computes it)
  static float scale(int n_in, int n_out) { return psp_ac_scale(n_in, n_out); }
  // src = scale * dst: the TL + 1 cells cover (TL + 1) / scale pixels (+ 1 for the ends, + float rounding); with one
  // source pixel the scale is 0 and every destination index reads it: the region is the whole axis
  static double region(int TL, int n_in, int n_out) {
    return n_in > 1 ? (TL + 1) * ((double)(n_out - 1) / (n_in - 1)) + 4.0 : (double)n_out;
  }
  __device__ static __forceinline__ AxisMapU map(int dst, float r, int n_in) {
    const AcMap a = ac_map(dst, r, n_in);
    AxisMapU m;
    m.i0 = a.i0;
    m.i1 = a.i0 + a.p;
    m.lam = a.l1;
    return m;
  }
  __device__ static __forceinline__ int first_ge(int t, float r, int n_in, int n_out) {
    return first_dst_ge_ac(t, r, n_in, n_out);
  }
  __device__ static __forceinline__ float lerp(float v00, float v01, float v10, float v11, float lx, float ly) {
    const AcMap mx = {0, 0, 1.f - lx, lx}, my = {0, 0, 1.f - ly, ly};
    return lerp_ac(v00, v01, v10, v11, mx, my);
  }
};

struct UpTile {
  int ya, xa, yb, xb;        // owned low-resolution tile [ya, yb) x [xa, xb)
  int Y0e, Y0o, Y1, X0e, X0o, X1;  // full-resolution rows / columns with i0 >= ya-1 (e), i0 >= ya (o), i0 >= yb
  int RH, RW;                // extended region (<= RMAX each)
};

// dynamic LDS carve-up shared by both kernels (the statistics planes follow in the backward)
struct UpSmem {
  float* lowt;               // [C][TLP][TLP]
  int *r_i0, *r_i1, *c_i0, *c_i1;  // [RMAX] local source indices (0 = low-resolution row ya-1)
  float *r_lam, *c_lam;      // [RMAX]
  int *rbeg, *cbeg;          // [TL+3] first region row / column whose source cell is >= ya-1+t
  float* rest;
};

__device__ __forceinline__ UpSmem up_carve(float* smem, int C, int TL, int RMAX) {
  const int TLP = TL + 2;
  UpSmem s;
  s.lowt = smem;
  s.r_i0 = (int*)(smem + C * TLP * TLP);
  s.r_i1 = s.r_i0 + RMAX;
  s.r_lam = (float*)(s.r_i1 + RMAX);
  s.c_i0 = (int*)(s.r_lam + RMAX);
  s.c_i1 = s.c_i0 + RMAX;
  s.c_lam = (float*)(s.c_i1 + RMAX);
  s.rbeg = (int*)(s.c_lam + RMAX);
  s.cbeg = s.rbeg + (TL + 3);
  s.rest = (float*)(s.cbeg + (TL + 3));
  return s;
}

// phase 0 of both kernels: the low-resolution tile with its halo (clamped into the image) and the axis tables.
// Ends with a barrier.
template <class M>
__device__ __forceinline__ UpTile up_stage(const UpSmem& s, const float* __restrict__ lowb, int C, int h, int wl, int H,
                                           int W, float rh, float rw, int TL, int RMAX) {
  const int TLP = TL + 2;
  UpTile t;
  t.ya = blockIdx.y * TL;
  t.xa = blockIdx.x * TL;
  t.yb = min(t.ya + TL, h);
  t.xb = min(t.xa + TL, wl);
  t.Y0e = M::first_ge(t.ya - 1, rh, h, H);
  t.Y0o = M::first_ge(t.ya, rh, h, H);
  t.Y1 = M::first_ge(t.yb, rh, h, H);
  t.X0e = M::first_ge(t.xa - 1, rw, wl, W);
  t.X0o = M::first_ge(t.xa, rw, wl, W);
  t.X1 = M::first_ge(t.xb, rw, wl, W);
  // RMAX bounds the region by construction of the plan (M::region: the pixels TL + 1 source cells can cover under this
  // rule); the clamp keeps every LDS index inside its table whatever the rounding of the float maps does
  if (t.Y1 - t.Y0e > RMAX) t.Y0e = t.Y1 - RMAX;
  if (t.X1 - t.X0e > RMAX) t.X0e = t.X1 - RMAX;
  t.Y0o = max(t.Y0o, t.Y0e);
  t.X0o = max(t.X0o, t.X0e);
  t.RH = t.Y1 - t.Y0e;
  t.RW = t.X1 - t.X0e;
  for (int i = threadIdx.x; i < C * TLP * TLP; i += 256) {
    const int c = i / (TLP * TLP), rem = i - c * TLP * TLP;
    const int ly = rem / TLP, lx = rem - ly * TLP;
    int gy = t.ya - 1 + ly, gx = t.xa - 1 + lx;
    gy = gy < 0 ? 0 : (gy > h - 1 ? h - 1 : gy);
    gx = gx < 0 ? 0 : (gx > wl - 1 ? wl - 1 : gx);
    s.lowt[i] = lowb[((int64_t)c * h + gy) * wl + gx];
  }
  for (int i = threadIdx.x; i < t.RH; i += 256) {
    const AxisMapU m = M::map(t.Y0e + i, rh, h);
    s.r_i0[i] = min(max(m.i0 - (t.ya - 1), 0), TLP - 1);
    s.r_i1[i] = min(max(m.i1 - (t.ya - 1), 0), TLP - 1);
    s.r_lam[i] = m.lam;
  }
  for (int i = threadIdx.x; i < t.RW; i += 256) {
    const AxisMapU m = M::map(t.X0e + i, rw, wl);
    s.c_i0[i] = min(max(m.i0 - (t.xa - 1), 0), TLP - 1);
    s.c_i1[i] = min(max(m.i1 - (t.xa - 1), 0), TLP - 1);
    s.c_lam[i] = m.lam;
  }
  if (threadIdx.x < TL + 3) {
    const int k = threadIdx.x;  // local cell index: global source index ya-1+k
    s.rbeg[k] = min(max(M::first_ge(t.ya - 1 + k, rh, h, H), t.Y0e), t.Y1) - t.Y0e;
    s.cbeg[k] = min(max(M::first_ge(t.xa - 1 + k, rw, wl, W), t.X0e), t.X1) - t.X0e;
  }
  __syncthreads();
  return t;
}

// soft-max statistics of one full-resolution pixel, interpolated out of the tile: me = max_c z (-3e38 in place of -inf),
// s = sum_c exp(z - me) in double, zy = z[lab] (0 if none).  Two passes over the classes: the maximum first, so that the
// sum needs no rescaling.
template <class M>
__device__ __forceinline__ void up_px_stats(const float* __restrict__ lowt, int P2, int C, int o00, int o01, int o10,
                                            int o11, float lx, float ly, int lab, float& me, double& s, float& zy) {
  float m = -INFINITY;
  for (int c = 0; c < C; ++c) {
    const float* t = lowt + c * P2;
    m = fmaxf(m, M::lerp(t[o00], t[o01], t[o10], t[o11], lx, ly));
  }
  me = (m == -INFINITY) ? -3.0e38f : m;
  s = 0.0;
  zy = 0.f;
  for (int c = 0; c < C; ++c) {
    const float* t = lowt + c * P2;
    const float z = M::lerp(t[o00], t[o01], t[o10], t[o11], lx, ly);
    s += (double)expf(z - me);
    zy = (lab == c) ? z : zy;
  }
}

// ---- forward --------------------------------------------------------------------------------------------------------
// grid = (tiles_x, tiles_y, B), block = 256.  One record per block, image-major.
template <class M>
__global__ __launch_bounds__(256) void train_ce_up_fwd_k(const float* __restrict__ low, const long long* __restrict__ y,
                                                         const float* __restrict__ w, long long ignore, float thresh,
                                                         int C, int h, int wl, int H, int W, float rh, float rw, int TL,
                                                         int RMAX, float* __restrict__ loss_px,
                                                         TrainRecord* __restrict__ rec, TrainWords* __restrict__ words) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const UpSmem s = up_carve(smem, C, TL, RMAX);
  const int b = blockIdx.z, TLP = TL + 2, P2 = TLP * TLP;
  const UpTile t = up_stage<M>(s, low + (int64_t)b * C * h * wl, C, h, wl, H, W, rh, rw, TL, RMAX);
  const int ro = t.Y0o - t.Y0e, co = t.X0o - t.X0e;  // the owned part of the region starts here
  const int OH = t.Y1 - t.Y0o, OW = t.X1 - t.X0o;
  double lsum = 0.0, wsum = 0.0, hsum = 0.0;
  int nvalid = 0, nhard = 0;
  for (int p = threadIdx.x; p < OH * OW; p += 256) {
    const int oi = p / OW, oj = p - oi * OW;
    const int ri = ro + oi, ci = co + oj;
    const int64_t pix = ((int64_t)b * H + (t.Y0o + oi)) * W + (t.X0o + oj);
    bool counted, bad;
    const int lab = train_label(y[pix], ignore, C, counted, bad);
    nvalid += counted ? 1 : 0;
    if (bad) words->err = 1;  // every writer stores the same value
    float lv = 0.f;
    if (lab >= 0) {
      const int r0 = s.r_i0[ri] * TLP, r1 = s.r_i1[ri] * TLP, c0 = s.c_i0[ci], c1 = s.c_i1[ci];
      float me, zy;
      double se;
      up_px_stats<M>(s.lowt, P2, C, r0 + c0, r0 + c1, r1 + c0, r1 + c1, s.c_lam[ci], s.r_lam[ri], lab, me, se, zy);
      // -log_softmax(z)[y] = log(sum exp(z - m)) - (z_y - m), rounded to float once (T2)
      const float ce = (float)(log(se) - ((double)zy - (double)me));
      const float wy = (w != nullptr) ? w[lab] : 1.f;
      lv = wy * ce;
      wsum += (double)wy;
    }
    loss_px[pix] = lv;
    lsum += (double)lv;
    const bool hard = lv > thresh;
    nhard += hard ? 1 : 0;
    hsum += hard ? (double)lv : 0.0;
  }
  __shared__ double s_d[3][4];
  __shared__ int s_i[2][4];
  lsum = wave_sum_d(lsum);
  wsum = wave_sum_d(wsum);
  hsum = wave_sum_d(hsum);
  nvalid = wave_sum_i(nvalid);
  nhard = wave_sum_i(nhard);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    s_d[0][wave] = lsum;
    s_d[1][wave] = wsum;
    s_d[2][wave] = hsum;
    s_i[0][wave] = nvalid;
    s_i[1][wave] = nhard;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    TrainRecord r;
    r.loss = (s_d[0][0] + s_d[0][1]) + (s_d[0][2] + s_d[0][3]);
    r.w = (s_d[1][0] + s_d[1][1]) + (s_d[1][2] + s_d[1][3]);
    r.hard = (s_d[2][0] + s_d[2][1]) + (s_d[2][2] + s_d[2][3]);
    r.n_valid = s_i[0][0] + s_i[0][1] + s_i[0][2] + s_i[0][3];
    r.n_hard = s_i[1][0] + s_i[1][1] + s_i[1][2] + s_i[1][3];
    rec[((int64_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = r;
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------
// dlow[b,c,i,j] = sum over the selected full-resolution pixels whose footprint touches (i, j) of
//   (bilinear weight) * K * (softmax(z)_c - [c == y]),  K = g * coef * w[y].
// CK classes per thread in phase B: 8 amortises the per-pixel statistics reads; 1 where a tile has too few
// (pixel, chunk) items to occupy the block (large ratios: TL = 2).
template <class M, int CK>
__global__ __launch_bounds__(256) void train_ce_up_bwd_k(const float* __restrict__ low, const long long* __restrict__ y,
                                                         const float* __restrict__ w, long long ignore, int ohem, int C,
                                                         int h, int wl, int H, int W, float rh, float rw, int TL,
                                                         int RMAX, const float* __restrict__ loss_px,
                                                         const float* __restrict__ g,
                                                         const TrainWords* __restrict__ words,
                                                         float* __restrict__ dlow) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const UpSmem s = up_carve(smem, C, TL, RMAX);
  float* pm = s.rest;  // RMAX*RMAX each: max, K / sum, K, label of the region's pixels
  float* pA = pm + RMAX * RMAX;
  float* pK = pA + RMAX * RMAX;
  int* plab = (int*)(pK + RMAX * RMAX);
  const int b = blockIdx.z, TLP = TL + 2, P2 = TLP * TLP;
  const UpTile t = up_stage<M>(s, low + (int64_t)b * C * h * wl, C, h, wl, H, W, rh, rw, TL, RMAX);
  const float gc = g[0] * words->coef;

  // ---- phase A: statistics of every selected pixel of the extended region
  for (int p = threadIdx.x; p < t.RH * t.RW; p += 256) {
    const int ri = p / t.RW, ci = p - ri * t.RW;
    const int64_t pix = ((int64_t)b * H + (t.Y0e + ri)) * W + (t.X0e + ci);
    bool counted, bad;
    int lab = train_label(y[pix], ignore, C, counted, bad);
    bool sel = lab >= 0;
    if (ohem) sel = sel && (loss_px[pix] != kUnselected);
    float me = 0.f, A = 0.f, K = 0.f;
    if (sel) {
      const int r0 = s.r_i0[ri] * TLP, r1 = s.r_i1[ri] * TLP, c0 = s.c_i0[ci], c1 = s.c_i1[ci];
      float zy;
      double se;
      up_px_stats<M>(s.lowt, P2, C, r0 + c0, r0 + c1, r1 + c0, r1 + c1, s.c_lam[ci], s.r_lam[ri], lab, me, se, zy);
      K = gc * ((w != nullptr) ? w[lab] : 1.f);
      A = (float)((double)K / se);
    }
    pm[p] = me;
    pA[p] = A;
    pK[p] = K;
    plab[p] = sel ? lab : -1;
  }
  __syncthreads();

  // ---- phase B: a thread owns one low-resolution pixel and CK classes.  The pixels that touch low-resolution pixel
  // (yl, xl) live in the four source cells (yl-1 | yl) x (xl-1 | xl); inside one cell all pixels interpolate between
  // the same four low-resolution values, which sit in registers.
  const int nlx = t.xb - t.xa, nly = t.yb - t.ya;
  const int nchunk = (C + CK - 1) / CK;
  float* dlb = dlow + (int64_t)b * C * h * wl;
  for (int item = threadIdx.x; item < nchunk * nly * nlx; item += 256) {
    const int ck = item / (nly * nlx), rem = item - ck * nly * nlx;
    const int ty = rem / nlx, tx = rem - ty * nlx;
    const int yl = ty + 1, xl = tx + 1;  // local coordinates inside lowt
    const int c0 = ck * CK;
    double acc[CK];
#pragma unroll
    for (int k = 0; k < CK; ++k) acc[k] = 0.0;
    for (int qy = 0; qy < 2; ++qy) {
      const int cy = yl - 1 + qy;  // source cell row (local)
      const int i_lo = s.rbeg[cy], i_hi = s.rbeg[cy + 1];
      if (i_lo >= i_hi) continue;
      const int cy1 = s.r_i1[i_lo];  // constant inside the cell
      for (int qx = 0; qx < 2; ++qx) {
        const int cx = xl - 1 + qx;
        const int j_lo = s.cbeg[cx], j_hi = s.cbeg[cx + 1];
        if (j_lo >= j_hi) continue;
        const int cx1 = s.c_i1[j_lo];
        float v00[CK], v01[CK], v10[CK], v11[CK];
#pragma unroll
        for (int k = 0; k < CK; ++k) {
          const float* tt = s.lowt + min(c0 + k, C - 1) * P2;
          v00[k] = tt[cy * TLP + cx];
          v01[k] = tt[cy * TLP + cx1];
          v10[k] = tt[cy1 * TLP + cx];
          v11[k] = tt[cy1 * TLP + cx1];
        }
        for (int ri = i_lo; ri < i_hi; ++ri) {
          const float ly = s.r_lam[ri];
          const float wyv = ((cy == yl) ? (1.f - ly) : 0.f) + ((cy1 == yl) ? ly : 0.f);
          if (wyv == 0.f) continue;
          for (int ci = j_lo; ci < j_hi; ++ci) {
            const float lx = s.c_lam[ci];
            const float wv = wyv * (((cx == xl) ? (1.f - lx) : 0.f) + ((cx1 == xl) ? lx : 0.f));
            const int p = ri * t.RW + ci;
            const int lb = plab[p];
            if (wv == 0.f || lb < 0) continue;
            const float mm = pm[p], A = pA[p], K = pK[p];
#pragma unroll
            for (int k = 0; k < CK; ++k) {
              const float e = expf(M::lerp(v00[k], v01[k], v10[k], v11[k], lx, ly) - mm);
              const float tv = A * e;
              const float dz = (lb == c0 + k) ? tv - K : tv;  // T2's per-pixel gradient, rounded as T2 rounds it
              acc[k] += (double)wv * (double)dz;
            }
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < CK; ++k)
      if (c0 + k < C) dlb[((int64_t)(c0 + k) * h + (t.ya + ty)) * wl + (t.xa + tx)] = (float)acc[k];
  }
}

struct UpTrainPlan {
  int TL, RMAX, tiles_x, tiles_y;
  size_t lds_fwd, lds_bwd;
};

// the low-resolution tile edge: as large as the LDS budget of the backward and the region bound allow.  M::region bounds
// the full-resolution rows (columns) whose i0 falls into TL + 1 consecutive source cells.
template <class M>
static bool plan_train_up(int C, int h, int wl, int H, int W, UpTrainPlan* out) {
  if (C < kUpMinClasses || C > kUpMaxClasses || h <= 0 || wl <= 0 || H < h || W < wl) return false;
  for (int TL = 8; TL >= 1; --TL) {
    const double rh_d = M::region(TL, h, H), rw_d = M::region(TL, wl, W);
    const double rmax_d = rh_d > rw_d ? rh_d : rw_d;
    if (rmax_d > (double)kUpMaxRegion) continue;
    const int RMAX = (int)rmax_d;
    const size_t TLP = TL + 2;
    const size_t base = sizeof(float) * ((size_t)C * TLP * TLP + 6 * (size_t)RMAX + 2 * (size_t)(TL + 3));
    const size_t bwd = base + sizeof(float) * 4 * (size_t)RMAX * RMAX;
    if (bwd <= kUpLdsBudget) {
      out->TL = TL;
      out->RMAX = RMAX;
      out->tiles_x = (wl + TL - 1) / TL;
      out->tiles_y = (h + TL - 1) / TL;
      out->lds_fwd = base;
      out->lds_bwd = bwd;
      return out->tiles_x <= 65535 && out->tiles_y <= 65535;
    }
  }
  return false;
}

static inline bool up_aligned(const void* p, size_t bytes) { return (((uintptr_t)p) % bytes) == 0; }

template <class M>
static size_t up_workspace_bytes(int B, int C, int h, int w, int H, int W) {
  UpTrainPlan p;
  if (B <= 0 || !plan_train_up<M>(C, h, w, H, W, &p)) return 0;
  return kOffRecords + (size_t)B * p.tiles_x * p.tiles_y * sizeof(TrainRecord);
}

template <class M>
static int up_fwd(const float* low, const int64_t* y, const float* wgt, int64_t ignore_label, float thresh,
                  int reduce_mean, int B, int C, int h, int w, int H, int W, float* loss_px, void* workspace,
                  size_t workspace_bytes, void* words, void* stream) {
  SEA_CHECK_ARG(low && y && loss_px && workspace && words);
  UpTrainPlan p;
  SEA_CHECK_ARG(B > 0 && B <= 65535 && plan_train_up<M>(C, h, w, H, W, &p));
  SEA_CHECK_ARG((int64_t)B * H * W < ((int64_t)1 << 31));
  SEA_CHECK_ARG(workspace_bytes >= up_workspace_bytes<M>(B, C, h, w, H, W));
  SEA_CHECK_ARG(up_aligned(workspace, 16) && up_aligned(words, 8) && up_aligned(y, 8) && up_aligned(low, 4));
  TrainRecord* rec = (TrainRecord*)((char*)workspace + kOffRecords);
  hipStream_t s = (hipStream_t)stream;
  const float rh = M::scale(h, H), rw = M::scale(w, W);
  auto k = train_ce_up_fwd_k<M>;
  if (p.lds_fwd > 48 * 1024)
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_fwd);
  hipLaunchKernelGGL(k, dim3(p.tiles_x, p.tiles_y, B), dim3(256), p.lds_fwd, s, low, (const long long*)y, wgt,
                     (long long)ignore_label, thresh, C, h, w, H, W, rh, rw, p.TL, p.RMAX, loss_px, rec,
                     (TrainWords*)words);
  hipLaunchKernelGGL(train_reduce_k, dim3(1), dim3(256), 0, s, (const TrainRecord*)rec, B * p.tiles_x * p.tiles_y,
                     reduce_mean ? 0 : 1, thresh, (int*)((char*)workspace + kOffHist), (TrainWords*)words);
  SEA_RETURN_LAST();
}

template <class M>
static int up_bwd(const float* low, const int64_t* y, const float* wgt, int64_t ignore_label, int ohem, int B, int C,
                  int h, int w, int H, int W, const float* loss_px, const float* g, const void* words, float* dlow,
                  void* stream) {
  SEA_CHECK_ARG(low && y && loss_px && g && words && dlow);
  UpTrainPlan p;
  SEA_CHECK_ARG(B > 0 && B <= 65535 && plan_train_up<M>(C, h, w, H, W, &p));
  SEA_CHECK_ARG((int64_t)B * H * W < ((int64_t)1 << 31));
  SEA_CHECK_ARG(up_aligned(words, 8) && up_aligned(y, 8) && up_aligned(low, 4) && up_aligned(dlow, 4));
  hipStream_t s = (hipStream_t)stream;
  const float rh = M::scale(h, H), rw = M::scale(w, W);
  const dim3 grid(p.tiles_x, p.tiles_y, B), block(256);
#define SEA_T2U_BWD(CK)                                                                                              \
  do {                                                                                                               \
    auto k = train_ce_up_bwd_k<M, CK>;                                                                               \
    if (p.lds_bwd > 48 * 1024)                                                                                       \
      (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bwd);         \
    hipLaunchKernelGGL(k, grid, block, p.lds_bwd, s, low, (const long long*)y, wgt, (long long)ignore_label, ohem, C, \
                       h, w, H, W, rh, rw, p.TL, p.RMAX, loss_px, g, (const TrainWords*)words, dlow);                \
  } while (0)
  if (((C + 7) / 8) * p.TL * p.TL >= 256)
    SEA_T2U_BWD(8);
  else
    SEA_T2U_BWD(1);
#undef SEA_T2U_BWD
  SEA_RETURN_LAST();
}

}  // namespace sea

using namespace sea;

extern "C" int sea_train_ce_up_tile(int C, int h, int w, int H, int W) {
  UpTrainPlan p;
  return plan_train_up<MapHalfPixel>(C, h, w, H, W, &p) ? p.TL : 0;
}

extern "C" size_t sea_train_ce_up_workspace_bytes(int B, int C, int h, int w, int H, int W) {
  return up_workspace_bytes<MapHalfPixel>(B, C, h, w, H, W);
}

extern "C" int sea_train_ce_up_fwd(const float* low, const int64_t* y, const float* wgt, int64_t ignore_label,
                                   float thresh, int reduce_mean, int B, int C, int h, int w, int H, int W,
                                   float* loss_px, void* workspace, size_t workspace_bytes, void* words, void* stream) {
  return up_fwd<MapHalfPixel>(low, y, wgt, ignore_label, thresh, reduce_mean, B, C, h, w, H, W, loss_px, workspace,
                              workspace_bytes, words, stream);
}

// workspace: the gather needs no scratch; the arguments are kept for a variant with partial sums
extern "C" int sea_train_ce_up_bwd(const float* low, const int64_t* y, const float* wgt, int64_t ignore_label, int ohem,
                                   int B, int C, int h, int w, int H, int W, const float* loss_px, const float* g,
                                   const void* words, float* dlow, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  (void)workspace;
  (void)workspace_bytes;
  return up_bwd<MapHalfPixel>(low, y, wgt, ignore_label, ohem, B, C, h, w, H, W, loss_px, g, words, dlow, stream);
}

// ---- T2u-ac: the same kernels with PSPNet's align_corners=True rule ----------------------------------------------------
extern "C" int sea_train_ce_up_ac_tile(int C, int h, int w, int H, int W) {
  UpTrainPlan p;
  return plan_train_up<MapCorners>(C, h, w, H, W, &p) ? p.TL : 0;
}

extern "C" size_t sea_train_ce_up_ac_workspace_bytes(int B, int C, int h, int w, int H, int W) {
  return up_workspace_bytes<MapCorners>(B, C, h, w, H, W);
}

extern "C" int sea_train_ce_up_ac_fwd(const float* low, const int64_t* y, const float* wgt, int64_t ignore_label,
                                      float thresh, int reduce_mean, int B, int C, int h, int w, int H, int W,
                                      float* loss_px, void* workspace, size_t workspace_bytes, void* words,
                                      void* stream) {
  return up_fwd<MapCorners>(low, y, wgt, ignore_label, thresh, reduce_mean, B, C, h, w, H, W, loss_px, workspace,
                            workspace_bytes, words, stream);
}

extern "C" int sea_train_ce_up_ac_bwd(const float* low, const int64_t* y, const float* wgt, int64_t ignore_label,
                                      int ohem, int B, int C, int h, int w, int H, int W, const float* loss_px,
                                      const float* g, const void* words, float* dlow, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  (void)workspace;
  (void)workspace_bytes;
  return up_bwd<MapCorners>(low, y, wgt, ignore_label, ohem, B, C, h, w, H, W, loss_px, g, words, dlow, stream);
}
