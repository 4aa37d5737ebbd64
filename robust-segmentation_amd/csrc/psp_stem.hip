// P4 (model side): the torchvision-style stem of PSPNet(clean=False) for frozen parameters
// (backbones/resnet_ddcat.py:115-131: Conv2d(3, 64, 7, stride 2, pad 3, bias=False) -> BatchNorm -> ReLU ->
// MaxPool2d(3, 2, 1)), forward and input gradient, one launch each:
//   out = maxpool3x3s2p1(relu(scale[c] * conv7x7s2p3(x, w)[c] + shift[c]))
// The library line writes the pre-pool map (115 MB at 8 x 473^2), passes over it for BatchNorm and ReLU, pools it, keeps
// it for the backward, and ATen's pool keeps int64 indices besides.  Here the pre-pool map lives in LDS only, and what the
// backward needs is one byte per OUTPUT element.
//   psp_stem_fwd : a block owns 7 x 8 pooled pixels x 64 channels = 15 x 17 = 255 pre-pool positions (each computed once
//                  per block: 255 / (4 * 56) = 1.14 x the convolution).  Phase 1: one lane = one pre-pool position; its
//                  7 x 7 x 3 = 147 inputs live in registers and the channels are a loop of pairs, so the weights are
//                  wave-uniform scalar loads (2 x 147 per iteration, which depend on the loop counter and cannot be
//                  hoisted) and the body is 294 FMAs in two independent chains.  v = scale * conv + shift goes to LDS as
//                  tile[c][position] (row length 255, odd: conflict-free for lanes = positions and for lanes = channels).
//                  Phase 2: one lane = one channel of one pooled pixel: the row-major scan of the 3 x 3 window over the
//                  positions inside the map with a strict ">" (torch's winner: ReLU is monotone, so it changes neither
//                  the winner nor its first occurrence where v_max > 0), out = max(v_max, 0) and rec = ky * 3 + kx of
//                  the winner, 15 where v_max <= 0 (no gradient passes).  out / rec are NHWC: a wave writes 256 / 64
//                  contiguous bytes.
//   psp_stem_bwd : a gather.  A block owns 8 x 8 patches of 2 x 2 input pixels; the patch (m, n) needs the pre-pool
//                  gradient g at rows m - 1 ... m + 2, columns n - 1 ... n + 2 (stride 2: an even input row meets the
//                  taps ky = 1, 3, 5, an odd one ky = 0, 2, 4, 6), so the block builds the 11 x 11 x 64 tile of g in LDS
//                  first: a pre-pool position belongs to at most 2 x 2 pool windows, and g is the sum, rows outer and
//                  columns inner, of dout of those windows whose rec names it, times scale[c] (lanes = channels: dout and
//                  rec are read in whole NHWC pixels).  Then, as M9's backward, wave q takes channels [16 q, 16 q + 16)
//                  for all 64 patches (weights wave-uniform; every one of a channel's 147 weights meets exactly one of the
//                  lane's 3 x 2 x 2 sums) and the four partial sums meet in LDS in a fixed order.  Every element of dx is
//                  written.
// All fp32 FMA in a fixed order, no atomics: bitwise repeatable.  Finite inputs.  Any H, W >= 1.
#include "sea_common.h"

namespace sea {

constexpr int PS_CO = 64;                    // output channels
constexpr int PS_K = 147;                    // 3 * 7 * 7 weights per output channel
constexpr int PS_PH = 7, PS_PW = 8;          // pooled pixels of a forward block
constexpr int PS_TH = 2 * PS_PH + 1, PS_TW = 2 * PS_PW + 1, PS_TN = PS_TH * PS_TW;   // 15 x 17 = 255 pre-pool positions
constexpr int PS_NONE = 15;                  // rec: no gradient
constexpr int PS_BP = 8;                     // backward: 8 x 8 patches of 2 x 2 input pixels per block
constexpr int PS_GW = PS_BP + 3, PS_GN = PS_GW * PS_GW;                              // 11 x 11 = 121 positions of g
static_assert(PS_TN <= 256 && (PS_TN & 1) == 1 && (PS_GN & 1) == 1, "one lane per position; odd LDS row lengths");
static_assert(PS_CO * PS_TN * 4 <= 65536 && 4 * 12 * 64 <= PS_CO * PS_GN, "LDS");

// x (B,3,H,W) NCHW, w (64,3,7,7), out (B,Hp,Wp,64) NHWC, rec the same shape in bytes (may be null)
__global__ __launch_bounds__(256) void psp_stem_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ scale,
                                                           const float* __restrict__ shift, float* __restrict__ out,
                                                           unsigned char* __restrict__ rec, int H, int W, int Hc, int Wc,
                                                           int Hp, int Wp) {
  __shared__ float tile[PS_CO * PS_TN];
  const int tid = threadIdx.x;
  const int b = blockIdx.z, pi0 = blockIdx.y * PS_PH, pj0 = blockIdx.x * PS_PW;
  if (tid < PS_TN) {
    const int ti = tid / PS_TW, tj = tid - ti * PS_TW;
    // pre-pool position (i, j) = (2 pi0 - 1 + ti, 2 pj0 - 1 + tj); its input window starts at (2 i - 3, 2 j - 3).  Positions
    // outside the map are computed from whatever the bounds check leaves and never looked at in phase 2.
    const int Y0 = 2 * (2 * pi0 - 1 + ti) - 3, X0 = 2 * (2 * pj0 - 1 + tj) - 3;
    const int64_t plane = (int64_t)H * W;
    const float* xb = x + (int64_t)b * 3 * plane;
    float xin[PS_K];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int ky = 0; ky < 7; ++ky)
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
          const int Y = Y0 + ky, X = X0 + kx;
          const bool ok = Y >= 0 && Y < H && X >= 0 && X < W;
          xin[c * 49 + ky * 7 + kx] = ok ? xb[c * plane + (int64_t)Y * W + X] : 0.f;
        }
#pragma unroll 1
    for (int o = 0; o < PS_CO; o += 2) {
      const float* w0 = w + o * PS_K;
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int t = 0; t < PS_K; ++t) {
        s0 = fmaf(w0[t], xin[t], s0);
        s1 = fmaf(w0[PS_K + t], xin[t], s1);
      }
      tile[o * PS_TN + tid] = fmaf(scale[o], s0, shift[o]);
      tile[(o + 1) * PS_TN + tid] = fmaf(scale[o + 1], s1, shift[o + 1]);
    }
  }
  __syncthreads();
  const int c = tid & 63;
  const int q = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float* tc = tile + c * PS_TN;
  for (int p = q; p < PS_PH * PS_PW; p += 4) {
    const int pr = p / PS_PW, pc = p - pr * PS_PW;
    const int pi = pi0 + pr, pj = pj0 + pc;
    if (pi >= Hp || pj >= Wp) continue;         // (wave-uniform)
    float vmax = -INFINITY;
    int best = PS_NONE;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int i = 2 * pi - 1 + ky, j = 2 * pj - 1 + kx;
        const float v = tc[(2 * pr + ky) * PS_TW + 2 * pc + kx];
        if (i >= 0 && i < Hc && j >= 0 && j < Wc && v > vmax) vmax = v, best = ky * 3 + kx;
      }
    if (!(vmax > 0.f)) vmax = 0.f, best = PS_NONE;
    const int64_t at = (((int64_t)b * Hp + pi) * Wp + pj) * PS_CO + c;
    out[at] = vmax;
    if (rec != nullptr) rec[at] = (unsigned char)best;
  }
}

// dout (B,Hp,Wp,64) NHWC, rec the same shape in bytes, w (64,3,7,7) -> dx (B,3,H,W) NCHW
__global__ __launch_bounds__(256) void psp_stem_bwd_kernel(const float* __restrict__ dout,
                                                           const unsigned char* __restrict__ rec,
                                                           const float* __restrict__ w, const float* __restrict__ scale,
                                                           float* __restrict__ dx, int H, int W, int Hc, int Wc, int Hp,
                                                           int Wp) {
  __shared__ float gt[PS_CO * PS_GN];           // g[c][position]; afterwards the partial sums [4][12][64]
  const int tid = threadIdx.x, ln = tid & 63;
  const int q = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.z, m0 = blockIdx.y * PS_BP, n0 = blockIdx.x * PS_BP;
  const float sc = scale[ln];
  for (int pos = q; pos < PS_GN; pos += 4) {    // lanes = channels; everything but the loads' lane offset is wave-uniform
    const int ti = pos / PS_GW, tj = pos - ti * PS_GW;
    const int i = m0 - 1 + ti, j = n0 - 1 + tj;
    float g = 0.f;
    if (i >= 0 && i < Hc && j >= 0 && j < Wc) {
      // an even row is the middle row (ky = 1) of window i / 2; an odd one the last row (ky = 2) of window (i - 1) / 2 and
      // the first (ky = 0) of window (i + 1) / 2, if there is one
      const int nr = (i & 1) ? ((i + 1) / 2 < Hp ? 2 : 1) : 1, nc = (j & 1) ? ((j + 1) / 2 < Wp ? 2 : 1) : 1;
      for (int a = 0; a < nr; ++a) {
        const int pi = (i >> 1) + a, ky = (i & 1) ? 2 - 2 * a : 1;
        for (int e = 0; e < nc; ++e) {
          const int pj = (j >> 1) + e, kx = (j & 1) ? 2 - 2 * e : 1;
          const int64_t at = (((int64_t)b * Hp + pi) * Wp + pj) * PS_CO + ln;
          const float d = dout[at];
          g += (int)rec[at] == ky * 3 + kx ? d : 0.f;
        }
      }
      g *= sc;
    }
    gt[ln * PS_GN + pos] = g;
  }
  __syncthreads();
  // patch (m, n) = (m0 + pm, n0 + pn) owns dx rows 2 m, 2 m + 1 and columns 2 n, 2 n + 1.  Input row Y = 2 i - 3 + ky, so
  // tap ky meets row parity py = 1 - (ky & 1) at pre-pool row i = m + (py + 3 - ky) / 2 = m - 1 + ra[ky]
  const int pm = ln >> 3, pn = ln & 7;
  float acc[3][2][2];
#pragma unroll
  for (int c = 0; c < 3; ++c) acc[c][0][0] = acc[c][0][1] = acc[c][1][0] = acc[c][1][1] = 0.f;
#pragma unroll 1
  for (int oo = 0; oo < PS_CO / 4; ++oo) {
    const int o = q * (PS_CO / 4) + oo;
    const float* go = gt + o * PS_GN + pm * PS_GW + pn;
    float g[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int e = 0; e < 4; ++e) g[a][e] = go[a * PS_GW + e];
    const float* wo = w + o * PS_K;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int ky = 0; ky < 7; ++ky)
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
          const int py = 1 - (ky & 1), px = 1 - (kx & 1);
          const int ra = (py + 3 - ky) / 2 + 1, ca = (px + 3 - kx) / 2 + 1;
          acc[c][py][px] = fmaf(wo[c * 49 + ky * 7 + kx], g[ra][ca], acc[c][py][px]);
        }
  }
  __syncthreads();                              // every wave is done with g: the tile becomes part[4][12][64]
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
      for (int px = 0; px < 2; ++px) gt[(q * 12 + c * 4 + py * 2 + px) * 64 + ln] = acc[c][py][px];
  __syncthreads();
  // wave q finishes sums 3 q ... 3 q + 2 of every patch: (channel, row, column) = (k / 4, (k / 2) & 1, k & 1)
  const int64_t plane = (int64_t)H * W;
  float* xb = dx + (int64_t)b * 3 * plane;
  const int Y0 = 2 * (m0 + pm), X0 = 2 * (n0 + pn);
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int k = q * 3 + t;
    const float v = ((gt[k * 64 + ln] + gt[(12 + k) * 64 + ln]) + gt[(24 + k) * 64 + ln]) + gt[(36 + k) * 64 + ln];
    const int c = k >> 2, Y = Y0 + ((k >> 1) & 1), X = X0 + (k & 1);
    if (Y < H && X < W) xb[c * plane + (int64_t)Y * W + X] = v;
  }
}

}  // namespace sea

using namespace sea;

// x (B,3,H,W) NCHW fp32 contiguous; w (64,3,7,7); scale / shift (64): the folded eval BatchNorm; out (B,Hp,Wp,64) NHWC
// with Hc = (H-1)/2+1, Hp = (Hc-1)/2+1 (W alike); rec (B,Hp,Wp,64) bytes or NULL
extern "C" int sea_psp_stem_fwd(const float* x, const float* w, const float* scale, const float* shift, float* out,
                                unsigned char* rec, int B, int H, int W, void* stream) {
  SEA_CHECK_ARG(x && w && scale && shift && out && B > 0 && B <= 65535 && H > 0 && W > 0);
  const int Hc = (H - 1) / 2 + 1, Wc = (W - 1) / 2 + 1, Hp = (Hc - 1) / 2 + 1, Wp = (Wc - 1) / 2 + 1;
  const dim3 grid((unsigned)((Wp + PS_PW - 1) / PS_PW), (unsigned)((Hp + PS_PH - 1) / PS_PH), (unsigned)B);
  SEA_CHECK_ARG(grid.y <= 65535);
  hipLaunchKernelGGL(psp_stem_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, w, scale, shift, out, rec, H, W, Hc,
                     Wc, Hp, Wp);
  SEA_RETURN_LAST();
}

// dout (B,Hp,Wp,64) NHWC and rec of the forward -> dx (B,3,H,W) NCHW, every element written
extern "C" int sea_psp_stem_bwd(const float* dout, const unsigned char* rec, const float* w, const float* scale, float* dx,
                                int B, int H, int W, void* stream) {
  SEA_CHECK_ARG(dout && rec && w && scale && dx && B > 0 && B <= 65535 && H > 0 && W > 0);
  const int Hc = (H - 1) / 2 + 1, Wc = (W - 1) / 2 + 1, Hp = (Hc - 1) / 2 + 1, Wp = (Wc - 1) / 2 + 1;
  const dim3 grid((unsigned)((Wc + PS_BP - 1) / PS_BP), (unsigned)((Hc + PS_BP - 1) / PS_BP), (unsigned)B);
  SEA_CHECK_ARG(grid.y <= 65535);
  hipLaunchKernelGGL(psp_stem_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, dout, rec, w, scale, dx, H, W, Hc, Wc,
                     Hp, Wp);
  SEA_RETURN_LAST();
}
