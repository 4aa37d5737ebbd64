// M2 / M6: which kernel a bilinear up-sampling call (sea_upsample_bilinear_*, sea_tap_gather_*) runs, with which template
// parameter, grid and launch-time scalars -- the WHOLE decision, and every refusal that depends on integers only, as one pure
// host function.  Plain C++17 without HIP headers (tests/test_upsample_plan_cpu.py sweeps it through sea_upsample_plan).  The
// launchers of upsample_kernels.hip / fpn_fused.hip check their pointers, fill a query, take the plan and decide nothing.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sea_hip.h"
#include "launch_grid.h"  // SEA_ERR_ARG, grid_for_xcd

namespace sea {
// One value per kernel function of the family (upsample_*_kernel, tap_gather_*_kernel; GENERAL = the one without a suffix).
// The template values S that exist for each are the lists of the launchers' dispatch_s calls; DESIGN.md, "M2", has the map.
enum UpsampleKernel {
  UPK_NCHW_FWD_GENERAL, UPK_NCHW_FWD_POW2, UPK_NCHW_FWD_CELLS, UPK_NCHW_BWD_GENERAL, UPK_NCHW_BWD_ROWS, UPK_NCHW_BWD_POW2,
  UPK_NHWC_FWD, UPK_NHWC_FWD_CELLS, UPK_NHWC_BWD_GENERAL, UPK_NHWC_BWD_SMALL, UPK_NHWC_BWD_POW2,
  UPK_TAP_FWD, UPK_TAP_BWD_GENERAL, UPK_TAP_BWD_POW2
};

struct UpsampleQuery {
  int op;                // SEA_UP_* of sea_hip.h
  int64_t planes;        // NCHW: planes (B * C); NHWC and tap gather: B
  int C, h, w, H, W;     // C: NHWC and tap gather only
  int64_t pixel_stride;  // NHWC: floats between consecutive pixels of y / gy
  uintptr_t src, dst;    // what the kernel reads / writes: alignment is all that matters (two inputs: their bitwise OR)
  bool general_only;     // SEA_UPSAMPLE_GENERAL and SEA_XCD_ORDER: the launchers copy them from the process configuration,
  int xcd_order;         // which the plan itself never reads
};
struct UpsamplePlan {
  int kernel, S;         // S: the template parameter (0 where the kernel has none)
  int grid_x, grid_y, threads;
  size_t lds;            // dynamic LDS bytes (the tiled NCHW backward)
  int chunk, nchunks;    // the two general NCHW kernels: planes per launch at most (the grid's z extent), launches; else 0
  int64_t total;         // work items of a grid-stride kernel: float4s, cells, input pixels or the rows kernel's units
  int xo, nt;            // the kernel's `xcd` argument; NCHW forward cells: non-temporal stores
  int lcols, RP, bands, per_xcd, TI, RMAX;  // NCHW backward: rows (four) and tiled (two)
  int nbh, nbw;          // tap gather forward: blocks of kTapBlock x kTapBlock output pixels per axis
};

constexpr int kUpsampleChunk = 65535;  // planes per launch of the general NCHW kernels (gridDim.z)
constexpr int kTapBlock = 4;           // tap gather forward: one lane = a 4 x 4 block of output pixels

// integer power-of-two factor in both axes (2, 4, 8, 16), 0 otherwise
static inline int pow2_factor(int h, int w, int H, int W) {
  for (int S = 2; S <= 16; S *= 2)
    if ((int64_t)h * S == H && (int64_t)w * S == W) return S;
  return 0;
}

static inline int upsample_plan(const UpsampleQuery& q, UpsamplePlan* p) {
  *p = UpsamplePlan{};
  const int h = q.h, w = q.w, H = q.H, W = q.W, CG = q.C / 4;
  const int64_t n = q.planes;
  if (q.op < SEA_UP_NCHW_FWD || q.op > SEA_UP_TAP_BWD || q.xcd_order < 0 || q.xcd_order > 2 || n <= 0 || h <= 0 || w <= 0)
    return SEA_ERR_ARG;
  // (tap gather forward: the 3x3 coarse window per tap covers 4 consecutive sample positions only for factors >= 3)
  const int fmin = q.op == SEA_UP_TAP_FWD ? 3 : 1;
  if ((int64_t)H < (int64_t)fmin * h || (int64_t)W < (int64_t)fmin * w) return SEA_ERR_ARG;
  if (q.op >= SEA_UP_NHWC_FWD && (n > INT32_MAX || q.C <= 0 || (q.C % 4) != 0 || ((q.src | q.dst) & 15) != 0)) return SEA_ERR_ARG;
  if ((q.op == SEA_UP_NHWC_FWD || q.op == SEA_UP_NHWC_BWD) && (q.pixel_stride < q.C || (q.pixel_stride % 4) != 0))
    return SEA_ERR_ARG;
  const int S = q.general_only ? 0 : pow2_factor(h, w, H, W);
  p->threads = 256, p->grid_y = 1;
  auto chunked = [&](int kernel, int gx, int gy) {  // the general NCHW kernels: grid z = planes
    p->kernel = kernel, p->grid_x = gx, p->grid_y = gy;
    p->chunk = kUpsampleChunk, p->nchunks = (int)((n + kUpsampleChunk - 1) / kUpsampleChunk);
    return 0;
  };
  auto grid_stride = [&](int kernel, int s, int64_t total, int items_per_block, int xo) {
    p->kernel = kernel, p->S = s, p->total = total, p->xo = xo, p->grid_x = grid_for_xcd(total, items_per_block);
    return 0;
  };
  // pure streams (the other side is S^2 times smaller): the plain block order measured faster than the XCD-contiguous one
  const int xo_stream = q.xcd_order == 2;  // (151 planes x 8, 128 -> 512: forward 341 vs 379 us, backward 386 vs 411 us)

  switch (q.op) {
    case SEA_UP_NCHW_FWD:
      if (S && (q.dst & 15) == 0 && (W & 3) == 0) {  // float4 stores: W % 4 == 0 and a 16-byte aligned base
        if (S == 2) return grid_stride(UPK_NCHW_FWD_POW2, 2, n * H * (W / 4), 256, xo_stream);  // one float4 per lane
        p->nt = n * H * W * 4 > (192ll << 20);  // non-temporal stores by output size
        return grid_stride(UPK_NCHW_FWD_CELLS, S, n * (h + 1) * (W / 4), 256, xo_stream);
      }
      return chunked(UPK_NCHW_FWD_GENERAL, (W + 63) / 64, (H + 15) / 16);
    case SEA_UP_NCHW_BWD: {
      const int cols = W / 4;
      if (S && (W & 3) == 0 && (cols == 32 || cols == 64 || cols == 128 || cols == 256) && (q.src & 15) == 0 &&
          n < (1 << 24)) {
        int lcols = 5;
        while ((1 << lcols) < cols) ++lcols;
        const int nsub = 256 / cols, RP = 16 / S > 2 ? 16 / S : 2;  // RP input rows per sub-band: ~5 cells of S rows each
        const int bands = (h + nsub * RP - 1) / (nsub * RP);
        const int64_t units = n * bands;
        if (units < (1ll << 30)) {
          p->kernel = UPK_NCHW_BWD_ROWS, p->S = S, p->total = units, p->lcols = lcols, p->RP = RP, p->bands = bands;
          p->per_xcd = q.xcd_order ? (int)((units + 7) / 8) : 0;
          p->grid_x = p->per_xcd ? p->per_xcd * 8 : (int)units;
          return 0;
        }
      }
      const int VL = S / 2 >= 4 ? 4 : S / 2;  // vector loads of VL floats at multiples of S/2 floats from the row start
      if (S && (q.src & (uintptr_t)(VL * 4 - 1)) == 0) return grid_stride(UPK_NCHW_BWD_POW2, S, n * h * w, 256, xo_stream);
      // tiled: power-of-two input tiles (as feature maps are), region <= 80x80 full-res pixels (~25 KB of LDS, 6 blocks / CU)
      const double sh = (double)H / h, sw = (double)W / w, s = sh > sw ? sh : sw;
      for (int t = 32; t >= 1; t >>= 1) {
        const int rm = (int)((t + 1) * s) + 4;
        const size_t b = sizeof(float) * ((size_t)rm * (rm + 1) + 4 * (size_t)rm + 2 * (size_t)(t + 3) + (size_t)rm * (t + 1));
        if (rm <= 80 && b <= 48 * 1024) {
          p->TI = t, p->RMAX = rm, p->lds = b;
          return chunked(UPK_NCHW_BWD_GENERAL, (w + t - 1) / t, (h + t - 1) / t);
        }
      }
      return SEA_ERR_ARG;  // no tile fits (a factor beyond 38)
    }
    case SEA_UP_NHWC_FWD:  // cells are the default for power-of-two factors (x16 cells: 2 x 16 float4 interpolants per lane)
      if (S == 2 || S == 4 || S == 8) return grid_stride(UPK_NHWC_FWD_CELLS, S, n * (h + 1) * (w + 1) * CG, 256, q.xcd_order);
      return grid_stride(UPK_NHWC_FWD, S == 16 ? 16 : 0, n * H * W * CG, 256 * 2, q.xcd_order);
    case SEA_UP_NHWC_BWD: {
      const int64_t total = n * h * w * CG;
      if (S == 2 || S == 4 || S == 8) return grid_stride(UPK_NHWC_BWD_POW2, S, total, 256, q.xcd_order);
      if (total >= 65536 || n * h * w >= 65536) return grid_stride(UPK_NHWC_BWD_GENERAL, 0, total, 256, q.xcd_order);
      p->kernel = UPK_NHWC_BWD_SMALL, p->total = total;  // one block per coarse pixel x 16 channel groups
      p->grid_x = (int)(n * h * w), p->grid_y = (CG + 15) / 16;
      return 0;
    }
    case SEA_UP_TAP_FWD:  // the kernel indexes inside one image with 32-bit offsets
      if ((int64_t)H * W * CG >= (1ll << 31) || (int64_t)h * w * 9 * CG >= (1ll << 31)) return SEA_ERR_ARG;
      p->nbh = (H + kTapBlock - 1) / kTapBlock, p->nbw = (W + kTapBlock - 1) / kTapBlock;
      return grid_stride(UPK_TAP_FWD, (S == 4 || S == 8) ? S : 0, n * p->nbh * p->nbw * CG, 256, q.xcd_order);
    default: {  // SEA_UP_TAP_BWD
      const bool p2 = S == 4 || S == 8;
      return grid_stride(p2 ? UPK_TAP_BWD_POW2 : UPK_TAP_BWD_GENERAL, p2 ? S : 0, n * h * w * CG, 256, q.xcd_order);
    }
  }
}

}  // namespace sea
