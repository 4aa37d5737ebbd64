// K2: which kernel a call of sea_loss_fwd_bwd runs, with which template parameters and on which grid -- the WHOLE decision,
// as one pure host function.  Plain C++17 without HIP headers: a host compiler builds it alone (tests/test_loss_plan_cpu.py
// sweeps it through sea_loss_plan).  The launchers of loss_kernels.hip / loss_stream.hip / loss_split.hip take a LossPlan
// and decide nothing; `tiles` (the grid's x extent = records per image that loss_finalize sums) is computed here only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sea_hip.h"

#ifndef SEA_ERR_ARG
#define SEA_ERR_ARG 1  // == hipErrorInvalidValue
#endif

namespace sea {
// loss_nchw_reg<T, cpad, vec, grad, exact, tune> | loss_nchw_stream<T, grad> (C > 192, with or without gradient) |
// loss_nchw_fwd<T, ch, waves> (no gradient) | loss_nchw_split<T, C, waves> (gradient, C = 150 / 151) | loss_nhwc_lds<T, grad>
enum K2Kernel { K2_REG, K2_STREAM_GRAD, K2_FWD, K2_SPLIT, K2_NHWC };

struct LossQuery {
  int elem_bytes /* 4 | 2 */, layout, C;
  int64_t HW;
  bool grad;
  uintptr_t logits, dlogits;  // addresses (alignment is all that matters); dlogits is read only under `grad`
  unsigned variant;           // SEA_K2_* word of sea_hip.h, 0 = the shipped choice
};
struct LossPlan {
  int kernel, cpad, exact, vec, tune, ch, waves, tiles;
  size_t lds;  // dynamic LDS bytes (K2_NHWC)
};

// The register kernel's instantiations, per pixels-per-lane: the ONE list.  The tables below and the instantiation switch
// of loss_kernels.hip are both expanded from it.  19, 21 (Cityscapes, VOC) and 150, 151 (ADE) serve only C == that value.
#define SEA_K2_CPADS_VEC4(X, V) X(8, V) X(16, V) X(19, V) X(21, V) X(24, V) X(32, V)
#define SEA_K2_CPADS_VEC2(X, V) SEA_K2_CPADS_VEC4(X, V) X(48, V) X(64, V)
#define SEA_K2_CPADS_VEC1(X, V) SEA_K2_CPADS_VEC2(X, V) X(96, V) X(128, V) X(150, V) X(151, V) X(160, V) X(192, V)
#define SEA_K2_REG_INSTANCES(X) SEA_K2_CPADS_VEC4(X, 4) SEA_K2_CPADS_VEC2(X, 2) SEA_K2_CPADS_VEC1(X, 1)

#define SEA_K2_ENTRY(CP, V) CP,
constexpr int kK2Cpad4[] = {SEA_K2_CPADS_VEC4(SEA_K2_ENTRY, 4)};
constexpr int kK2Cpad2[] = {SEA_K2_CPADS_VEC2(SEA_K2_ENTRY, 2)};
constexpr int kK2Cpad1[] = {SEA_K2_CPADS_VEC1(SEA_K2_ENTRY, 1)};
#undef SEA_K2_ENTRY

template <size_t N>
constexpr int k2_cpad_for(const int (&table)[N], int C) {  // first entry that fits C (0: none)
  for (int e : table)
    if ((e == 19 || e == 21 || e == 150 || e == 151) ? C == e : C <= e) return e;
  return 0;
}

static inline int loss_plan(const LossQuery& q, LossPlan* p) {
  *p = LossPlan{};
  const int eb = q.elem_bytes;
  if ((eb != 4 && eb != 2) || q.C <= 0 || q.HW <= 0) return SEA_ERR_ARG;
  // ---- the word: every field must name something ------------------------------------------------------------------
  const unsigned word = q.variant;
  const unsigned fv = word & SEA_K2_VEC_MASK, tune_w = (word >> SEA_K2_TUNE_SHIFT) & 15u, v = (word >> SEA_K2_STREAM_SHIFT) & 15u;
  const bool reg_only = (word & SEA_K2_REG_ONLY) != 0;
  auto in = [](unsigned x, unsigned set) { return (set >> x) & 1u; };  // set = one bit per allowed value
  if ((word >> 13) || !in(fv, 0x17) || !in(tune_w, 0x80c5) || !in(v, 0x801f)) return SEA_ERR_ARG;
  auto tiles = [&](int64_t px_per_block) {  // records per image; 0 = does not fit the grid
    const int64_t t = (q.HW - 1) / px_per_block + 1;
    return t <= INT32_MAX ? (int)t : 0;
  };
  p->vec = 1;
  if (q.layout == SEA_LAYOUT_NHWC) {
    p->kernel = K2_NHWC;
    p->lds = (size_t)256 * (size_t)(q.C | 1) * sizeof(float);  // odd row stride (in dwords): lanes hit distinct banks
    if (p->lds > 160 * 1024 - 64) return SEA_ERR_ARG;
    return (p->tiles = tiles(256)) ? 0 : SEA_ERR_ARG;
  }
  if (q.layout != SEA_LAYOUT_NCHW) return SEA_ERR_ARG;
  // n pixels per lane: every plane start (b * C + c) * HW + px0 must be aligned to n elements
  auto al = [&](int n) {
    const uintptr_t bytes = (uintptr_t)eb * n;
    return (q.HW % n) == 0 && (q.logits % bytes) == 0 && (!q.grad || (q.dlogits % bytes) == 0);
  };
  // no gradient: beyond 32 classes the class vector no longer fits the registers at a useful occupancy -> streaming kernel.
  // Measured cold (tools/k2_lab.py): C=151 fp32 200 us vs 225 us register kernel, bf16 130 us vs 165 us; at C=21 the register
  // kernel (all 21 plane loads of a lane in flight at once) is as fast (fp32) or faster (16-bit: 28.5 vs 32.7 us) than the
  // chunk pipeline, which pays one memory round trip per chunk.
  const int v16 = 16 / eb;
  if (!reg_only && !q.grad && fv == 0 && al(v16) && (q.C > 32 || v != 0)) {
    p->kernel = K2_FWD;
    p->vec = v16;
    constexpr int kChunk[5] = {4, 4, 8, 6, 2}, kWaves[5] = {0, 5, 3, 4, 8};  // by v; the default: CH = 4 at 5 waves (fp32, 93
    p->ch = kChunk[v % 15], p->waves = v % 15 ? kWaves[v] : (eb == 4 ? 5 : 4);  // VGPRs) / 4 waves (16-bit, 8 px per lane: 127)
    return (p->tiles = tiles(256 * v16)) ? 0 : SEA_ERR_ARG;
  }
  // ADE-sized class vectors with gradient: split over the wave halves, one 32-bit word (ppw pixels) per lane and plane,
  // 32-bit lane offsets.  Waves per SIMD asked of the compiler, measured cold (tools/k2_lab.py, 8 x 151 x 512 x 512): fp32
  // 4 waves 464 us (3: 464, 5: 470; register kernel 485); bf16 3 waves 256 us (4 and 5 spill: 430 / 551 us; register 293).
  const int ppw = 4 / eb;
  if (!reg_only && q.grad && fv == 0 && v != 15 && (q.C == 150 || q.C == 151) && (q.HW % ppw) == 0 &&
      ((q.logits | q.dlogits) & 3) == 0 && q.HW <= (((int64_t)1 << 31) - 1) / ((int64_t)q.C * eb)) {
    if (v != 0) return SEA_ERR_ARG;  // a streaming variant names no gradient kernel
    p->kernel = K2_SPLIT;
    p->cpad = q.C, p->exact = 1, p->vec = ppw, p->waves = eb == 4 ? 4 : 3;
    return (p->tiles = tiles(128 * ppw)) ? 0 : SEA_ERR_ARG;
  }
  // register kernel: the widest allowed pixels-per-lane whose table holds C
  if (al(4) && (fv == 0 || fv == 4) && (p->cpad = k2_cpad_for(kK2Cpad4, q.C)))
    p->vec = 4;
  else if (al(2) && fv != 1 && (p->cpad = k2_cpad_for(kK2Cpad2, q.C)))
    p->vec = 2;
  else
    p->cpad = k2_cpad_for(kK2Cpad1, q.C);
  p->kernel = p->cpad ? K2_REG : K2_STREAM_GRAD;
  p->exact = q.C == p->cpad;
  // TUNE (bit 0: non-temporal gradient stores, bit 1: non-temporal logit loads, bit 2: 4 waves/SIMD) exists in three fp32
  // cells, each with its measured winner (kernel_bench, MI355X): C=21 with gradient nt loads + stores at 4 waves/SIMD (74 %
  // of 8 TB/s vs 65 %), C=151 with gradient nt loads (69 % vs 67.6 %), C=21 without gradient nt loads at 4 waves/SIMD.
  // The winner is the default of a word without vec / TUNE / stream field; 15 = explicitly none.  Elsewhere TUNE is ignored.
  const int cell = (eb != 4 || p->kernel != K2_REG) ? 0
                   : (q.C == 21 && p->vec == 4)     ? (q.grad ? 7 : 6)
                   : (q.C == 151 && q.grad)         ? 2
                                                    : 0;
  if (cell && ((word & 0xfffu) == 0 || tune_w == (unsigned)cell))
    p->tune = cell;
  else if (cell && tune_w != 0 && tune_w != 15)
    return SEA_ERR_ARG;
  return (p->tiles = tiles(256 * p->vec)) ? 0 : SEA_ERR_ARG;
}

}  // namespace sea
