// M8: which kernel a call of sea_gemm_split* runs, with which template parameters, on which grid and with how much LDS -- the
// WHOLE decision, as one pure host function.  Plain C++17 without HIP headers: a host compiler builds it alone
// (tests/test_gemm_plan_cpu.py sweeps it through sea_gemm_plan).  The launchers of gemm_split.hip / gemm_split_pp.hip /
// gemm_split_big.hip take a GemmPlan and decide nothing; the limits that make a kernel inapplicable are stated here only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sea_hip.h"

#ifndef SEA_ERR_ARG
#define SEA_ERR_ARG 1  // == hipErrorInvalidValue
#endif

namespace sea {
// gemm_split_kernel<TERMS, S16, F16, EPI, PRO> (128 x 128 tiles, three blocks per CU) | gemm_split_pp_kernel<TERMS, F16, EPI,
// PRO, DEPTH> (128 x 128, two LDS stages, two blocks per CU) | gemm_split_big_kernel<F16, WM, WN, TN, PRO, DEPTH>: 256 x 256
// tiles (waves 4 x 2) and 128 x 384 tiles (waves 2 x 4), one block of 512 threads per CU
enum GemmKernel { GEMM_SINGLE, GEMM_PP, GEMM_BIG256, GEMM_BIG384 };

struct GemmQuery {
  int M, N, K, terms /* 1 | 2 | 3 bf16 terms, 22 = fp16 x 2 */, batch;
  int64_t lda, ldc, ld_add;  // ld_add: SeaGemmEpilogue.ld_addend as passed (0 without epilogue block)
  int pro;                   // prologue on A: 0 none, 1 A * GELU'(t), 2 GELU(A), 3 ReLU gate
  bool fused;                // epilogue extras: addend | gelu_out | gelu_grad_of
  unsigned variant;          // SEA_GEMM_* word of sea_hip.h, 0 = the shipped choice
};
struct GemmPlan {
  int kernel, terms_t /* TERMS: 1 | 2 | 3 */, f16, s16, epi, pro, depth;
  int bm, bn, npad, mblocks, nblocks, tiles, grid /* blocks: tiles rounded up to the 8 XCDs */, threads;
  size_t lds;  // dynamic LDS bytes
};

// Smallest tile count for the 128 x 384 kernel: one round of one block per CU has to be at least three quarters full
// (profiles/r5_gemm_wide_ab.md).
constexpr int kGemmWideMin = 192;

// The `variant` word (include/sea_hip.h): 0 = the shipped dispatch.  Bits 0-1 force a K-loop kernel, bit 2 the 16x16x32
// fragments.  The kernels of every pipeline give the SAME BITS (same split, same MFMA order); the two fragment shapes differ in
// the last bits (summation order).
//   pipe 0 = the single-stage loop (32 KB of LDS, three blocks per CU), 1 = ping-pong (two LDS stages, one barrier per K step,
//   the split in the MFMA shadow, loads two K steps ahead; two blocks per CU), 2 = per launch (shipped): the one-block-per-CU
//   kernels and the ping-pong loop where they win IN the attack loop (below), 3 = the one-block-per-CU kernels wherever
//   they apply.
constexpr int gemm_variant_pipe(unsigned variant) {
  switch (variant & SEA_GEMM_PIPE_MASK) {
    case SEA_GEMM_PIPE_SINGLE: return 0;
    case SEA_GEMM_PIPE_PINGPONG: return 1;
    case SEA_GEMM_PIPE_BIG: return 3;
    default: return 2;
  }
}

static inline int gemm_plan(const GemmQuery& q, GemmPlan* p) {
  *p = GemmPlan{};
  const int M = q.M, N = q.N, K = q.K, terms = q.terms, pro = q.pro;
  // ---- arguments: the word, the shape, the strides, which extras go together ---------------------------------------
  if ((q.variant & ~(unsigned)(SEA_GEMM_PIPE_MASK | SEA_GEMM_SHAPE16)) != 0) return SEA_ERR_ARG;
  if (terms != 1 && terms != 2 && terms != 3 && terms != 22) return SEA_ERR_ARG;
  if (M <= 0 || N <= 0 || K <= 0 || (K % 32) != 0 || q.batch <= 0) return SEA_ERR_ARG;
  // M * lda < 2^30 (32-bit lane offsets into A), written without the product: any int64 stride is an answer, not an overflow
  if (q.lda < K || q.ldc < N || (q.lda % 4) != 0 || q.lda > ((1ll << 30) - 1) / M) return SEA_ERR_ARG;
  // a prologue excludes the epilogue extras; the prologues with a second operand (1, 3) exist for one or two terms only
  if (pro < 0 || pro > 3 || (pro != 0 && q.fused) || (terms == 3 && (pro == 1 || pro == 3))) return SEA_ERR_ARG;
  const int64_t npad = ((int64_t)N + 127) / 128 * 128;  // rows of the packed weight image
  const int64_t mb128 = (M + 127) / 128, t128 = mb128 * (npad / 128);
  if (npad > INT32_MAX || t128 >= (1ll << 30) || t128 * q.batch >= (1ll << 30)) return SEA_ERR_ARG;  // (128 x 128 tiles bound the others)
  const int64_t total = t128 * q.batch;

  // ---- which kernel -------------------------------------------------------------------------------------------------
  // MFMA shape: 32x32x16 fragments (default) or 16x16x32 (SEA_GEMM_SHAPE16, single-stage loop only): the chip holds a higher
  // clock on the small shape in MFMA-dense loops (MI355X guide, DVFS give-back item 7); which one wins is measured IN the attack
  // loop, where the clock is the limiter (profiles/r4_rejected_experiments.md: +3.6 % per step on the small shape)
  const bool s16 = (q.variant & SEA_GEMM_SHAPE16) != 0;
  const int pipe = gemm_variant_pipe(q.variant);
  const bool c32 = q.ldc < (1ll << 28);  // the ping-pong and one-block-per-CU epilogues keep 32-bit lane offsets into C
  int kernel = GEMM_SINGLE;
  // One-block-per-CU kernels for the products that are bound by the bytes a CU pulls through its L1: two terms, no epilogue
  // extras, 32-bit offsets into A rows (lda < 2^22).  pipe 3 forces them wherever they apply; pipe 2 takes 256 x 256 tiles
  // from 1024 tiles on (the Winograd-domain products) and 128 x 384 tiles where they fill the chip in whole rounds (256 CUs: the
  // 32 x 32-pixel stage's M = 8192 products).  N % BN == 0 makes the packed image end on a tile (npad == N).
  if (!s16 && (terms == 22 || terms == 2) && !q.fused && (pipe == 2 || pipe == 3) && c32 && q.lda < (1ll << 22)) {
    const int64_t t256 = (N % 256) == 0 ? (int64_t)((M + 255) / 256) * (N / 256) * q.batch : 0;
    const int64_t t384 = (N % 384) == 0 ? mb128 * (N / 384) * q.batch : 0;
    // (one round of one block per CU: measured in the loop -- 39 / 48 / 45 us against 41 / 61 / 50 us for the plain / GELU' /
    // GELU launches of the M = 8192 products; on two or more rounds the 128 x 128 kernels win, profiles/r5_gemm_wide_ab.md)
    const bool wide_fits = t384 >= kGemmWideMin && t384 <= 256 && K >= 192;
    if (pro == 0 && M >= 256 && t256 > 0 && (pipe == 3 ? t384 == 0 : t256 >= 1024))
      kernel = GEMM_BIG256;
    else if (t384 > 0 && M >= 128 && (pipe == 3 || wide_fits))
      kernel = GEMM_BIG384;
  }
  // per launch (pipe 2): the ping-pong kernel where it wins IN the attack loop (profiles/r5_gemm_pipe_ab.md): a VALU-heavy
  // prologue (GELU / GELU' / gate on A: hidden in its MFMA shadow) on a grid that fills two blocks per CU at least as
  // well as three (768 tiles are one round of three blocks per CU but one and a half of two).  Three bf16 terms keep the
  // single-stage kernel (96 KB of stages), whatever the word asks for.
  const int64_t r2 = (total + 511) / 512 * 512, r3 = (total + 767) / 768 * 768;
  if (kernel == GEMM_SINGLE && !s16 && terms != 3 && c32 && q.ld_add < (1ll << 28) &&
      (pipe == 1 || (pipe == 2 && pro != 0 && r2 <= r3)))
    kernel = GEMM_PP;

  // ---- template parameters, geometry ----------------------------------------------------------------------------------
  p->kernel = kernel;
  p->terms_t = terms == 22 ? 2 : terms;
  p->f16 = terms == 22;
  p->s16 = s16;
  p->epi = q.fused;
  p->pro = pro;
  // register sets of staged loads: the prologues with a second operand keep one (two would not fit 256 VGPRs next to 64
  // accumulators), and so do the 256 x 256 tiles (128 accumulators)
  p->depth = kernel == GEMM_SINGLE ? 0 : (kernel == GEMM_BIG256 || pro == 1 || pro == 3) ? 1 : 2;
  p->bm = kernel == GEMM_BIG256 ? 256 : 128;
  p->bn = kernel == GEMM_BIG256 ? 256 : kernel == GEMM_BIG384 ? 384 : 128;
  p->npad = (int)npad;
  p->mblocks = (M + p->bm - 1) / p->bm;
  p->nblocks = p->npad / p->bn;
  p->tiles = (int)((int64_t)p->mblocks * p->nblocks * q.batch);
  p->grid = (p->tiles + 7) / 8 * 8;
  p->threads = kernel >= GEMM_BIG256 ? 512 : 256;
  // two stages of A and W term images (+ the tile's row scales and their inverses: fp16 x 2 only in the ping-pong kernel)
  p->lds = kernel == GEMM_SINGLE   ? 0
           : kernel == GEMM_PP     ? (size_t)2 * 2 * p->terms_t * 8192 + (p->f16 ? 1024 : 0)
           : kernel == GEMM_BIG256 ? (size_t)131072 + 2048
                                   : (size_t)131072 + 1024;
  return 0;
}

}  // namespace sea
