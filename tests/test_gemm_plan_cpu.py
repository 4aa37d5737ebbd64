"""M8's selection plan (csrc/gemm_plan.h through sea_gemm_plan / _native.gemm_plan): which kernel a sea_gemm_split* call runs,
with which template parameters, grid and LDS bytes, without a device.

(a) pins rows of the map; (b) sweeps the plan against ``_dispatch_before_the_plan``, a transcription of the dispatch as it
stood before the plan existed (gemm_split_impl trying launchers that could refuse); (c) asserts on every successful plan of
the sweep what a launch depends on; (d) the header is plain host C++.

How the pinned rows follow from that dispatch (t128 = ceil(M/128) * ceil(N/128) * batch; t256 = ceil(M/256) * (N/256) * batch
where N % 256 == 0, else 0; t384 = ceil(M/128) * (N/384) * batch where N % 384 == 0, else 0; r2 / r3 = t128 rounded up to
512 / 768; default word = pipe 2; all with 32x32 fragments, terms 22 or 2, no fused epilogue unless stated):
  * 36 x 8192 x 512 x 512 (Winograd product): t256 = 32 * 2 * 36 = 2304 >= 1024, no prologue, M >= 256 -> 256 x 256 tiles,
    512 threads, depth 1 (its only instantiation), LDS 2 * 64 KB + 2 * 256 floats = 133120, grid 2304 (a multiple of 8).
  * 8192 x 1536 x 384: 1536 % 256 == 0 but t256 = 32 * 6 = 192 < 1024; t384 = 64 * 4 = 256 in [192, 256] and K >= 192 ->
    128 x 384 tiles, LDS 2 * 64 KB + 2 * 128 floats = 132096; depth 2, but 1 with the prologues that read a second operand
    (1, 3).  Batch 4 of 8192 x 384 x 384 (the slices of a split-K product): t384 = 64 * 1 * 4 = 256, the same.
  * 8192 x 1536 x 96: K < 192 closes the 128 x 384 window; no prologue -> single-stage, t128 = 64 * 12 = 768 tiles.  With
    prologue 1: r2 = 1024 > r3 = 768 -> still single-stage.  8192 x 2048 x 96 with prologue 1: t128 = 1024 = r2 <= r3 = 1536
    -> ping-pong (t256 = 256 < 1024 and a prologue: no 256 x 256; 2048 % 384 != 0).
  * 300 x 200 x 96: t128 = 3 * 2 = 6, r2 = 512 <= r3 = 768: ping-pong with a prologue (LDS 2 stages * 2 operands * 2 terms *
    8 KB + 1 KB of row scales = 66560; depth 1 for prologue 3), single-stage (LDS 0) without.
  * a fused epilogue excludes the one-block-per-CU kernels and is no prologue -> single-stage with EPI; pipe=1 -> ping-pong
    with EPI, depth 2.
  * three terms: the ping-pong launcher refused them and the one-block-per-CU kernels never took them -> single-stage for
    every pipe; prologues 1 / 3 are an invalid argument (SEA_CHECK_ARG in the three-term branch).
  * mfma_shape=16 skipped both attempts -> single-stage with S16 for every pipe.
  * pipe=3, N = 768 (t384 != 0 rules the 256 x 256 tiles out): M = 1000 -> 128 x 384; M = 100 < 128 -> neither, and pipe 3 is
    not ping-pong -> single-stage.
  * ldc = 2^28: both the one-block-per-CU and the ping-pong launcher refused (32-bit offsets into C) -> single-stage.
  * lda = 2^22 (needs M * lda < 2^30, so M < 256): the one-block-per-CU launcher refused.  128 x 384 x 192 with prologue 3:
    pipe=3 -> 128 x 384 tiles at lda = K, single-stage at lda = 2^22; default word -> ping-pong (t128 = 3) either way; batch
    192 of it (t384 = 192): 128 x 384 tiles at lda = K, and single-stage at lda = 2^22 since r2 = 1024 > r3 = 768.  (Under the
    default word a shape in the 128 x 384 window has t128 = 3 * t384 in [576, 768]: never a ping-pong grid.)
"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

@pytest.fixture(scope="module")
def native():
    from semseg import _native
    if not os.path.exists(_native.LIB_PATH):
        import sys
        sys.path.insert(0, PKG)
        import build_native
        build_native.build(verbose=False)
    return _native


def _ceil(a, b):
    return -(-a // b)


def _has(plan, **want):
    assert plan["rc"] == 0, plan
    got = {k: plan[k] for k in want}
    assert got == want, plan


# ------------------------------------------------------------------------------------------------ (a) the pinned rows
def test_one_block_per_cu_rows(native):
    P = native.gemm_plan
    _has(P(8192, 512, 512, 22, batch=36), kernel="big256", terms_t=2, f16=True, s16=False, epi=False, pro=0, depth=1, bm=256, bn=256,
         mblocks=32, nblocks=2, tiles=2304, grid=2304, threads=512, lds=133120)
    _has(P(8192, 512, 512, 2, batch=36), kernel="big256", terms_t=2, f16=False, depth=1, tiles=2304)
    _has(P(8192, 1536, 384, 22), kernel="big384", pro=0, depth=2, bm=128, bn=384, mblocks=64, nblocks=4, tiles=256, grid=256,
         threads=512, lds=132096)
    for pro, depth in ((1, 1), (2, 2), (3, 1)):
        _has(P(8192, 1536, 384, 22, prologue=pro), kernel="big384", pro=pro, depth=depth, tiles=256, lds=132096)
    _has(P(8192, 384, 384, 22, batch=4, prologue=2), kernel="big384", pro=2, depth=2, nblocks=1, tiles=256)
    # K < 192
    _has(P(8192, 1536, 96, 22), kernel="single", tiles=768, grid=768, threads=256, lds=0, depth=0)
    _has(P(8192, 1536, 96, 22, prologue=1), kernel="single", pro=1, tiles=768)
    _has(P(8192, 2048, 96, 22, prologue=1), kernel="pp", pro=1, depth=1, tiles=1024)
    # pipe=3 at N = 768
    _has(P(1000, 768, 96, 22, pipe=3), kernel="big384", mblocks=8, nblocks=2, tiles=16, grid=16)
    _has(P(100, 768, 96, 22, pipe=3), kernel="single", tiles=6, grid=8)
    _has(P(1000, 512, 96, 22, pipe=3), kernel="big256", mblocks=4, nblocks=2, tiles=8)
    _has(P(1000, 512, 96, 22, pipe=3, prologue=2), kernel="single")          # 256 x 256 tiles have no prologue
    _has(P(1000, 512, 96, 22), kernel="single")                              # default word: 8 tiles are not 1024


def test_pingpong_and_single_rows(native):
    P = native.gemm_plan
    _has(P(300, 200, 96, 22, prologue=3), kernel="pp", terms_t=2, f16=True, epi=False, pro=3, depth=1, bm=128, bn=128, npad=256,
         mblocks=3, nblocks=2, tiles=6, grid=8, threads=256, lds=66560)
    _has(P(300, 200, 96, 22), kernel="single", pro=0, tiles=6, grid=8, threads=256, lds=0)
    _has(P(300, 200, 96, 2, prologue=2), kernel="pp", f16=False, depth=2, lds=65536)
    _has(P(300, 200, 96, 1, pipe=1), kernel="pp", terms_t=1, depth=2, lds=32768)
    _has(P(300, 200, 96, 22, fused=True), kernel="single", epi=True, pro=0)
    _has(P(300, 200, 96, 22, fused=True, pipe=1), kernel="pp", epi=True, pro=0, depth=2)
    _has(P(8192, 1536, 384, 22, fused=True), kernel="single", epi=True)      # no epilogue extras in the one-block-per-CU kernels
    for pipe in (0, 1, 2, 3):
        _has(P(300, 200, 96, 3, pipe=pipe), kernel="single", terms_t=3, f16=False)
        _has(P(300, 200, 96, 3, pipe=pipe, prologue=2), kernel="single", terms_t=3, pro=2)
        assert P(300, 200, 96, 3, pipe=pipe, prologue=1)["rc"] == 1 and P(300, 200, 96, 3, pipe=pipe, prologue=3)["rc"] == 1
        for shape in ((8192, 512, 512, 22, 36), (8192, 1536, 384, 22, 1), (300, 200, 96, 2, 1)):
            _has(P(*shape[:4], batch=shape[4], pipe=pipe, mfma_shape=16), kernel="single", s16=True, lds=0)


def test_stride_limits_choose_the_single_stage_kernel(native):
    P = native.gemm_plan
    for shape, kw, kernel in (((8192, 512, 512, 22), dict(batch=36), "big256"), ((8192, 1536, 384, 22), {}, "big384"),
                              ((300, 200, 96, 22), dict(prologue=3), "pp"), ((300, 200, 96, 22), dict(pipe=1), "pp")):
        _has(P(*shape, ldc=(1 << 28) - 1, **kw), kernel=kernel)
        _has(P(*shape, ldc=1 << 28, **kw), kernel="single")
    _has(P(300, 200, 96, 22, fused=True, pipe=1, ld_add=(1 << 28) - 1), kernel="pp")
    _has(P(300, 200, 96, 22, fused=True, pipe=1, ld_add=1 << 28), kernel="single", epi=True)
    # lda = 2^22
    for lda, kernels in ((192, ("big384", "pp", "big384")), ((1 << 22) - 4, ("big384", "pp", "big384")), (1 << 22, ("single", "pp", "single"))):
        _has(P(128, 384, 192, 22, lda=lda, prologue=3, pipe=3), kernel=kernels[0])
        _has(P(128, 384, 192, 22, lda=lda, prologue=3), kernel=kernels[1], tiles=3)
        _has(P(128, 384, 192, 22, lda=lda, prologue=3, batch=192), kernel=kernels[2])


def test_invalid_arguments(native):
    P, L = native.gemm_plan, native.lib()
    out = (ctypes.c_int32 * 16)()
    for word in (8, 9, 16, 0x100, 1 << 31):
        assert L.sea_gemm_plan(300, 200, 96, 22, 1, 96, 200, 0, 0, 0, word, out) == 1
    for word in range(8):
        assert L.sea_gemm_plan(300, 200, 96, 22, 1, 96, 200, 0, 0, 0, word, out) == 0
    assert L.sea_gemm_plan(300, 200, 96, 22, 1, 96, 200, 0, 0, 0, 0, None) == 1
    assert P(300, 200, 48, 22)["rc"] == 1 and P(0, 200, 96, 22)["rc"] == 1 and P(300, 0, 96, 22)["rc"] == 1
    assert P(300, 200, 0, 22)["rc"] == 1 and P(300, 200, 96, 22, batch=0)["rc"] == 1
    assert P(300, 200, 96, 4)["rc"] == 1 and P(300, 200, 96, 0)["rc"] == 1
    assert P(300, 200, 96, 22, lda=92)["rc"] == 1 and P(300, 200, 96, 22, lda=98)["rc"] == 1 and P(300, 200, 96, 22, ldc=199)["rc"] == 1
    assert P(256, 200, 96, 22, lda=1 << 22)["rc"] == 1                       # M * lda < 2^30
    assert P(1 << 24, 1 << 20, 32, 22)["rc"] == 1                            # 2^17 * 2^13 = 2^30 tiles of 128 x 128
    assert P(1 << 22, 1 << 15, 32, 22, batch=128)["rc"] == 1 and P(1 << 22, 1 << 15, 32, 22, batch=127)["rc"] == 0
    assert P(300, 200, 96, 22, prologue=4)["rc"] == 1 and P(300, 200, 96, 22, prologue=-1)["rc"] == 1
    for pro in (1, 2, 3):
        assert P(300, 200, 96, 22, prologue=pro, fused=True)["rc"] == 1      # prologue and epilogue extras are exclusive
    assert P(2 ** 31 - 1, 128, 32, 22)["rc"] == 1 and P(1, 2 ** 31 - 1, 32, 22)["rc"] == 1


def test_plan_header_is_plain_host_cxx():
    """csrc/gemm_plan.h is C++17 for any host compiler: no HIP header, no device code"""
    path = os.path.join(PKG, "csrc", "gemm_plan.h")
    text = open(path).read()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text
    assert re.findall(r'#include [<"]([^>"]+)[>"]', text) == ["stddef.h", "stdint.h", "../../include/sea_hip.h"]
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    cmd = [cxx] if cxx else [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-nogpuinc", "-nogpulib"]
    subprocess.run(cmd + ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(path), "-x", "c++", "-"],
                   input='#include "gemm_plan.h"\nint main() { sea::GemmPlan p; return sea::gemm_plan(sea::GemmQuery{}, &p); }\n',
                   text=True, check=True)
    header = open(os.path.join(ROOT, "include", "sea_hip.h")).read()
    assert "int sea_gemm_plan(" in header and "csrc/gemm_plan.h" in header


# ------------------------------------------------------------------------------------------------ (b), (c) the sweep
def _dispatch_before_the_plan(M, N, K, terms, batch, lda, ldc, ld_add, pro, fused, word):
    """The dispatch as it stood before gemm_plan.h, statement by statement: the entry points' term check, gemm_split_impl, and
    the refusal conditions of gemm_split_big_launch / gemm_split_pp_launch.  None = SEA_ERR_ARG, else (kernel, terms_t, f16,
    s16, epi, pro, depth, bm, bn, mblocks, nblocks, tiles, grid)."""
    if terms not in (1, 2, 3, 22):                                           # sea_gemm_split / _fused (sea_gemm_split_f16: 22)
        return None
    if word & ~7:
        return None
    if not (M > 0 and N > 0 and K > 0 and K % 32 == 0 and batch > 0):
        return None
    if not (lda >= K and ldc >= N and lda % 4 == 0 and M * lda < 1 << 30):
        return None
    npad = _ceil(N, 128) * 128
    mblocks, nblocks = _ceil(M, 128), npad // 128
    total = mblocks * nblocks * batch
    if not total < 1 << 30:
        return None
    shape16 = bool(word & 4)
    if pro and fused:                                                        # a_gelu / a_gelu_grad_of against the epilogue extras
        return None
    if pro in (1, 3) and terms not in (1, 2, 22):
        return None
    pipe = {1: 0, 2: 1, 3: 3, 0: 2}[word & 3]
    f16 = terms == 22

    def big_launch(shape, pro):
        BM, BN = (128, 384) if shape else (256, 256)
        if ldc >= 1 << 28 or lda >= 1 << 22 or N % BN or npad < N or npad % 128 or (shape == 0 and pro != 0):
            return None
        if npad % BN:
            return None
        mb, nb = _ceil(M, BM), N // BN
        tot = mb * nb * batch
        if tot >= 1 << 30:
            return None
        depth = 1 if shape == 0 else {0: 2, 1: 1, 2: 2, 3: 1}[pro]
        return (2 + shape, 2, f16, False, False, pro, depth, BM, BN, mb, nb, tot, _ceil(tot, 8) * 8)

    def pp_launch():
        if ldc >= 1 << 28 or ld_add >= 1 << 28:
            return None
        if terms not in (22, 2, 1):
            return None
        depth = {2: 2, 1: 1, 3: 1}.get(pro, 2)
        return (1, 2 if f16 else terms, f16, False, bool(fused) and pro == 0, pro, depth, 128, 128, mblocks, nblocks, total,
                _ceil(total, 8) * 8)

    if not shape16 and terms in (22, 2) and not fused and pipe in (2, 3):
        t256 = _ceil(M, 256) * (N // 256) * batch if N % 256 == 0 else 0
        t384 = _ceil(M, 128) * (N // 384) * batch if N % 384 == 0 else 0
        if pro == 0 and M >= 256 and t256 > 0 and (t384 == 0 if pipe == 3 else t256 >= 1024):
            r = big_launch(0, 0)
            if r:
                return r
        wide_fits = 192 <= t384 <= 256 and K >= 192
        if t384 > 0 and M >= 128 and (pipe == 3 or wide_fits):
            r = big_launch(1, pro)
            if r:
                return r
    r2, r3 = _ceil(total, 512) * 512, _ceil(total, 768) * 768
    pingpong = pipe == 1 or (pipe == 2 and pro != 0 and r2 <= r3)
    if not shape16 and terms != 3 and pingpong:
        r = pp_launch()
        if r:
            return r
    if terms == 3 and pro not in (0, 2):
        return None
    epi = pro == 0 and bool(fused)                                           # SEA_GS_PRO: the prologues first, then `fused`
    return (0, 2 if f16 else terms, f16, shape16, epi, pro, 0, 128, 128, mblocks, nblocks, total, _ceil(total, 8) * 8)


SWEEP_M = (1, 128, 256, 1000, 8192)
SWEEP_N = (1, 200, 256, 384, 768, 1536, 2048)
SWEEP_K = (96, 192, 48)
SWEEP_TERMS = (1, 2, 3, 22)
SWEEP_BATCH = (1, 4, 36)
SWEEP_MODES = ((0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (2, 1))               # (prologue, fused)
SWEEP_WORDS = tuple(range(8))


def _sweep_strides(N, K):                                                    # (lda, ldc, ld_add) around the 2^22 / 2^28 limits
    return ((K, N, 0), (K + 4, N + 1, N + 1), ((1 << 22) - 4, N, 0), (1 << 22, N, 0), (K, (1 << 28) - 1, 0),
            (K, 1 << 28, 0), (K, N, (1 << 28) - 1), (K, N, 1 << 28))


def test_sweep_agrees_with_the_dispatch_before_the_plan(native):
    plan = native.lib().sea_gemm_plan
    out = (ctypes.c_int32 * 16)()
    n, seen = 0, set()
    for M in SWEEP_M:
        for N in SWEEP_N:
            for K in SWEEP_K:
                for lda, ldc, ld_add in _sweep_strides(N, K):
                    for terms in SWEEP_TERMS:
                        for batch in SWEEP_BATCH:
                            for pro, fused in SWEEP_MODES:
                                for word in SWEEP_WORDS:
                                    want = _dispatch_before_the_plan(M, N, K, terms, batch, lda, ldc, ld_add, pro, fused, word)
                                    rc = plan(M, N, K, terms, batch, lda, ldc, ld_add, pro, fused, word, out)
                                    n += 1
                                    got = out[:]
                                    where = (M, N, K, terms, batch, lda, ldc, ld_add, pro, fused, word, got, want)
                                    assert rc == (want is None), where       # 0 | 1; word 0 never fails where it did not
                                    if rc:
                                        continue
                                    kernel, terms_t, f16, s16, epi, pro_t, depth, bm, bn, npad, mblocks, nblocks, tiles, grid, threads, lds = got
                                    assert tuple(got[:9] + got[10:14]) == want, where
                                    # (c) what every launch depends on
                                    assert (npad >= N and npad % 128 == 0 and npad % bn == 0 and nblocks * bn <= npad
                                            and mblocks * bm >= M and nblocks * bn >= N
                                            and mblocks * nblocks * batch == tiles >= 1
                                            and grid % 8 == 0 and tiles <= grid < tiles + 8
                                            and threads == (512 if kernel >= 2 else 256)
                                            and lds == (0, 4 * terms_t * 8192 + 1024 * f16, 133120, 132096)[kernel] <= 160 * 1024
                                            and (ldc < 1 << 28 or kernel == 0)), where
                                    seen.add(tuple(got[:7]))
    assert n == (len(SWEEP_M) * len(SWEEP_N) * len(SWEEP_K) * 8 * len(SWEEP_TERMS) * len(SWEEP_BATCH) * len(SWEEP_MODES)
                 * len(SWEEP_WORDS)) == 483840
    # every instantiation of the three launch switches is reached: 2 * (3 * 5 + 3) single-stage, 3 * 5 ping-pong, 2 * 5 big
    assert len(seen) == 36 + 15 + 10 and {s[0] for s in seen} == {0, 1, 2, 3}
