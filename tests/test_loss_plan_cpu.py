"""K2's selection plan (csrc/loss_plan.h through sea_loss_plan / _native.loss_plan): which kernel a call runs, without a device.

(a) pins the map from (dtype, layout, C, H*W, gradient, alignment, variant word) to kernel and template parameters -- the map
the docstring of test_loss_nograd_gpu.py relies on -- and that a word which names no kernel is an invalid argument (1);
(b) sweeps the plan and asserts what every launch depends on: the return is 0 or 1; the tile count (grid x = records that
loss_finalize / K7 read) fits the workspace of sea_loss_workspace_bytes; the register kernel has C <= CPAD and EXACT only at
C == CPAD; the chosen pixels-per-lane divides H*W and both pointers are aligned to it; the default word never fails in NCHW.

"al(n)" below: H*W % n == 0 and the logits pointer (and the gradient pointer, if any) is a multiple of n * elem_bytes.
An address that is not a multiple of the element size itself is no tensor of that dtype; the library has always run such a
call at one pixel per lane rather than refuse it, so for those combinations of the sweep (fp32 at a 2-byte offset) the
alignment invariant reads "vec == 1" -- nothing wider may be chosen -- and word 0 still never fails.
"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import PKG, ROOT

F32, BF16 = torch.float32, torch.bfloat16
NCHW, NHWC = 0, 1
EVEN, ODD = 48 * 52, 47 * 53


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
def test_voc_register_kernel_and_its_tune(native):
    P = native.loss_plan
    _has(P(F32, NCHW, 21, EVEN, True), kernel="reg", cpad=21, exact=True, vec=4, tune=7, tiles=_ceil(EVEN, 1024))
    _has(P(F32, NCHW, 21, EVEN, False), kernel="reg", cpad=21, exact=True, vec=4, tune=6)
    _has(P(F32, NCHW, 21, EVEN, False, variant=4), kernel="reg", cpad=21, vec=4, tune=0)
    _has(P(F32, NCHW, 21, EVEN, True, variant=native.k2_variant(vec=4, tune=7)), kernel="reg", vec=4, tune=7)
    _has(P(F32, NCHW, 21, EVEN, True, variant=native.k2_variant(tune=15)), kernel="reg", vec=4, tune=0)
    for grad in (True, False):
        _has(P(F32, NCHW, 21, ODD, grad), kernel="reg", cpad=21, vec=1, tune=0, tiles=_ceil(ODD, 256))
        _has(P(BF16, NCHW, 21, EVEN, grad), kernel="reg", cpad=21, vec=4, tune=0)   # TUNE is fp32 only
    # pixels per lane: the word, then alignment (fp32: 16 / 8 bytes on both pointers)
    _has(P(F32, NCHW, 21, EVEN, True, variant=2), cpad=21, vec=2, tune=0)
    _has(P(F32, NCHW, 21, EVEN, True, variant=1), cpad=21, vec=1, tune=0)
    _has(P(F32, NCHW, 21, EVEN, True, 0, 8), cpad=21, vec=2, tune=0)
    _has(P(F32, NCHW, 21, EVEN, True, 4, 0), cpad=21, vec=1, tune=0)
    _has(P(F32, NCHW, 21, EVEN, False, 0, 4), cpad=21, vec=4, tune=6)               # no gradient: its pointer is not read


def test_cpad_tables(native):
    P = native.loss_plan
    first = {4: [(8, 8), (9, 16), (16, 16), (17, 24), (19, 19), (20, 24), (21, 21), (22, 24), (25, 32), (32, 32)],
             2: [(33, 48), (48, 48), (49, 64), (64, 64)],
             1: [(65, 96), (97, 128), (129, 160), (149, 160), (150, 150), (151, 151), (152, 160), (161, 192), (192, 192)]}
    for vec, rows in first.items():
        for C, cpad in rows:
            _has(P(F32, NCHW, C, EVEN, True, variant=native.k2_variant(stream=15)), kernel="reg", cpad=cpad, exact=C == cpad,
                 vec=vec, tiles=_ceil(EVEN, 256 * vec))
    _has(P(F32, NCHW, 37, EVEN, True, 8, 8), kernel="reg", cpad=48, exact=False, vec=2)    # al(2) only
    _has(P(F32, NCHW, 37, EVEN, True), kernel="reg", cpad=48, vec=2)                       # al(4): no 4-pixel kernel above 32
    _has(P(F32, NCHW, 64, EVEN, True, variant=4), cpad=64, vec=2)
    _has(P(F32, NCHW, 21, EVEN, False, variant=1), cpad=21, vec=1)
    for grad in (True, False):
        _has(P(F32, NCHW, 200, ODD, grad), kernel="stream_grad", vec=1, tiles=_ceil(ODD, 256))
    _has(P(F32, NCHW, 200, EVEN, True), kernel="stream_grad", vec=1, tiles=_ceil(EVEN, 256))
    _has(P(F32, NCHW, 32767, EVEN, True), kernel="stream_grad")


def test_ade_split_kernel(native):
    P = native.loss_plan
    for C in (150, 151):
        _has(P(F32, NCHW, C, EVEN, True), kernel="split", cpad=C, waves=4, vec=1, tiles=_ceil(EVEN, 128))
        _has(P(BF16, NCHW, C, EVEN, True), kernel="split", cpad=C, waves=3, vec=2, tiles=_ceil(EVEN, 256))
        _has(P(F32, NCHW, C, ODD, True), kernel="split", waves=4, tiles=_ceil(ODD, 128))
        _has(P(BF16, NCHW, C, ODD, True), kernel="reg", cpad=C, vec=1)                      # odd H*W: no whole words
    _has(P(BF16, NCHW, 151, EVEN, True, 2, 0), kernel="reg", cpad=151, vec=1)              # 2-byte aligned only
    _has(P(F32, NCHW, 151, EVEN, True, variant=native.k2_variant(reg_only=True)), kernel="reg", cpad=151, exact=True, vec=1, tune=2)
    _has(P(F32, NCHW, 151, EVEN, True, variant=native.k2_variant(tune=15, reg_only=True)), kernel="reg", cpad=151, tune=0)
    _has(P(F32, NCHW, 151, EVEN, True, variant=native.k2_variant(stream=15)), kernel="reg", cpad=151, vec=1, tune=0)
    _has(P(F32, NCHW, 151, EVEN, True, variant=native.k2_variant(vec=1, tune=2)), kernel="reg", cpad=151, vec=1, tune=2)
    _has(P(F32, NCHW, 150, EVEN, True, variant=native.k2_variant(reg_only=True)), kernel="reg", cpad=150, tune=0)
    # 32-bit lane offsets: C * H*W * elem_bytes < 2^31
    hw = 2 ** 31 // (151 * 4)
    _has(P(F32, NCHW, 151, hw, True), kernel="split")
    _has(P(F32, NCHW, 151, hw + 1, True), kernel="reg", cpad=151, tune=2)


def test_streaming_kernel_without_gradient(native):
    P = native.loss_plan
    _has(P(F32, NCHW, 151, EVEN, False), kernel="fwd", ch=4, waves=5, vec=4, tiles=_ceil(EVEN, 1024))
    _has(P(BF16, NCHW, 151, EVEN, False), kernel="fwd", ch=4, waves=4, vec=8, tiles=_ceil(EVEN, 2048))
    _has(P(F32, NCHW, 33, EVEN, False), kernel="fwd")
    _has(P(F32, NCHW, 32, EVEN, False), kernel="reg", cpad=32, vec=4)
    for dtype, vec in ((F32, 4), (BF16, 8)):
        for v, pair in ((1, (4, 5)), (2, (8, 3)), (3, (6, 4)), (4, (2, 8))):
            for C in (5, 21, 151):
                _has(P(dtype, NCHW, C, EVEN, False, variant=v << 8), kernel="fwd", ch=pair[0], waves=pair[1], vec=vec)
            assert native.k2_variant(stream=v) == v << 8
    _has(P(F32, NCHW, 151, ODD, False), kernel="reg", cpad=151, vec=1, tune=0)             # no 16-byte alignment
    _has(P(BF16, NCHW, 151, 2492, False), kernel="reg", cpad=151, vec=1)                    # 4 | H*W, but 16-bit needs 8
    _has(P(F32, NCHW, 151, EVEN, False, variant=1), kernel="reg", cpad=151, vec=1)
    _has(P(F32, NCHW, 151, EVEN, False, variant=native.k2_variant(reg_only=True)), kernel="reg", cpad=151, vec=1)
    _has(P(F32, NCHW, 5, EVEN, False, variant=native.k2_variant(stream=2, reg_only=True)), kernel="reg", cpad=8, vec=4)


def test_channels_last(native):
    P = native.loss_plan
    for grad in (True, False):
        _has(P(F32, NHWC, 151, ODD, grad), kernel="nhwc", vec=1, tiles=_ceil(ODD, 256))
        _has(P(BF16, NHWC, 21, EVEN, grad), kernel="nhwc", tiles=_ceil(EVEN, 256))
        _has(P(F32, NHWC, 159, EVEN, grad), kernel="nhwc")
        assert P(F32, NHWC, 160, EVEN, grad)["rc"] == 1      # 256 x 161 floats of LDS
        assert P(F32, NHWC, 161, EVEN, grad)["rc"] == 1
    assert P(F32, 2, 21, EVEN, True)["rc"] == 1


def test_words_that_name_no_kernel_are_invalid(native):
    P = native.loss_plan
    # the TUNE instantiations that are gone: 1-5 at C = 21, 1 and 3 at C = 151 (fp32, gradient)
    for t in (1, 2, 3, 4, 5):
        assert P(F32, NCHW, 21, EVEN, True, variant=4 | t << 4)["rc"] == 1, t
        assert P(F32, NCHW, 21, EVEN, True, variant=t << 4)["rc"] == 1, t
    for t in (1, 3):
        assert P(F32, NCHW, 151, EVEN, True, variant=1 | t << 4)["rc"] == 1, t
        assert P(F32, NCHW, 151, EVEN, True, variant=native.K2_REG_ONLY | t << 4)["rc"] == 1, t
    # a TUNE of another cell
    assert P(F32, NCHW, 21, EVEN, True, variant=4 | 6 << 4)["rc"] == 1
    assert P(F32, NCHW, 21, EVEN, False, variant=4 | 7 << 4)["rc"] == 1
    assert P(F32, NCHW, 151, EVEN, True, variant=1 | 7 << 4)["rc"] == 1
    # numbers no cell ever had, anywhere
    for t in (1, 3, 4, 5, 8, 9, 10, 11, 12, 13, 14):
        assert P(F32, NCHW, 5, EVEN, True, variant=t << 4)["rc"] == 1, t
    # ... while a shipped number outside its cell is ignored, as before
    _has(P(F32, NCHW, 5, EVEN, True, variant=7 << 4), kernel="reg", cpad=8, vec=4, tune=0)
    _has(P(BF16, NCHW, 21, EVEN, True, variant=4 | 7 << 4), kernel="reg", cpad=21, vec=4, tune=0)
    # the split kernel's wave-count words (1 = 5 waves, 2 = 3 waves, 3 = 4 waves) and any other streaming variant there
    for dtype in (F32, BF16):
        for C in (150, 151):
            for v in (1, 2, 3, 4):
                assert P(dtype, NCHW, C, EVEN, True, variant=v << 8)["rc"] == 1, (dtype, C, v)
    # fields without meaning
    for word in (3, 5, 8, 15, 5 << 8, 14 << 8, 1 << 13, 1 << 16, 1 << 31):
        assert P(F32, NCHW, 21, EVEN, True, variant=word)["rc"] == 1, hex(word)
        assert P(F32, NHWC, 21, EVEN, True, variant=word)["rc"] == 1, hex(word)
    for bad in (dict(vec=3), dict(tune=1), dict(tune=5), dict(stream=5)):
        with pytest.raises(ValueError):
            native.k2_variant(**bad)
    assert native.k2_variant() == 0 and native.k2_variant(reg_only=True) == 0x1000 == native.K2_REG_ONLY
    assert native.k2_variant(tune=15, reg_only=True) == 0x1000 | 15 << 4 and native.k2_variant(stream=15) == native.K2_NO_SPLIT
    # shapes and types
    assert P(F32, NCHW, 0, EVEN, True)["rc"] == 1 and P(F32, NCHW, 21, 0, True)["rc"] == 1
    out = (ctypes.c_int32 * 8)()
    assert native.lib().sea_loss_plan(3, NCHW, 21, EVEN, 1, 0, 0, 0, out) == 1
    assert native.lib().sea_loss_plan(0, NCHW, 21, EVEN, 1, 0, 0, 0, None) == 1


def test_header_constants_match(native):
    header = open(os.path.join(ROOT, "include", "sea_hip.h")).read()
    defs = dict(re.findall(r"^#define (SEA_K2_\w+) (.+)$", header, flags=re.M))
    assert int(defs["SEA_K2_VEC_MASK"].rstrip("u"), 0) == native.K2_VEC_MASK
    assert int(defs["SEA_K2_TUNE_SHIFT"]) == native.K2_TUNE_SHIFT and int(defs["SEA_K2_STREAM_SHIFT"]) == native.K2_STREAM_SHIFT
    assert int(defs["SEA_K2_REG_ONLY"].rstrip("u"), 0) == native.K2_REG_ONLY
    assert defs["SEA_K2_NO_SPLIT"] == "(15u << SEA_K2_STREAM_SHIFT)" and native.K2_NO_SPLIT == 15 << 8


def test_plan_header_is_plain_host_cxx():
    """csrc/loss_plan.h is C++17 for any host compiler: no HIP header, no device code"""
    path = os.path.join(PKG, "csrc", "loss_plan.h")
    text = open(path).read()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text
    assert re.findall(r'#include [<"]([^>"]+)[>"]', text) == ["stddef.h", "stdint.h", "../../include/sea_hip.h"]
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    cmd = [cxx] if cxx else [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-nogpuinc", "-nogpulib"]
    subprocess.run(cmd + ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(path), "-x", "c++", "-"],
                   input='#include "loss_plan.h"\nint main() { sea::LossPlan p; return sea::loss_plan(sea::LossQuery{}, &p); }\n',
                   text=True, check=True)


# ------------------------------------------------------------------------------------------------ (b) the sweep
def test_plan_invariants_sweep(native):
    L = native.lib()
    plan, ws_bytes = L.sea_loss_plan, L.sea_loss_workspace_bytes
    out = (ctypes.c_int32 * 8)()
    words = [0, 1, 2, 4] + [v << 8 for v in (1, 2, 3, 4)] + [15 << 8, native.K2_REG_ONLY, native.K2_REG_ONLY | 15 << 4]
    offsets = (0, 2, 4, 8)
    base_l, base_g = 1 << 20, 1 << 21
    n = 0
    for HW in (1, 2, 4, 7, 8, 128, 2491, 2496, 262144):
        room = ws_bytes(1, HW)
        for C in range(1, 261):
            for dtype, eb in ((0, 4), (1, 2)):
                for grad in (0, 1):
                    for ol in offsets:
                        for og in offsets:
                            elem_aligned = ol % eb == 0 and (not grad or og % eb == 0)
                            for word in words:
                                rc = plan(dtype, NCHW, C, HW, grad, base_l + ol, base_g + og, word, out)
                                n += 1
                                if rc:
                                    assert rc == 1 and word != 0, (rc, C, HW, eb, grad, ol, og, word)
                                    continue
                                kernel, cpad, exact, vec, tune, ch, waves, tiles = out
                                where = (C, HW, eb, grad, ol, og, hex(word), list(out))
                                assert tiles >= 1 and (tiles + 1) * 16 <= room, where
                                if kernel == 0:
                                    assert C <= cpad and exact == (C == cpad), where
                                if elem_aligned:
                                    assert HW % vec == 0 and ol % (vec * eb) == 0 and (not grad or og % (vec * eb) == 0), where
                                else:
                                    assert vec == 1, where
    assert n == 9 * 260 * 2 * 2 * 16 * len(words)
    for C in (261, 1000, 32767):     # word 0 never fails in NCHW
        for dtype in (0, 1, 2):
            for grad in (0, 1):
                for HW in (1, 2496, 262144):
                    assert plan(dtype, NCHW, C, HW, grad, base_l, base_g, 0, out) == 0 and out[0] in (1, 2), (C, dtype, grad, HW)
