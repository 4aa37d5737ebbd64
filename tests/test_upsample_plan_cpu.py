"""M2's selection plan (csrc/upsample_plan.h through sea_upsample_plan / _native.upsample_plan): which kernel a call of
sea_upsample_bilinear_{fwd, bwd, nhwc_fwd, nhwc_bwd} or sea_tap_gather_{fwd, bwd} runs, with which template parameter, grid and
launch scalars, without a device.

(a) pins rows of the map; (b) sweeps the plan against ``_dispatch_before_the_plan``, a transcription of the six launcher
bodies as they stood before the plan existed; (c) asserts on every successful plan of the sweep what a launch depends on;
(d) the header is plain host C++; and the source checks say that the decision lives nowhere else.

How the pinned rows follow from that dispatch (S = the power-of-two factor 2 / 4 / 8 / 16 common to both axes, else 0, and 0
under general_only; grid_for_xcd(n, b) = ceil(n / b) clamped to [1, 2048], rounded up to a multiple of 8):
  NCHW forward.  The vector kernels need S, W % 4 == 0 and a 16-byte aligned y; S >= 4 -> cells<S> over planes * (h + 1) * W/4
  items, S == 2 -> pow2<2> over planes * H * W/4; everything else the general kernel on (ceil(W/64), ceil(H/16), planes) in
  chunks of 65535 planes.
  * 13x11 -> 50x45: no common factor -> general, grid (1, 4).  5x3 -> 10x6: S = 2 but W = 6 -> general.  2x4 -> 4x8: pow2<2>,
    8 items -> grid 8; with y off by 4 bytes -> general.  2x3 -> 8x12: cells<4>, 1 * 3 * 3 = 9 items.  3x2 -> 24x16: cells<8>;
    1x2 -> 16x32: cells<16>.  nt = output bytes > 192 MB: 1208 planes of 512^2 (1.27 GB) -> 1, the small rows -> 0.
    65536 planes on the general kernel: two launches.
  NCHW backward.  rows<S> when S, W/4 in {32, 64, 128, 256}, gy 16-byte aligned, planes < 2^24, units = planes * bands < 2^30:
  lcols = log2(W/4), nsub = 256 / (W/4) sub-bands of RP = max(16 / S, 2) input rows, bands = ceil(h / (nsub * RP)).
  * 1x64 -> 2x128: S = 2, lcols 5, nsub 8, RP 8, bands 1.  1x8 -> 16x128: S = 16, RP 2, bands 1.  17x8 -> 272x128: RP 2,
    nsub 8 -> bands = ceil(17 / 16) = 2.  With SEA_XCD_ORDER on, per_xcd = ceil(units / 8) and the grid is 8 * per_xcd.
  Otherwise pow2<S> if gy is aligned to VL = min(4, S/2) floats (1 / 2 / 4 for S = 2 / 4 / >= 8): 2x3 -> 8x12 with gy off by
  4 bytes (VL = 2 needs 8) goes on to the tiled kernel, off by 8 bytes stays; 2x3 -> 4x6 takes any float address.
  Tiled: the largest power-of-two tile TI <= 32 with RMAX = int((TI + 1) * max ratio) + 4 <= 80 and
  4 * (RMAX * (RMAX + 1) + 4 * RMAX + 2 * (TI + 3) + RMAX * (TI + 1)) <= 48 KB of LDS.
  * 30x30 -> 119x119: ratio 3.967: TI = 32 gives 134, TI = 16 gives int(67.4) + 4 = 71 -> lds 4 * (5112 + 284 + 38 + 1207) =
    26564, grid (2, 2).  1x1 -> 40x40: TI = 1 gives 84 > 80 -> no tile fits: SEA_ERR_ARG.
  NHWC forward: S in {2, 4, 8} -> cells<S> over B * (h + 1) * (w + 1) * C/4 items of 256 per block; S == 16 -> <16>, else <0>,
  over B * H * W * C/4 items of 512 per block.
  NHWC backward: S in {2, 4, 8} -> pow2<S>; else total = B * h * w * C/4 < 65536 and B * h * w < 65536 -> small on a
  (B * h * w, ceil(C/64)) grid; else general.  16x16 -> 256x256 at C = 4: S = 16, total 256 -> small.  64x64 -> 96x96 at
  C = 64: total = 4096 * 16 = 65536 -> general.
  Tap gather: forward needs H >= 3h and W >= 3w (x2: SEA_ERR_ARG) and 32-bit offsets inside one image; x4 / x8 get <4> / <8>
  in both directions, everything else (x3: 2x2 -> 6x6; x16) <0> forward and the general kernel backward (x2 too).
"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

CSRC = os.path.join(PKG, "csrc")


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


def _plan(native, *a, **kw):
    kw.setdefault("general_only", False)                                     # not this process's environment
    kw.setdefault("xcd_order", 1)
    return native.upsample_plan(*a, **kw)


# ------------------------------------------------------------------------------------------------ (a) the pinned rows
def test_nchw_forward_rows(native):
    P = lambda *a, **kw: _plan(native, "nchw_fwd", *a, **kw)
    _has(P(1, 13, 11, 50, 45), kernel="nchw_fwd_general", S=0, grid_x=1, grid_y=4, threads=256, lds=0, chunk=65535, nchunks=1)
    _has(P(1, 5, 3, 10, 6), kernel="nchw_fwd_general", S=0, grid_x=1, grid_y=1)
    _has(P(1, 2, 4, 4, 8, dst_addr=4), kernel="nchw_fwd_general", S=0)
    _has(P(1, 2, 4, 4, 8), kernel="nchw_fwd_pow2", S=2, total=8, grid_x=8, grid_y=1, xo=0, chunk=0, nchunks=0)
    _has(P(1, 2, 4, 4, 8, src_addr=4), kernel="nchw_fwd_pow2", S=2)            # x is read with scalar loads
    _has(P(1, 2, 3, 8, 12), kernel="nchw_fwd_cells", S=4, total=9, grid_x=8, nt=0, xo=0)
    _has(P(1, 3, 2, 24, 16), kernel="nchw_fwd_cells", S=8, total=4 * 4, nt=0)
    _has(P(1, 1, 2, 16, 32), kernel="nchw_fwd_cells", S=16, total=2 * 8, nt=0)
    _has(P(151 * 8, 128, 128, 512, 512), kernel="nchw_fwd_cells", S=4, total=1208 * 129 * 128, grid_x=2048, nt=1, xo=0)
    _has(P(151 * 8, 128, 128, 512, 512, xcd_order=2), kernel="nchw_fwd_cells", xo=1)
    _has(P(65535, 13, 11, 50, 45), kernel="nchw_fwd_general", chunk=65535, nchunks=1)
    _has(P(65536, 13, 11, 50, 45), kernel="nchw_fwd_general", chunk=65535, nchunks=2)
    for shape in ((2, 4, 4, 8), (2, 3, 8, 12), (3, 2, 24, 16), (1, 2, 16, 32)):
        _has(P(1, *shape, general_only=True), kernel="nchw_fwd_general", S=0)


def test_nchw_backward_rows(native):
    P = lambda *a, **kw: _plan(native, "nchw_bwd", *a, **kw)
    _has(P(1, 1, 64, 2, 128), kernel="nchw_bwd_rows", S=2, lcols=5, RP=8, bands=1, total=1, per_xcd=1, grid_x=8, grid_y=1)
    _has(P(1, 1, 8, 16, 128), kernel="nchw_bwd_rows", S=16, lcols=5, RP=2, bands=1, total=1)
    _has(P(3, 17, 8, 272, 128), kernel="nchw_bwd_rows", S=16, lcols=5, RP=2, bands=2, total=6, per_xcd=1, grid_x=8)
    _has(P(3, 17, 8, 272, 128, xcd_order=0), kernel="nchw_bwd_rows", total=6, per_xcd=0, grid_x=6)
    for W, lcols in ((128, 5), (256, 6), (512, 7), (1024, 8)):
        _has(P(2, 4, W // 4, 16, W), kernel="nchw_bwd_rows", S=4, lcols=lcols, RP=4, bands=_ceil(4, (256 >> lcols) * 4))
    for W in (64, 2048, 192, 384):                                           # W / 4 is not 32, 64, 128 or 256
        _has(P(2, 4, W // 4, 16, W), kernel="nchw_bwd_pow2", S=4, total=2 * 4 * (W // 4))
    _has(P(1, 1, 64, 2, 128, src_addr=4), kernel="nchw_bwd_pow2", S=2)        # rows need 16 bytes, pow2<2> one float
    _has(P((1 << 24) - 1, 1, 64, 2, 128), kernel="nchw_bwd_rows")
    _has(P(1 << 24, 1, 64, 2, 128), kernel="nchw_bwd_pow2", S=2, total=1 << 30)
    # the alignment of pow2<S>: VL = 1 / 2 / 4 floats for S = 2 / 4 / >= 8
    _has(P(1, 2, 3, 4, 6, src_addr=4), kernel="nchw_bwd_pow2", S=2, total=6, grid_x=8, xo=0)
    _has(P(1, 2, 3, 8, 12, src_addr=8), kernel="nchw_bwd_pow2", S=4)
    _has(P(1, 2, 3, 8, 12, src_addr=4), kernel="nchw_bwd_general", S=0)
    _has(P(1, 2, 3, 16, 24, src_addr=16), kernel="nchw_bwd_pow2", S=8)
    _has(P(1, 2, 3, 16, 24, src_addr=8), kernel="nchw_bwd_general", S=0)
    _has(P(1, 2, 3, 32, 48), kernel="nchw_bwd_pow2", S=16, xo=0)
    _has(P(1, 2, 3, 32, 48, xcd_order=2), kernel="nchw_bwd_pow2", S=16, xo=1)
    _has(P(1, 2, 3, 32, 48, src_addr=8), kernel="nchw_bwd_general", S=0)
    _has(P(1, 2, 3, 8, 12, dst_addr=4), kernel="nchw_bwd_pow2", S=4)          # gx takes scalar stores
    # the tiled kernel
    _has(P(1, 30, 30, 119, 119), kernel="nchw_bwd_general", S=0, TI=16, RMAX=71, lds=26564, grid_x=2, grid_y=2, chunk=65535, nchunks=1)
    _has(P(65536, 30, 30, 119, 119), kernel="nchw_bwd_general", nchunks=2)
    _has(P(1, 1, 64, 2, 128, general_only=True), kernel="nchw_bwd_general", S=0, TI=32, RMAX=70, lds=30520, grid_x=2, grid_y=1)
    assert P(1, 1, 1, 40, 40)["rc"] == 1                                     # no tile fits


def test_nhwc_rows(native):
    F = lambda *a, **kw: _plan(native, "nhwc_fwd", *a, **kw)
    B = lambda *a, **kw: _plan(native, "nhwc_bwd", *a, **kw)
    for S in (2, 4, 8):
        _has(F(2, 3, 5, 3 * S, 5 * S, C_=8), kernel="nhwc_fwd_cells", S=S, total=2 * 4 * 6 * 2, grid_x=8, grid_y=1, xo=1)
        _has(F(2, 3, 5, 3 * S, 5 * S, C_=8, general_only=True), kernel="nhwc_fwd", S=0, total=2 * 15 * S * S * 2)
        _has(B(2, 3, 5, 3 * S, 5 * S, C_=8), kernel="nhwc_bwd_pow2", S=S, total=2 * 15 * 2, grid_x=8, xo=1)
        _has(B(2, 3, 5, 3 * S, 5 * S, C_=8, general_only=True), kernel="nhwc_bwd_small", S=0, grid_x=30, grid_y=1)
    _has(F(2, 3, 5, 48, 80, C_=8), kernel="nhwc_fwd", S=16, total=2 * 48 * 80 * 2, grid_x=_ceil(_ceil(15360, 512), 8) * 8)
    _has(F(2, 3, 5, 96, 160, C_=8), kernel="nhwc_fwd", S=0)                   # x32
    _has(F(2, 3, 5, 7, 11, C_=8, xcd_order=0), kernel="nhwc_fwd", S=0, xo=0)
    _has(F(2, 3, 5, 6, 20, C_=8), kernel="nhwc_fwd", S=0)                     # x2 and x4: no common factor
    _has(B(1, 16, 16, 256, 256, C_=4), kernel="nhwc_bwd_small", S=0, total=256, grid_x=256, grid_y=1, threads=256)
    _has(B(1, 2, 2, 6, 6, C_=132), kernel="nhwc_bwd_small", S=0, grid_x=4, grid_y=3)
    _has(B(1, 64, 64, 96, 96, C_=64), kernel="nhwc_bwd_general", S=0, total=65536, grid_x=256, xo=1)
    _has(B(1, 64, 64, 96, 96, C_=60), kernel="nhwc_bwd_small", total=4096 * 15)
    _has(B(16, 64, 64, 96, 96, C_=4), kernel="nhwc_bwd_general", total=65536)  # B * h * w = 65536 as well
    _has(B(1, 64, 64, 1024, 1024, C_=64), kernel="nhwc_bwd_general", S=0)     # x16 has no pow2 instantiation
    # arguments: channels in fours, the pixel stride, 16-byte alignment of every tensor
    for P in (F, B):
        assert P(2, 3, 5, 6, 10, C_=6)["rc"] == 1 and P(2, 3, 5, 6, 10, C_=0)["rc"] == 1 and P(0, 3, 5, 6, 10, C_=8)["rc"] == 1
        assert P(2, 3, 5, 6, 10, C_=8, pixel_stride=4)["rc"] == 1 and P(2, 3, 5, 6, 10, C_=8, pixel_stride=10)["rc"] == 1
        assert P(2, 3, 5, 6, 10, C_=8, pixel_stride=24)["rc"] == 0
        assert P(2, 3, 5, 6, 10, C_=8, src_addr=8)["rc"] == 1 and P(2, 3, 5, 6, 10, C_=8, dst_addr=4)["rc"] == 1
        assert P(2, 3, 5, 2, 10, C_=8)["rc"] == 1 and P(2, 3, 5, 6, 4, C_=8)["rc"] == 1 and P(2, 0, 5, 6, 10, C_=8)["rc"] == 1


def test_tap_gather_rows(native):
    F = lambda *a, **kw: _plan(native, "tap_fwd", *a, **kw)
    B = lambda *a, **kw: _plan(native, "tap_bwd", *a, **kw)
    for S in (4, 8):
        _has(F(2, 3, 5, 3 * S, 5 * S, C_=8), kernel="tap_fwd", S=S, nbh=_ceil(3 * S, 4), nbw=_ceil(5 * S, 4),
             total=2 * _ceil(3 * S, 4) * _ceil(5 * S, 4) * 2, grid_y=1, xo=1)
        _has(B(2, 3, 5, 3 * S, 5 * S, C_=8), kernel="tap_bwd_pow2", S=S, total=2 * 15 * 2, grid_x=8, xo=1)
        _has(F(2, 3, 5, 3 * S, 5 * S, C_=8, general_only=True), kernel="tap_fwd", S=0)
        _has(B(2, 3, 5, 3 * S, 5 * S, C_=8, general_only=True), kernel="tap_bwd_general", S=0)
    _has(F(1, 2, 2, 6, 6, C_=4), kernel="tap_fwd", S=0, nbh=2, nbw=2, total=4, grid_x=8)
    _has(B(1, 2, 2, 6, 6, C_=4), kernel="tap_bwd_general", S=0, total=4)
    _has(F(1, 2, 2, 32, 32, C_=4), kernel="tap_fwd", S=0)                     # x16
    _has(B(1, 2, 2, 32, 32, C_=4), kernel="tap_bwd_general", S=0)
    for general in (False, True):
        assert F(1, 2, 2, 4, 4, C_=4, general_only=general)["rc"] == 1      # x2: a factor below 3
        _has(B(1, 2, 2, 4, 4, C_=4, general_only=general), kernel="tap_bwd_general", S=0)
    assert F(1, 2, 2, 6, 5, C_=4)["rc"] == 1 and F(1, 2, 2, 6, 6, C_=4, src_addr=8)["rc"] == 1 and F(1, 2, 2, 6, 6, C_=2)["rc"] == 1
    # 32-bit offsets inside one image: H * W * C/4 and h * w * 9 * C/4 below 2^31
    _has(F(1, 16, 16, 1024, 1024, C_=8188), kernel="tap_fwd", S=0)
    assert F(1, 16, 16, 1024, 1024, C_=8192)["rc"] == 1


def test_invalid_arguments(native):
    L = native.lib()
    out = (ctypes.c_int32 * 20)()
    assert L.sea_upsample_plan(0, 1, 0, 2, 4, 4, 8, 0, 0, 0, 0, 1, None) == 1
    assert L.sea_upsample_plan(0, 1, 0, 2, 4, 4, 8, 0, 0, 0, 0, 1, out) == 0 and out[0] == 1 and out[1] == 2
    for op in (-1, 6):
        assert L.sea_upsample_plan(op, 1, 8, 2, 4, 4, 8, 8, 0, 0, 0, 1, out) == 1
    for xcd in (-1, 3):
        assert L.sea_upsample_plan(0, 1, 0, 2, 4, 4, 8, 0, 0, 0, 0, xcd, out) == 1
    for op in ("nchw_fwd", "nchw_bwd"):
        P = lambda *a: _plan(native, op, *a)
        assert P(0, 2, 4, 4, 8)["rc"] == 1 and P(1, 0, 4, 4, 8)["rc"] == 1 and P(1, 2, 0, 4, 8)["rc"] == 1
        assert P(1, 2, 4, 1, 8)["rc"] == 1 and P(1, 2, 4, 4, 3)["rc"] == 1 and P(1, 2, 4, 2, 4)["rc"] == 0


def test_the_binding_defaults_to_the_process_configuration(native):
    L = native.lib()
    got = native.upsample_plan("nchw_bwd", 3, 17, 8, 272, 128)
    assert got == native.upsample_plan("nchw_bwd", 3, 17, 8, 272, 128, general_only=L.sea_process_config(1),
                                       xcd_order=L.sea_process_config(0))
    assert set(got) == set(native._UPSAMPLE_PLAN_FIELDS) - {"total_lo", "total_hi"} | {"total", "rc"}
    assert len(native.UPSAMPLE_KERNELS) == 14 and len(native.UPSAMPLE_OPS) == 6


# ------------------------------------------------------------------------------------------------ (d) and the source checks
def test_plan_header_is_plain_host_cxx():
    """csrc/upsample_plan.h (and launch_grid.h under it) is C++17 for any host compiler: no HIP header, no device code"""
    for name in ("upsample_plan.h", "launch_grid.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert "hip/" not in text and "__device__" not in text and "__global__" not in text and "sea_common.h" not in re.findall(r"#include (.*)", text)
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    cmd = [cxx] if cxx else [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-nogpuinc", "-nogpulib"]
    subprocess.run(cmd + ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", CSRC, "-x", "c++", "-"],
                   input='#include "upsample_plan.h"\nint main() { sea::UpsamplePlan p;\n'
                         '  return sea::upsample_plan(sea::UpsampleQuery{}, &p) + sea::grid_for(1, 256); }\n',
                   text=True, check=True)
    header = open(os.path.join(ROOT, "include", "sea_hip.h")).read()
    assert "int sea_upsample_plan(" in header and "csrc/upsample_plan.h" in header
    ops = {k: int(v) for k, v in re.findall(r"#define SEA_UP_(\w+) (\d+)", header)}
    assert ops == {"NCHW_FWD": 0, "NCHW_BWD": 1, "NHWC_FWD": 2, "NHWC_BWD": 3, "TAP_FWD": 4, "TAP_BWD": 5}


def test_the_decision_lives_in_the_plan_only(native):
    """No launcher recomputes the factor or consults the process switch except to fill a query; the duplicated index rules are
    gone; the grid limit has one definition; the export is declared, bound and in the library."""
    texts = {n: open(os.path.join(CSRC, n)).read() for n in sorted(os.listdir(CSRC))}
    for name, text in texts.items():
        if name != "upsample_plan.h":
            assert "pow2_factor" not in text and "plan_bwd" not in text and "upsample_general_only" not in text, name
        if name in ("upsample_plan.h", "sea_common.h", "api_misc.cpp"):      # the plan's field; the struct; where it is read once
            continue
        # every read of the switch is an initialiser of an UpsampleQuery (the statement that builds the query)
        for m in re.finditer(r"upsample_general", text):
            stmt = text[text.rfind(";", 0, m.start()) + 1:m.start()]
            assert "UpsampleQuery{" in stmt and re.search(r"process_config\(\)\.$", stmt), (name, stmt)
        assert "general_only" not in text or "UpsampleQuery{" in text, name
    for name in ("upsample_kernels.hip", "fpn_fused.hip"):
        body = texts[name]
        assert "#define SEA_LAUNCH" not in body and "switch (S)" not in body and "xcd_order_enabled" not in body, name
    everything = "\n".join(texts.values())
    assert "nhwc_axis" not in everything and "first_dst_with_i0_ge" not in everything
    assert len(re.findall(r"float lerp2\(", everything)) == 1 and "float lerp2(" in texts["bilinear_map.h"]
    assert len(re.findall(r"\bstruct AxisMap\b", everything)) == 0 and len(re.findall(r"\bstruct AxisMapU\b", everything)) == 1
    assert len(re.findall(r"constexpr int LOG = S == 2", everything)) == 1    # Pow2<S>::LOG of bilinear_map.h
    assert len(re.findall(r"kMaxGridX\s*=", everything)) == 1 and "kMaxGridX =" in texts["launch_grid.h"]
    # the symbol: declared in the header, bound with a prototype, exported by the library (test_host_cpu.py checks the sets)
    header = open(os.path.join(ROOT, "include", "sea_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t|size_t|const char\*)\s+(sea_\w+)\s*\(", header, flags=re.M))
    assert "sea_upsample_plan" in declared and "sea_upsample_plan" in native.EXPORTS and declared == set(native.EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "sea_upsample_plan" in set(re.findall(r" T (sea_\w+)", out))
    assert native.lib().sea_abi_version() == 3


# ------------------------------------------------------------------------------------------------ (b), (c) the sweep
K_FG, K_FP, K_FC, K_BG, K_BR, K_BP, K_NF, K_NFC, K_NBG, K_NBS, K_NBP, K_TF, K_TBG, K_TBP = range(14)


def _grid_for(n, block):
    return min(max(_ceil(n, block), 1), 256 * 8)


def _grid_for_xcd(n, block):
    return _ceil(_grid_for(n, block), 8) * 8


def _pow2_factor(h, w, H, W):
    for S in (2, 4, 8, 16):
        if h * S == H and w * S == W:
            return S
    return 0


def _dispatch_before_the_plan(op, n, C, h, w, H, W, stride, src, dst, general_only, xcd):
    """The six launcher bodies as they stood before upsample_plan.h, statement by statement (the pointer checks aside).  None =
    SEA_ERR_ARG, else the plan's fields in the order of _UPSAMPLE_PLAN_FIELDS with `total` as one integer."""
    def plan(kernel, S=0, gx=1, gy=1, lds=0, chunk=0, nchunks=0, total=0, xo=0, nt=0, lcols=0, RP=0, bands=0, per_xcd=0, TI=0,
             RMAX=0, nbh=0, nbw=0):
        return (kernel, S, gx, gy, 256, lds, chunk, nchunks, total, xo, nt, lcols, RP, bands, per_xcd, TI, RMAX, nbh, nbw)

    if op in (0, 1):                                                         # sea_upsample_bilinear_fwd / _bwd
        planes = n
        if not (planes > 0 and h > 0 and w > 0 and H >= h and W >= w):
            return None
        S = 0 if general_only else _pow2_factor(h, w, H, W)
        nchunks = len(range(0, planes, 65535))
    if op == 0:
        if S and dst & 15 == 0:
            if W & 3 == 0:
                if S >= 4:
                    total = planes * (h + 1) * (W // 4)
                    return plan(K_FC, S, _grid_for_xcd(total, 256), total=total, xo=int(xcd == 2),
                                nt=int(planes * H * W * 4 > 192 << 20))
                total = planes * H * (W // 4)
                return plan(K_FP, 2, _grid_for_xcd(total, 256), total=total, xo=int(xcd == 2))
        return plan(K_FG, 0, (W + 63) // 64, (H + 15) // 16, chunk=65535, nchunks=nchunks)
    if op == 1:
        VL = 4 if S // 2 >= 4 else S // 2
        cols = W // 4
        if S and W & 3 == 0 and cols in (32, 64, 128, 256) and src & 15 == 0 and planes < 1 << 24:
            lcols = 5
            while 1 << lcols < cols:
                lcols += 1
            nsub = 256 // cols
            RP = 16 // S if 16 // S > 2 else 2
            bands = (h + nsub * RP - 1) // (nsub * RP)
            units = planes * bands
            if units < 1 << 30:
                per_xcd = (units + 7) // 8 if xcd else 0
                return plan(K_BR, S, per_xcd * 8 if per_xcd else units, total=units, lcols=lcols, RP=RP, bands=bands, per_xcd=per_xcd)
        if S and src & (VL * 4 - 1) == 0 and W % (VL if VL > 1 else 1) == 0:
            total = planes * h * w
            return plan(K_BP, S, _grid_for_xcd(total, 256), total=total, xo=int(xcd == 2))
        sh, sw = H / h, W / w                                                # plan_bwd
        s = sh if sh > sw else sw
        t = 32
        while t >= 1:
            rm = int((t + 1) * s) + 4
            b = 4 * (rm * (rm + 1) + 4 * rm + 2 * (t + 3) + rm * (t + 1))
            if rm <= 80 and b <= 48 * 1024:
                return plan(K_BG, 0, (w + t - 1) // t, (h + t - 1) // t, lds=b, chunk=65535, nchunks=nchunks, TI=t, RMAX=rm)
            t >>= 1
        return None
    B = n
    if op in (2, 3):                                                         # sea_upsample_bilinear_nhwc_fwd / _bwd
        if not (B > 0 and C > 0 and C % 4 == 0 and h > 0 and w > 0 and H >= h and W >= w):
            return None
        if not (stride >= C and stride % 4 == 0):
            return None
        if (src | dst) & 15:
            return None
        S = 0 if general_only else _pow2_factor(h, w, H, W)
    if op == 2:
        total = B * H * W * (C // 4)
        if S in (2, 4, 8):
            cells = B * (h + 1) * (w + 1) * (C // 4)
            return plan(K_NFC, S, _grid_for_xcd(cells, 256), total=cells, xo=xcd)
        return plan(K_NF, 16 if S == 16 else 0, _grid_for_xcd(total, 256 * 2), total=total, xo=xcd)
    if op == 3:
        total = B * h * w * (C // 4)
        if S in (2, 4, 8):
            return plan(K_NBP, S, _grid_for_xcd(total, 256), total=total, xo=xcd)
        if total < 65536 and B * h * w < 65536:
            return plan(K_NBS, 0, B * h * w, (C // 4 + 15) // 16, total=total)
        return plan(K_NBG, 0, _grid_for_xcd(total, 256), total=total, xo=xcd)
    if op == 4:                                                              # sea_tap_gather_fwd
        if not (B > 0 and C > 0 and C % 4 == 0 and h > 0 and w > 0):
            return None
        if not (H >= 3 * h and W >= 3 * w):
            return None
        if (src | dst) & 15:
            return None
        nBh, nBw = (H + 3) // 4, (W + 3) // 4
        total = B * nBh * nBw * (C // 4)
        if not (H * W * (C // 4) < 1 << 31 and h * w * 9 * (C // 4) < 1 << 31):
            return None
        if not general_only and h * 4 == H and w * 4 == W:
            S = 4
        elif not general_only and h * 8 == H and w * 8 == W:
            S = 8
        else:
            S = 0
        return plan(K_TF, S, _grid_for_xcd(total, 256), total=total, xo=xcd, nbh=nBh, nbw=nBw)
    if not (B > 0 and C > 0 and C % 4 == 0 and h > 0 and w > 0 and H >= h and W >= w):   # sea_tap_gather_bwd
        return None
    if (src | dst) & 15:
        return None
    total = B * h * w * (C // 4)
    if not general_only and h * 4 == H and w * 4 == W:
        return plan(K_TBP, 4, _grid_for_xcd(total, 256), total=total, xo=xcd)
    if not general_only and h * 8 == H and w * 8 == W:
        return plan(K_TBP, 8, _grid_for_xcd(total, 256), total=total, xo=xcd)
    return plan(K_TBG, 0, _grid_for_xcd(total, 256), total=total, xo=xcd)


SWEEP_SIZES = tuple(range(1, 10)) + (16, 30, 32, 33, 64, 128, 512)
SWEEP_MAPS = tuple((lambda h, w, f=f: (h * f, w * f)) for f in (1, 2, 3, 4, 8, 16, 32)) + (       # integer factors
    lambda h, w: (2 * h + 1, 3 * w + 2), lambda h, w: (h + 3, 2 * w), lambda h, w: (4 * h, 8 * w),  # ragged / two factors
    lambda h, w: ((7 * h + 1) // 2, (7 * w + 1) // 2), lambda h, w: (h - 1, 2 * w))                # x3.5; H < h
SWEEP_PLANES = (1, 8, 65535, 65536, 1 << 24)                                 # NCHW: the chunk and the rows kernel's plane limit
SWEEP_BC = ((1, 4), (2, 8), (1, 64), (16, 4), (3, 6))                        # NHWC / tap: B, C (64x64 at (1, 64): 65536 items)
SWEEP_ADDR = ((0, 0), (4, 0), (0, 8), (16, 4))                               # src, dst modulo 16 (and beyond)
SWEEP_CONFIG = tuple((g, x) for g in (0, 1) for x in (0, 1, 2))

TEMPLATE_VALUES = {K_FG: (0,), K_FP: (2,), K_FC: (4, 8, 16), K_BG: (0,), K_BR: (2, 4, 8, 16), K_BP: (2, 4, 8, 16), K_NF: (0, 16),
                   K_NFC: (2, 4, 8), K_NBG: (0,), K_NBS: (0,), K_NBP: (2, 4, 8), K_TF: (0, 4, 8), K_TBG: (0,), K_TBP: (4, 8)}
XCD_RANGE_KERNELS = {K_FP, K_FC, K_BP, K_NF, K_NFC, K_NBG, K_NBP, K_TF, K_TBG, K_TBP}     # their index space goes through xcd_range


def test_sweep_agrees_with_the_dispatch_before_the_plan(native):
    plan = native.lib().sea_upsample_plan
    out = (ctypes.c_int32 * 20)()
    n_calls, seen = 0, set()
    for h in SWEEP_SIZES:
        for w in SWEEP_SIZES:
            for size in SWEEP_MAPS:
                H, W = size(h, w)
                for op in range(6):
                    for n, C in (((p, 0) for p in SWEEP_PLANES) if op < 2 else SWEEP_BC):
                        stride = C + 8 if (op in (2, 3) and n == 2) else C
                        for src, dst in SWEEP_ADDR:
                            for general, xcd in SWEEP_CONFIG:
                                want = _dispatch_before_the_plan(op, n, C, h, w, H, W, stride, src, dst, general, xcd)
                                rc = plan(op, n, C, h, w, H, W, stride, src, dst, general, xcd, out)
                                n_calls += 1
                                g = out[:]
                                got = tuple(g[:8]) + ((g[9] << 32) | (g[8] & 0xffffffff),) + tuple(g[10:])
                                where = (op, n, C, h, w, H, W, stride, src, dst, general, xcd, got, want)
                                assert rc == (want is None), where
                                if rc:
                                    continue
                                assert got == want, where                    # every field of the plan
                                # (c) what every launch depends on
                                (kernel, S, gx, gy, threads, lds, chunk, nchunks, total, xo, nt, lcols, RP, bands, per_xcd, TI,
                                 RMAX, nbh, nbw) = got
                                assert gx >= 1 and gy >= 1 and threads == 256 and S in TEMPLATE_VALUES[kernel], where
                                assert kernel // 3 == op if op < 2 else kernel in ((K_NF, K_NFC), (K_NBG, K_NBS, K_NBP), (K_TF,),
                                                                                  (K_TBG, K_TBP))[op - 2], where
                                if kernel in XCD_RANGE_KERNELS:
                                    assert gx % 8 == 0 and gy == 1 and total >= 1 and gx <= 2048 and xo in (0, 1, 2), where
                                if kernel in (K_FG, K_BG):
                                    assert chunk == 65535 and (nchunks - 1) * chunk < n <= nchunks * chunk and gy <= 65535, where
                                else:
                                    assert chunk == 0 and nchunks == 0, where
                                if kernel == K_BG:
                                    assert 0 < lds <= 48 * 1024 and RMAX <= 80 and TI in (1, 2, 4, 8, 16, 32), where
                                    assert gx * TI >= w and gy * TI >= h and RMAX >= (TI + 1) * max(H / h, W / w), where
                                else:
                                    assert lds == 0 and TI == 0 and RMAX == 0, where
                                if kernel == K_BR:
                                    cols, nsub = 1 << lcols, 256 >> lcols
                                    assert cols * nsub == 256 and cols * 4 == W and bands * nsub * RP >= h > (bands - 1) * nsub * RP, where
                                    assert total == n * bands < 1 << 30 and W <= 1024, where   # V[2][1024] holds nsub rows of W floats
                                    assert (gx == per_xcd * 8 >= total and gx % 8 == 0) if xcd else (per_xcd == 0 and gx == total), where
                                if kernel == K_NBS:
                                    assert gx == n * h * w < 65536 and gy * 16 >= C // 4 > (gy - 1) * 16, where
                                if kernel == K_TF:
                                    assert nbh * 4 >= H > (nbh - 1) * 4 and nbw * 4 >= W > (nbw - 1) * 4 and total == n * nbh * nbw * (C // 4), where
                                seen.add((kernel, S))
    assert n_calls == len(SWEEP_SIZES) ** 2 * len(SWEEP_MAPS) * 6 * 5 * len(SWEEP_ADDR) * len(SWEEP_CONFIG)
    # every instantiation behind the six entry points is reached
    assert seen == {(k, S) for k, values in TEMPLATE_VALUES.items() for S in values}
