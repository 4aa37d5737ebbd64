#!/usr/bin/env python3
"""Bits of the M2 / tap-gather entry points on the pinned shapes of csrc/upsample_plan.h: one line per case, the case's name
and the SHA-256 of the output's bytes on seeded inputs.

    python devtools/upsample_plan_bits.py > listing.txt          (also under SEA_UPSAMPLE_GENERAL=1, SEA_XCD_ORDER=0 / 2)

Two commits whose listings are equal line for line compute the same bits on every kernel of the family: the smallest shape
that reaches each enumerator of the plan (tests/test_upsample_plan_cpu.py derives the map), every template value, misaligned
views (one float off) where alignment decides, and more than 65535 planes on the two chunked kernels.  The script calls the C
entries directly and uses nothing of the plan, so it runs unchanged on a commit from before the plan existed.
tests/test_upsample_plan_gpu.py runs the same cases against float64 references.
"""
import hashlib
import os
import sys
from collections import namedtuple

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "robust-segmentation_amd"))

# kernel / S: what the default dispatch reaches (asserted by the GPU test, not used here).  B, C: planes = B * C for NCHW.
# src_off / dst_off: floats by which the tensor the kernel reads / writes is displaced from a 16-byte aligned address.
Case = namedtuple("Case", "name op kernel S B C h w H W src_off dst_off", defaults=(0, 0))
CASES = [
    Case("nchw_fwd_general_ragged", "nchw_fwd", "nchw_fwd_general", 0, 1, 2, 13, 11, 50, 45),
    Case("nchw_fwd_general_w6", "nchw_fwd", "nchw_fwd_general", 0, 1, 2, 5, 3, 10, 6),
    Case("nchw_fwd_general_y_off", "nchw_fwd", "nchw_fwd_general", 0, 2, 3, 2, 4, 4, 8, 0, 1),
    Case("nchw_fwd_general_two_chunks", "nchw_fwd", "nchw_fwd_general", 0, 1, 65539, 1, 1, 2, 3),
    Case("nchw_fwd_pow2_2", "nchw_fwd", "nchw_fwd_pow2", 2, 2, 3, 2, 4, 4, 8),
    Case("nchw_fwd_cells_4", "nchw_fwd", "nchw_fwd_cells", 4, 2, 3, 2, 3, 8, 12),
    Case("nchw_fwd_cells_8", "nchw_fwd", "nchw_fwd_cells", 8, 1, 2, 3, 2, 24, 16),
    Case("nchw_fwd_cells_16", "nchw_fwd", "nchw_fwd_cells", 16, 1, 2, 1, 2, 16, 32),
    Case("nchw_bwd_rows_2", "nchw_bwd", "nchw_bwd_rows", 2, 1, 2, 1, 64, 2, 128),
    Case("nchw_bwd_rows_4", "nchw_bwd", "nchw_bwd_rows", 4, 1, 2, 2, 32, 8, 128),
    Case("nchw_bwd_rows_8", "nchw_bwd", "nchw_bwd_rows", 8, 1, 2, 2, 16, 16, 128),
    Case("nchw_bwd_rows_16", "nchw_bwd", "nchw_bwd_rows", 16, 1, 2, 1, 8, 16, 128),
    Case("nchw_bwd_rows_16_two_bands", "nchw_bwd", "nchw_bwd_rows", 16, 1, 3, 17, 8, 272, 128),
    Case("nchw_bwd_pow2_2_gy_off", "nchw_bwd", "nchw_bwd_pow2", 2, 2, 3, 2, 3, 4, 6, 1),
    Case("nchw_bwd_pow2_4", "nchw_bwd", "nchw_bwd_pow2", 4, 2, 3, 2, 3, 8, 12),
    Case("nchw_bwd_pow2_8", "nchw_bwd", "nchw_bwd_pow2", 8, 1, 2, 2, 3, 16, 24),
    Case("nchw_bwd_pow2_16", "nchw_bwd", "nchw_bwd_pow2", 16, 1, 2, 2, 3, 32, 48),
    Case("nchw_bwd_general_gy_off", "nchw_bwd", "nchw_bwd_general", 0, 2, 3, 2, 3, 8, 12, 1),
    Case("nchw_bwd_general_ragged", "nchw_bwd", "nchw_bwd_general", 0, 1, 2, 30, 30, 119, 119),
    Case("nchw_bwd_general_two_chunks", "nchw_bwd", "nchw_bwd_general", 0, 1, 65539, 1, 1, 2, 3),
    Case("nhwc_fwd_cells_2", "nhwc_fwd", "nhwc_fwd_cells", 2, 2, 8, 3, 5, 6, 10),
    Case("nhwc_fwd_cells_4", "nhwc_fwd", "nhwc_fwd_cells", 4, 2, 8, 3, 5, 12, 20),
    Case("nhwc_fwd_cells_8", "nhwc_fwd", "nhwc_fwd_cells", 8, 1, 4, 3, 5, 24, 40),
    Case("nhwc_fwd_16", "nhwc_fwd", "nhwc_fwd", 16, 1, 4, 3, 5, 48, 80),
    Case("nhwc_fwd_0", "nhwc_fwd", "nhwc_fwd", 0, 2, 8, 3, 5, 7, 11),
    Case("nhwc_bwd_pow2_2", "nhwc_bwd", "nhwc_bwd_pow2", 2, 2, 8, 3, 5, 6, 10),
    Case("nhwc_bwd_pow2_4", "nhwc_bwd", "nhwc_bwd_pow2", 4, 2, 8, 3, 5, 12, 20),
    Case("nhwc_bwd_pow2_8", "nhwc_bwd", "nhwc_bwd_pow2", 8, 1, 4, 3, 5, 24, 40),
    Case("nhwc_bwd_small_x16", "nhwc_bwd", "nhwc_bwd_small", 0, 1, 4, 16, 16, 256, 256),
    Case("nhwc_bwd_small_x3", "nhwc_bwd", "nhwc_bwd_small", 0, 2, 8, 2, 2, 6, 6),
    Case("nhwc_bwd_general", "nhwc_bwd", "nhwc_bwd_general", 0, 1, 64, 64, 64, 96, 96),
    Case("tap_fwd_4", "tap_fwd", "tap_fwd", 4, 2, 8, 3, 5, 12, 20),
    Case("tap_fwd_8", "tap_fwd", "tap_fwd", 8, 1, 4, 3, 5, 24, 40),
    Case("tap_fwd_0_x3", "tap_fwd", "tap_fwd", 0, 2, 8, 2, 2, 6, 6),
    Case("tap_bwd_pow2_4", "tap_bwd", "tap_bwd_pow2", 4, 2, 8, 3, 5, 12, 20),
    Case("tap_bwd_pow2_8", "tap_bwd", "tap_bwd_pow2", 8, 1, 4, 3, 5, 24, 40),
    Case("tap_bwd_general_x3", "tap_bwd", "tap_bwd_general", 0, 2, 8, 2, 2, 6, 6),
    Case("tap_bwd_general_x2", "tap_bwd", "tap_bwd_general", 0, 1, 4, 2, 2, 4, 4),
]


def src_shape(c):
    """Shape of what the entry reads, in the entry's own memory layout."""
    return {"nchw_fwd": (c.B, c.C, c.h, c.w), "nchw_bwd": (c.B, c.C, c.H, c.W), "nhwc_fwd": (c.B, c.h, c.w, c.C),
            "nhwc_bwd": (c.B, c.H, c.W, c.C), "tap_fwd": (c.B, c.h, c.w, 9, c.C), "tap_bwd": (c.B, c.H, c.W, c.C)}[c.op]


def dst_shape(c):
    return {"nchw_fwd": (c.B, c.C, c.H, c.W), "nchw_bwd": (c.B, c.C, c.h, c.w), "nhwc_fwd": (c.B, c.H, c.W, c.C),
            "nhwc_bwd": (c.B, c.h, c.w, c.C), "tap_fwd": (c.B, c.H, c.W, c.C), "tap_bwd": (c.B, c.h, c.w, 9, c.C)}[c.op]


def _buffer(shape, off):
    """Device float32 tensor of `shape` whose address is a 16-byte aligned one plus 4 * off bytes."""
    numel = 1
    for s in shape:
        numel *= s
    flat = torch.full((numel + 4,), float("nan"), dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    return flat[off:off + numel].view(shape)


def run(N, c, src_cpu):
    """Calls the entry of case `c` on `src_cpu` (float32, src_shape(c)); returns (source, output) on the device."""
    src, dst = _buffer(src_shape(c), c.src_off), _buffer(dst_shape(c), c.dst_off)
    src.copy_(src_cpu)
    L, st, a, b = N.lib(), N._stream(), src.data_ptr(), dst.data_ptr()
    if c.op == "nchw_fwd":
        rc = L.sea_upsample_bilinear_fwd(a, b, c.B * c.C, c.h, c.w, c.H, c.W, st)
    elif c.op == "nchw_bwd":
        rc = L.sea_upsample_bilinear_bwd(a, b, c.B * c.C, c.h, c.w, c.H, c.W, st)
    elif c.op == "nhwc_fwd":
        rc = L.sea_upsample_bilinear_nhwc_fwd(a, None, b, c.B, c.C, c.h, c.w, c.H, c.W, c.C, st)
    elif c.op == "nhwc_bwd":
        rc = L.sea_upsample_bilinear_nhwc_bwd(a, b, c.B, c.C, c.h, c.w, c.H, c.W, c.C, st)
    elif c.op == "tap_fwd":
        rc = L.sea_tap_gather_fwd(a, b, 0, c.B, c.C, c.h, c.w, c.H, c.W, 1, st)
    else:
        rc = L.sea_tap_gather_bwd(a, b, c.B, c.C, c.h, c.w, c.H, c.W, st)
    if rc != 0:
        raise RuntimeError(f"{c.name}: the entry returned {rc}")
    return src, dst


def main():
    from semseg import _native as N
    for i, c in enumerate(CASES):
        src_cpu = torch.randn(src_shape(c), generator=torch.Generator().manual_seed(1000 + i))
        _, out = run(N, c, src_cpu)
        torch.cuda.synchronize()
        print(c.name, hashlib.sha256(out.cpu().contiguous().numpy().tobytes()).hexdigest(), flush=True)


if __name__ == "__main__":
    main()
