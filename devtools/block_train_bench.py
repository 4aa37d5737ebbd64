#!/usr/bin/env python3
"""T3 micro-benchmark: forward + backward of ONE train-mode ConvNeXt block (drop rate 0.2, trainable weights, channels_last
input) with TRAIN_NATIVE_BLOCKS off against on, in one process, alternating the two; and T3a (sea_layernorm_bwd_params) alone
against F.layer_norm's autograd backward at the same row counts.  B = 8 at the four stage shapes of ConvNeXt-T on a 512 x 512
crop.  Device-event times, median of `--reps` windows of `--iters` calls after a warm-up of every shape.

    python devtools/block_train_bench.py [--reps 7] [--iters 20]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "robust-segmentation_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from semseg import _native as N  # noqa: E402
from semseg.models import convnext_upernet as M  # noqa: E402

SHAPES = [(128, 96), (64, 192), (32, 384), (16, 768)]   # (H = W, C)
B = 8


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us per call


def compare(fns, reps, iters):
    """{name: (median us, min, max)} of the alternated windows"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(window(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def block_step(blk, x, g, on):
    def f():
        M.TRAIN_NATIVE_BLOCKS = on
        blk.zero_grad(set_to_none=True)
        x.grad = None
        blk(x).backward(g)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of a device kernel"
    prev = M.TRAIN_NATIVE_BLOCKS
    try:
        for S, C in SHAPES:
            torch.manual_seed(0)
            blk = M.Block(C, drop_path=0.2).cuda().train()
            x = torch.randn(B, C, S, S, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
            g = torch.randn(B, C, S, S, device="cuda").contiguous(memory_format=torch.channels_last)
            r = compare({"off": block_step(blk, x, g, False), "on": block_step(blk, x, g, True)}, args.reps, args.iters)
            print(json.dumps({"what": "block fwd+bwd", "B": B, "HW": S, "C": C, "us_off": [round(v, 1) for v in r["off"]],
                              "us_on": [round(v, 1) for v in r["on"]], "on_over_off": round(r["on"][0] / r["off"][0], 3)}),
                  flush=True)
        for S, C in SHAPES:
            rows = B * S * S
            xr = torch.randn(rows, C, device="cuda")
            w, b = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda")
            gr = torch.randn(rows, C, device="cuda")
            _, mean, rstd = N.layernorm(xr, w, b, 1e-6)
            xa, wa, ba = xr.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
            ya = F.layer_norm(xa, (C,), wa, ba, 1e-6)

            def aten():
                torch.autograd.grad(ya, (xa, wa, ba), gr, retain_graph=True)

            r = compare({"aten": aten, "t3a": lambda: N.layernorm_backward_params(gr, xr, w, mean, rstd),
                         "m5_dx_only": lambda: N.layernorm_backward(gr, xr, w, mean, rstd)}, args.reps, args.iters)
            gb = 3 * rows * C * 4 / 1e9      # g and x read, dx written
            print(json.dumps({"what": "layernorm backward", "rows": rows, "C": C,
                              **{"us_" + k: [round(t, 1) for t in v] for k, v in r.items()},
                              "t3a_TBps": round(gb / r["t3a"][0] * 1e3, 2), "t3a_over_aten": round(r["t3a"][0] / r["aten"][0], 3)}),
                  flush=True)
    finally:
        M.TRAIN_NATIVE_BLOCKS = prev


if __name__ == "__main__":
    main()
