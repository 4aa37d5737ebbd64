#!/usr/bin/env python3
"""Milliseconds per APGD step on PSPNet-ResNet50 (mask-ce-bal, Linf, random-init weights), device path against the stock
PyTorch-ROCm forward / backward of the same module (pspnet.USE_NATIVE = False):

    python devtools/psp_bench.py [--batch 8] [--size 473] [--classes 21] [--steps 10] [--warmup 3] [--graph 1]

Prints one JSON line per mode, with the model-side roofline line: about 0.3 TFLOP per 473 x 473 image for the forward
(cls 3x3 0.14, layer4 0.10, layer3 0.05) and about the same again for the input gradient."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "robust-segmentation_amd")]

import torch  # noqa: E402


def _flops_per_image(model, size):
    """multiply-adds x 2 of every convolution of one forward at ``size`` x ``size`` (hooks on a CPU meta pass)"""
    total = [0]

    def hook(m, inp, out):
        k = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
        total[0] += 2 * out.shape[1] * out.shape[2] * out.shape[3] * k

    hs = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, torch.nn.Conv2d)]
    with torch.no_grad():
        model.to("meta")(torch.empty(1, 3, size, size, device="meta"))
    for h in hs:
        h.remove()
    return total[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=473)
    ap.add_argument("--classes", type=int, default=21)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--graph", type=int, default=1)
    ap.add_argument("--modes", type=str, default="native,stock")
    args = ap.parse_args()

    from semseg import attacker as A
    from semseg.models import PSPNet, pspnet
    from semseg.utils.utils import VOC_WTS

    B, S, C = args.batch, args.size, args.classes
    flops = _flops_per_image(PSPNet(50, C).eval(), S)
    torch.manual_seed(0)
    model = PSPNet(50, C).eval().cuda()
    for p in model.parameters():
        p.requires_grad_(False)
    x = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        y = model(x).max(1)[1]
    w = torch.tensor(VOC_WTS, device="cuda")[:C] if C == 21 else torch.ones(C, device="cuda")
    A.USE_HIP_GRAPH = bool(args.graph)
    for mode in args.modes.split(","):
        pspnet.USE_NATIVE = mode == "native"
        A.release_graph_cache(model)
        W, K = args.warmup, args.steps
        run = A.ApgdRun(model, x, y, 8.0 / 255, max(W + K + 1, A.GRAPH_MIN_ITER), "mask-ce-bal", "ce-avg", True, C, w,
                        x.clone())
        run.start()
        for i in range(W):
            run.step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(W, W + K):
            run.step(i)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / K
        tflops = 2 * flops * B / (ms * 1e-3) / 1e12      # forward + input gradient
        print(json.dumps({"model": "PSPNet_RN50", "mode": mode, "B": B, "size": S, "classes": C, "graph": bool(args.graph),
                          "ms_per_step": round(ms, 3), "fwd_tflop_per_image": round(flops / 1e12, 4),
                          "model_tflops": round(tflops, 1)}), flush=True)
    pspnet.USE_NATIVE = True
    A.release_graph_cache(model)


if __name__ == "__main__":
    main()
