#!/usr/bin/env python3
"""evaluate_msf (K10a + K10b, fused with the final up-sampling) against the stock-PyTorch formulation of the same loop
(reference semseg/val.py:340-365: interpolate -> model -> [flip] -> interpolate -> softmax -> +=), B = 8, 512^2, six
scales + flip, random-init UperNet-ConvNeXt-T (C = 21) and Segmenter ViT-S (C = 151); then K10b alone on its byte model
(score read + written once: 2*B*C*H*W*4 bytes) as a fraction of the 8 TB/s HBM peak.

    python devtools/msf_bench.py [--steps 3] [--json out.json]"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "robust-segmentation_amd")
sys.path[:0] = [ROOT, PKG]
from semseg import _native as N  # noqa: E402
from semseg import val as V  # noqa: E402
from tools.infer import build_model  # noqa: E402

HBM_PEAK_GBS = 8000.0
SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)


@torch.no_grad()
def stock_msf(model, images, labels, C):
    B, H, W = labels.shape
    score = torch.zeros(B, C, H, W, device=images.device)
    for s in SCALES:
        size = V.msf_scaled_size(s, H, W)
        x = F.interpolate(images, size=size, mode="bilinear", align_corners=True)
        score += F.interpolate(model(x), size=(H, W), mode="bilinear", align_corners=True).softmax(1)
        score += F.interpolate(model(torch.flip(x, dims=(3,))).flip(3), size=(H, W), mode="bilinear",
                               align_corners=True).softmax(1)
    return score.argmax(1)


def wall_ms(fn, steps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), sorted(ts)[len(ts) // 2]


def event_us(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(5):
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3 / reps)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args()
    N.lib()
    dev = torch.device("cuda:0")
    B, H, W = 8, 512, 512
    out = {"B": B, "H": H, "W": W, "scales": SCALES, "flip": True, "models": {}, "k10b": []}
    for cfg_name in ("pascalvoc_convnext.yaml", "ade20k_segmenter.yaml"):
        with open(os.path.join(PKG, "configs", cfg_name)) as f:
            cfg = yaml.load(f, Loader=yaml.SafeLoader)
        C = int(cfg["EVAL"]["N_CLS"])
        torch.manual_seed(0)
        model = build_model(cfg, random_init=True, device=dev)
        for p in model.parameters():
            p.requires_grad_(False)
        g = torch.Generator(device="cuda").manual_seed(C)
        images = torch.rand(B, 3, H, W, generator=g, device=dev)
        labels = torch.randint(0, C, (B, H, W), generator=g, device=dev)
        batch = [(images, labels)]
        fused = wall_ms(lambda: V._evaluate_msf_metrics(model, batch, dev, SCALES, True, n_classes=C, ignore_label=-1),
                        args.steps)
        torch.cuda.reset_peak_memory_stats()
        V._evaluate_msf_metrics(model, batch, dev, SCALES, True, n_classes=C, ignore_label=-1)
        fused_peak = torch.cuda.max_memory_allocated() / 2 ** 30
        stock = wall_ms(lambda: stock_msf(model, images, labels, C), args.steps)
        torch.cuda.reset_peak_memory_stats()
        stock_msf(model, images, labels, C)
        stock_peak = torch.cuda.max_memory_allocated() / 2 ** 30
        r = {"C": C, "evaluate_msf_ms": fused, "stock_ms": stock, "evaluate_msf_peak_GiB": fused_peak,
             "stock_peak_GiB": stock_peak}
        out["models"][cfg_name] = r
        print(f"{cfg_name} C={C}: evaluate_msf min/median {fused[0]:.1f}/{fused[1]:.1f} ms per batch (peak {fused_peak:.2f} GiB)"
              f" | stock PyTorch {stock[0]:.1f}/{stock[1]:.1f} ms (peak {stock_peak:.2f} GiB)", flush=True)
        del model, images, labels, batch
        torch.cuda.empty_cache()
    # K10b alone at the largest scale (1.75 -> 896^2), flip on
    for C, r in ((21, 4), (21, 1), (151, 4), (151, 16), (151, 1)):
        Hs = 896
        logits = torch.randn(B, C, Hs // r, Hs // r, device=dev) * 3
        score = torch.zeros(B, C, H, W, device=dev)
        us = event_us(lambda: N.msf_accumulate(logits, score, (Hs, Hs), flip=True))
        nbytes = 2 * B * C * H * W * 4
        gbs = nbytes / (us * 1e-6) / 1e9
        moved = nbytes + logits.numel() * 4
        rec = {"C": C, "r": r, "us": us, "model_bytes": nbytes, "GBps": gbs, "frac_of_8TBps": gbs / HBM_PEAK_GBS,
               "frac_incl_logits_read": moved / (us * 1e-6) / 1e9 / HBM_PEAK_GBS}
        out["k10b"].append(rec)
        print(f"K10b C={C} r={r:2d} (896^2 -> 512^2): {us:8.1f} us, {gbs:7.0f} GB/s on 2*B*C*H*W*4 = "
              f"{100 * gbs / HBM_PEAK_GBS:.1f} % of 8 TB/s ({100 * rec['frac_incl_logits_read']:.1f} % counting the logits read)",
              flush=True)
        del logits, score
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
