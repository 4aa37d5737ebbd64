#!/usr/bin/env python3
"""Multi-scale + flip clean evaluation (semseg.val.evaluate_msf; reference semseg/val.py:330-372) from the command line.

    python -m tools.eval_msf --cfg configs/pascalvoc_convnext.yaml --data val.pt --flip
    python -m tools.eval_msf --cfg configs/ade20k_segmenter.yaml --synthetic 16 --flip --json out.json

Data as in tools.infer: ``--data file.pt`` = {images (N,3,H,W) float in [0,1], labels (N,H,W) int64, -1 = ignore}, or
``--synthetic N`` seeded random images with random weights whose labels are the model's single-scale clean prediction.
Prints the per-class table and aAcc / mAcc / mIoU (percent)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from semseg import val as V  # noqa: E402
from tools.infer import build_model  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", type=str, default="configs/pascalvoc_convnext.yaml")
    ap.add_argument("--synthetic", type=int, default=0, help="evaluate N synthetic images (random weights)")
    ap.add_argument("--data", type=str, default=None, help=".pt file with {'images','labels'}")
    ap.add_argument("--random_init", action="store_true", help="seeded random weights instead of EVAL.MODEL_PATH")
    ap.add_argument("--scales", type=float, nargs="+", default=[0.5, 0.75, 1.0, 1.25, 1.5, 1.75])
    ap.add_argument("--flip", action="store_true")
    ap.add_argument("--batch_size", type=int, default=None)
    ap.add_argument("--image_size", type=int, default=None)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args(argv)
    if not args.synthetic and not args.data:
        ap.error("one of --synthetic N / --data file.pt is required")

    with open(args.cfg) as f:
        cfg = yaml.load(f, Loader=yaml.SafeLoader)
    test_cfg = cfg["EVAL"]
    C = int(test_cfg["N_CLS"])
    ignore = int(cfg.get("DATASET", {}).get("IGNORE_LABEL", -1))
    bs = args.batch_size or int(test_cfg["BATCH_SIZE"])
    device = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    model = build_model(cfg, random_init=bool(args.synthetic) or args.random_init, device=device)
    for p in model.parameters():
        p.requires_grad_(False)

    if args.synthetic:
        size = args.image_size or int(test_cfg["IMAGE_SIZE"][0])
        g = torch.Generator().manual_seed(1234)
        images = torch.rand(args.synthetic, 3, size, size, generator=g)
        with torch.no_grad():
            labels = torch.cat([model(images[i:i + bs].to(device)).argmax(1).cpu() for i in range(0, len(images), bs)])
    else:
        blob = torch.load(args.data, map_location="cpu")
        images, labels = blob["images"].float(), blob["labels"].long()
    batches = [(images[i:i + bs], labels[i:i + bs]) for i in range(0, len(images), bs)]

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    metrics = V._evaluate_msf_metrics(model, batches, device, args.scales, args.flip, n_classes=C, ignore_label=ignore)
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    ious, miou = metrics.compute_iou()
    acc, macc, aacc = metrics.compute_pixel_acc()
    f1, mf1 = metrics.compute_f1()
    print(f"{'class':>6} {'IoU':>7} {'Acc':>7} {'F1':>7}")
    for c in range(C):
        print(f"{c:>6} {ious[c]:>7.2f} {acc[c]:>7.2f} {f1[c]:>7.2f}")
    print(f"aAcc {float(aacc):.2f}  mAcc {macc:.2f}  mIoU {miou:.2f}  mF1 {mf1:.2f}   "
          f"({len(images)} images, scales {args.scales}, flip {args.flip}, {secs:.2f} s)")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"aAcc": float(aacc), "mAcc": macc, "mIoU": miou, "mF1": mf1, "IoU": ious, "Acc": acc, "F1": f1,
                       "scales": args.scales, "flip": args.flip, "n_images": len(images), "seconds": secs}, f, indent=1)


if __name__ == "__main__":
    main()
