#!/usr/bin/env python3
"""Sliding-window clean evaluation (semseg.val.evaluate_sliding; reference semseg/utils/segmenter_eval.py) from the
command line.

    python -m tools.eval_sliding --cfg configs/ade20k_segmenter.yaml --data val.pt --flip
    python -m tools.eval_sliding --cfg configs/ade20k_segmenter.yaml --synthetic 8 --image_size 512 683 --json out.json

Data as in tools.eval_msf: ``--data file.pt`` = {images (N,3,H,W) float in [0,1], labels (N,H,W) int64, -1 = ignore}, or
``--synthetic N`` seeded random images of ``--image_size H W`` (need not be square) with random weights whose labels are the
model's single-pass clean prediction.  The window size and stride default to ``window_size`` / ``window_stride`` of
configs/segmenter.yml for a SegMenter config and to ``EVAL.IMAGE_SIZE[0]`` otherwise.  Prints the per-class table and
aAcc / mAcc / mIoU (percent)."""
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


def default_window(cfg):
    """(window_size, window_stride) of a config: the Segmenter dataset defaults, else the evaluation size"""
    if cfg["MODEL"]["NAME"] == "SegMenter":
        from semseg.utils.utils import load_config_segmenter
        ds = load_config_segmenter(backbone=cfg["MODEL"]["BACKBONE"], n_cls=cfg["EVAL"]["N_CLS"])[1]
        return int(ds["window_size"]), int(ds["window_stride"])
    size = int(cfg["EVAL"]["IMAGE_SIZE"][0])
    return size, size


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", type=str, default="configs/ade20k_segmenter.yaml")
    ap.add_argument("--synthetic", type=int, default=0, help="evaluate N synthetic images (random weights)")
    ap.add_argument("--data", type=str, default=None, help=".pt file with {'images','labels'}")
    ap.add_argument("--random_init", action="store_true", help="seeded random weights instead of EVAL.MODEL_PATH")
    ap.add_argument("--image_size", type=int, nargs=2, default=None, metavar=("H", "W"), help="synthetic image size")
    ap.add_argument("--window_size", type=int, default=None)
    ap.add_argument("--window_stride", type=int, default=None)
    ap.add_argument("--flip", action="store_true")
    ap.add_argument("--batch_size", type=int, default=None, help="images per batch = windows per model call")
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
    ws, stride = default_window(cfg)
    ws = args.window_size or ws
    stride = args.window_stride or stride
    device = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    model = build_model(cfg, random_init=bool(args.synthetic) or args.random_init, device=device)
    for p in model.parameters():
        p.requires_grad_(False)

    if args.synthetic:
        H, W = args.image_size or (int(test_cfg["IMAGE_SIZE"][0]),) * 2
        g = torch.Generator().manual_seed(1234)
        images = torch.rand(args.synthetic, 3, H, W, generator=g)
        with torch.no_grad():
            labels = torch.cat([model(images[i:i + bs].to(device)).argmax(1).cpu() for i in range(0, len(images), bs)])
    else:
        blob = torch.load(args.data, map_location="cpu")
        images, labels = blob["images"].float(), blob["labels"].long()
    batches = [(images[i:i + bs], labels[i:i + bs]) for i in range(0, len(images), bs)]

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    metrics = V._evaluate_sliding_metrics(model, batches, device, ws, stride, batch_size=bs, flip=args.flip, n_classes=C,
                                          ignore_label=ignore)
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    ious, miou = metrics.compute_iou()
    acc, macc, aacc = metrics.compute_pixel_acc()
    f1, mf1 = metrics.compute_f1()
    print(f"{'class':>6} {'IoU':>7} {'Acc':>7} {'F1':>7}")
    for c in range(C):
        print(f"{c:>6} {ious[c]:>7.2f} {acc[c]:>7.2f} {f1[c]:>7.2f}")
    print(f"aAcc {float(aacc):.2f}  mAcc {macc:.2f}  mIoU {miou:.2f}  mF1 {mf1:.2f}   "
          f"({len(images)} images {tuple(images.shape[2:])}, window {ws}, stride {stride}, flip {args.flip}, {secs:.2f} s)")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"aAcc": float(aacc), "mAcc": macc, "mIoU": miou, "mF1": mf1, "IoU": ious, "Acc": acc, "F1": f1,
                       "window_size": ws, "window_stride": stride, "flip": args.flip, "n_images": len(images),
                       "image_size": list(images.shape[2:]), "seconds": secs}, f, indent=1)


if __name__ == "__main__":
    main()
