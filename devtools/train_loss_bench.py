#!/usr/bin/env python3
"""T2 (csrc/train_loss.hip) against the stock device criterion: event-timed forward + backward at the training size.

    python devtools/train_loss_bench.py [--pairs 7] [--B 8] [--size 512]

B x C x size x size logits (C = 21 and 151, fp32 and bf16, ``z_y += 6`` on 70 % of the pixels, 5 % ignored), CrossEntropy
and OhemCrossEntropy in both regimes (top-k: confident logits).  T2 and stock alternate inside one process; per row the
minimum over the pairs and the second-smallest time, the share of 8 TB/s on T2's byte model (forward B*H*W*(C*s + 12),
backward B*H*W*(2*C*s + 12), s = bytes per logit; not counted: the OHEM select's four histogram passes, sum pass and
mark pass over the 4-byte plane), the bytes the kernels actually move (for C > 32 the backward reads the logits twice:
3*C*s + 12) with the share on those, and the peak allocation of each (torch.cuda.max_memory_allocated, above what the inputs hold).  One JSON line per row."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "robust-segmentation_amd")]

import torch  # noqa: E402


def make(C, B, S, dtype, confident, dev):
    g = torch.Generator(device=dev).manual_seed(C)
    y = torch.randint(0, C, (B, S, S), generator=g, device=dev)
    z = torch.randn(B, C, S, S, generator=g, device=dev) * 3
    frac, boost = (0.995, 12.0 + 2.5 * math.log(C)) if confident else (0.7, 6.0)
    z.scatter_add_(1, y[:, None], ((torch.rand(B, S, S, generator=g, device=dev) < frac).float() * boost)[:, None])
    y[torch.rand(B, S, S, generator=g, device=dev) < 0.05] = -1
    return z.to(dtype).requires_grad_(True), y


def step(mod, z, y):
    z.grad = None
    mod(z, y).backward()


def timed(mod, z, y):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    step(mod, z, y)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args()
    assert args.pairs >= 5
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from semseg.losses import CrossEntropy, OhemCrossEntropy
    dev = torch.device("cuda:0")
    for C in (21, 151):
        for dtype in (torch.float32, torch.bfloat16):
            for kind, confident in (("CrossEntropy", False), ("Ohem/threshold", False), ("Ohem/top-k", True)):
                z, y = make(C, args.B, args.size, dtype, confident, dev)
                cls = CrossEntropy if kind == "CrossEntropy" else OhemCrossEntropy
                mods = {"t2": cls(-1, native=True).to(dev), "stock": cls(-1).to(dev)}
                for m in mods.values():      # warm-up: code objects, allocator
                    step(m, z, y)
                    step(m, z, y)
                times, peaks = {"t2": [], "stock": []}, {"t2": 0, "stock": 0}
                for _ in range(args.pairs):
                    for name, m in mods.items():
                        t, peak = timed(m, z, y)
                        times[name].append(t)
                        peaks[name] = max(peaks[name], peak)
                s = z.element_size()
                n = args.B * args.size * args.size
                model = n * (C * s + 12) + n * (2 * C * s + 12)
                moved = model + (n * C * s if C > 32 else 0) + (n * 4 * 7 if kind != "CrossEntropy" else 0)
                row = dict(kernel="T2", criterion=kind, C=C, dtype=str(dtype).split(".")[-1], B=args.B, size=args.size,
                           model_bytes=model, moved_bytes_upper=moved)
                for name in ("t2", "stock"):
                    ts = sorted(times[name])
                    row[f"{name}_us_min"], row[f"{name}_us_2nd"] = round(ts[0], 1), round(ts[1], 1)
                    row[f"{name}_peak_MB"] = round(peaks[name] / 2 ** 20, 1)
                row["t2_share_of_8TBs"] = round(model / (row["t2_us_min"] * 1e-6) / 8e12, 3)
                row["t2_share_of_8TBs_moved"] = round(moved / (row["t2_us_min"] * 1e-6) / 8e12, 3)
                row["stock_over_t2"] = round(row["stock_us_min"] / row["t2_us_min"], 2)
                print(json.dumps(row), flush=True)
                del z, y, mods


if __name__ == "__main__":
    main()
