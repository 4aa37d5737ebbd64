#!/usr/bin/env python3
"""Sliding-window evaluation of one batch, three ways, on random weights:

    python devtools/sw_bench.py [--B 8] [--size 512 683] [--window 512] [--windows 7] [--iters 3] [--case segmenter upernet]

    fused    ``segmenter_eval.inference`` with the model's ``forward_lowres`` hook: low-resolution window logits, K11a
             (merge + softmax, the model's up-sampling inside)
    fullres  the same function with the hook hidden: ``model(window)`` logits, K11a on full-resolution windows
    aten     ``model(window)`` logits, then the reference's ``merge_windows`` as ATen operations on device tensors, image
             by image (zeros, += per window, count, divide, F.interpolate, softmax)

Cases: ``segmenter`` = ViT-S/16 Segmenter, C = 151, stride = window; ``upernet`` = UperNet-ConvNeXt-T, C = 21, stride =
window / 2.  Besides the whole batch, the merge alone is timed on the logits of one forward (``merge_*``).

The modes alternate inside one process: two warm-up passes each, then ``--windows`` windows per mode of ``--iters`` passes
between two device events; the figure is the median window divided by ``--iters``, with the fastest and the slowest window
beside it.  Memory: ``torch.cuda.max_memory_allocated`` over one pass above what the inputs and the model hold.  A `#`
header line, then one JSON line per case."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "robust-segmentation_amd")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import yaml  # noqa: E402

CASES = {"segmenter": ("ade20k_segmenter.yaml", 1), "upernet": ("pascalvoc_convnext.yaml", 2)}


class NoHook(torch.nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x):
        return self.model(x)


def aten_merge(seg_maps, anchors, ws, shape, ori_shape, n_img):
    """the reference's merge_windows, image by image, on device tensors"""
    n_win = len(anchors)
    C = seg_maps.shape[1]
    H, W = shape
    out = []
    for b in range(n_img):
        logit = torch.zeros((C, H, W), device=seg_maps.device)
        count = torch.zeros((1, H, W), device=seg_maps.device)
        for window, (ha, wa) in zip(seg_maps[b * n_win:(b + 1) * n_win], anchors):
            logit[:, ha:ha + ws, wa:wa + ws] += window
            count[:, ha:ha + ws, wa:wa + ws] += 1
        logit = logit / count
        logit = F.interpolate(logit.unsqueeze(0), ori_shape, mode="bilinear")[0]
        out.append(F.softmax(logit, 0))
    return torch.stack(out)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def peak_of(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def summary(ts):
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3))


def alternate(fns, windows, iters):
    for f in fns.values():
        window(f, 2)
    times = {m: [] for m in fns}
    for _ in range(windows):
        for m, f in fns.items():
            times[m].append(window(f, iters))
    return {m: dict(summary(times[m]), peak_MB=round(peak_of(fns[m]) / 2 ** 20, 1)) for m in fns}


@torch.no_grad()
def bench(name, args, dev):
    from semseg import _native as N
    from semseg.utils.segmenter_eval import inference, sw_anchors
    from tools.infer import build_model
    cfg_name, div = CASES[name]
    with open(os.path.join(ROOT, "robust-segmentation_amd", "configs", cfg_name)) as f:
        conf = yaml.load(f, Loader=yaml.SafeLoader)
    C = int(conf["EVAL"]["N_CLS"])
    torch.manual_seed(0)
    model = build_model(conf, random_init=True, device=dev)
    for p in model.parameters():
        p.requires_grad_(False)
    plain = NoHook(model)
    ws, stride, B = args.window, args.window // div, args.B
    H, W = args.size
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    ha, wa = sw_anchors(H, W, ws, stride)
    anchors = [(a, b) for a in ha for b in wa]
    n_win = len(anchors)
    crops = torch.stack([x[:, :, a:a + ws, b:b + ws] for a, b in anchors], 1).flatten(0, 1).contiguous()

    def aten():
        seg = torch.empty(B * n_win, C, ws, ws, device=dev)
        for i in range(0, B * n_win, B):
            seg[i:i + B] = model(crops[i:i + B])
        return aten_merge(seg, anchors, ws, (H, W), (H, W), B)

    fns = {"fused": lambda: inference(model, x, ws, stride, B, n_cls=C),
           "fullres": lambda: inference(plain, x, ws, stride, B, n_cls=C), "aten": aten}
    p_f, p_p, p_a = fns["fused"](), fns["fullres"](), fns["aten"]()
    row = dict(case=name, model=conf["MODEL"]["NAME"], B=B, C=C, size=[H, W], window=ws, stride=stride, n_win=n_win,
               windows=args.windows, iters=args.iters,
               max_abs_diff=dict(fused_vs_fullres=float((p_f - p_p).abs().max()), fullres_vs_aten=float((p_p - p_a).abs().max())))
    del p_f, p_p, p_a
    row.update(alternate(fns, args.windows, args.iters))
    # the merge alone, on the logits of one forward
    low = torch.cat([model.forward_lowres(crops[i:i + B])[0].float() for i in range(0, B * n_win, B)]).contiguous()
    full = torch.cat([model(crops[i:i + B]) for i in range(0, B * n_win, B)]).contiguous()
    out = torch.empty(B, C, H, W, device=dev)
    merges = {"merge_fused": lambda: N.sw_merge(low, ws, ha, wa, (H, W), softmax=True, out=out),
              "merge_fullres": lambda: N.sw_merge(full, ws, ha, wa, (H, W), softmax=True, out=out),
              "merge_aten": lambda: aten_merge(full, anchors, ws, (H, W), (H, W), B)}
    row["low"] = list(low.shape[2:])
    row.update(alternate(merges, args.windows, max(args.iters, 10)))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=[512, 683])
    ap.add_argument("--window", type=int, default=512)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--case", nargs="+", default=["segmenter", "upernet"], choices=sorted(CASES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    print(f"# devtools/sw_bench.py: B = {args.B}, input {args.size[0]} x {args.size[1]}, window {args.window}, fp32, random "
          f"weights; ms per batch, median / fastest / slowest of {args.windows} windows of {args.iters} passes (merge_*: of "
          f"{max(args.iters, 10)}), modes alternating in one process; fused = inference with forward_lowres (K11a on "
          "low-resolution logits), fullres = inference on model(window) logits (K11a), aten = model(window) + the reference's "
          "merge_windows as ATen operations; merge_* = the merge alone on the logits of one forward; peak_MB = "
          "max_memory_allocated of one pass above the inputs and the model", flush=True)
    for name in args.case:
        bench(name, args, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
