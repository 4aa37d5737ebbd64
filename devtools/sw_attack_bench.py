#!/usr/bin/env python3
"""One APGD step through sliding windows, three ways, on random weights:

    python devtools/sw_attack_bench.py [--B 8] [--size 512 683] [--window 512] [--stride 512] [--windows 7] [--iters 5]
                                       [--case segmenter upernet]

    wrapper  ``segmenter_eval.SlidingWindowModel(model)``: K11c cut, ``forward_lowres`` window logits, K11a merge with the
             model's up-sampling inside; backward K11a' (low-res mode) and K11c'
    fullres  the same wrapper with the hook hidden: ``model(window)`` logits, K11a / K11a' in full-res mode
    aten     the same protocol as ATen operations under autograd: a stack of slices, ``model(window)`` (its own final
             up-sampling), a zero buffer and ``+=`` per window, ``/ count``

Every mode is a model handed to ``semseg.attacker.ApgdRun`` (loss mask-ce-avg, Linf, eps 8/255), which is stepped as
``apgd_train`` steps it (HIP-graph replay from the third step on).  The modes alternate inside one process: four warm-up
steps each, then ``--windows`` windows per mode of ``--iters`` steps between two device events; the figure is the median
window divided by ``--iters``, with the fastest and the slowest window beside it.  Memory: ``max_memory_allocated`` of one
eager forward + input gradient (seeded ``dlogits``) above what the inputs and the model hold.  ``max_abs_diff``: the
modes' logits and input gradients against each other on the same input.  A `#` header line, then one JSON line per case."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "robust-segmentation_amd")]

import torch  # noqa: E402
import yaml  # noqa: E402

CASES = {"segmenter": "ade20k_segmenter.yaml", "upernet": "pascalvoc_convnext.yaml"}


class NoHook(torch.nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x):
        return self.model(x)


class AtenSlidingWindow(torch.nn.Module):
    """the wrapper's protocol in ATen operations"""

    def __init__(self, model, ws, stride):
        super().__init__()
        self.model, self.ws, self.stride = model, ws, stride

    def forward(self, x):
        from semseg.utils.segmenter_eval import sw_anchors
        ws = self.ws
        ha, wa = sw_anchors(x.shape[2], x.shape[3], ws, self.stride)
        anchors = [(a, b) for a in ha for b in wa]
        crops = torch.stack([x[:, :, a:a + ws, b:b + ws] for a, b in anchors], 1).flatten(0, 1)
        seg = self.model(crops)
        seg = seg.view(x.shape[0], len(anchors), *seg.shape[1:])
        logit = torch.zeros(x.shape[0], seg.shape[2], x.shape[2], x.shape[3], device=x.device)
        count = torch.zeros(1, 1, x.shape[2], x.shape[3], device=x.device)
        for k, (a, b) in enumerate(anchors):
            logit[:, :, a:a + ws, b:b + ws] += seg[:, k]
            count[:, :, a:a + ws, b:b + ws] += 1
        return logit / count


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def summary(ts):
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3))


def forward_backward(m, x, dl):
    from semseg.attacker import _FrozenParameters
    xi = x.detach().clone().requires_grad_(True)
    with _FrozenParameters(m):
        out = m(xi)
    (g,) = torch.autograd.grad(out, [xi], dl)
    return out.detach(), g


def peak_of(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def bench(name, args, dev):
    from semseg import attacker as A
    from semseg.utils.segmenter_eval import SlidingWindowModel, sw_anchors
    from tools.infer import build_model
    with open(os.path.join(ROOT, "robust-segmentation_amd", "configs", CASES[name])) as f:
        conf = yaml.load(f, Loader=yaml.SafeLoader)
    C = int(conf["EVAL"]["N_CLS"])
    torch.manual_seed(0)
    model = build_model(conf, random_init=True, device=dev)
    for p in model.parameters():
        p.requires_grad_(False)
    ws, stride, B = args.window, args.stride, args.B
    H, W = args.size
    gen = torch.Generator().manual_seed(1)
    x = torch.rand(B, 3, H, W, generator=gen).to(dev)
    dl = torch.randn(B, C, H, W, generator=gen).to(dev)
    ha, wa = sw_anchors(H, W, ws, stride)
    modes = {"wrapper": SlidingWindowModel(model, ws, stride), "fullres": SlidingWindowModel(NoHook(model).eval(), ws, stride),
             "aten": AtenSlidingWindow(model, ws, stride).eval()}
    row = dict(case=name, model=conf["MODEL"]["NAME"], B=B, C=C, size=[H, W], window=ws, stride=stride,
               n_win=len(ha) * len(wa), windows=args.windows, iters=args.iters)
    # same input, same dlogits: outputs of the three modes against each other, then the eager peak of each
    ref, diffs, peaks = None, {}, {}
    for m, mod in modes.items():
        out, g = forward_backward(mod, x, dl)                    # warm-up: weight-derived caches are built once
        if ref is None:
            ref = (out, g)
        else:
            diffs[f"{m}_vs_wrapper"] = dict(logits=float((out - ref[0]).abs().max()), grad=float((g - ref[1]).abs().max()))
        del out, g
        peaks[m] = round(peak_of(lambda: forward_backward(mod, x, dl)) / 2 ** 20, 1)
    row["max_abs_diff"] = diffs
    row["max_abs"] = dict(logits=float(ref[0].abs().max()), grad=float(ref[1].abs().max()))
    del ref
    with torch.no_grad():
        y = modes["wrapper"](x).max(1)[1]
    weights = torch.ones(C, device=dev)
    n_steps = 4 + args.windows * args.iters
    runs, pos = {}, {}
    for m, mod in modes.items():
        run = A.ApgdRun(mod, x, y, 8.0 / 255, max(n_steps + 2, A.GRAPH_MIN_ITER), "mask-ce-avg", "ce-avg", True, C, weights,
                        x.clone())
        run.start()
        for i in range(4):
            run.step(i)
        runs[m], pos[m] = run, 4
    torch.cuda.synchronize()
    row["graph_replay"] = {m: r.graphs is not None for m, r in runs.items()}

    def stepper(m):
        def step():
            runs[m].step(pos[m])
            pos[m] += 1
        return step

    times = {m: [] for m in modes}
    for _ in range(args.windows):
        for m in modes:
            times[m].append(window(stepper(m), args.iters))
    for m, run in runs.items():
        run.release_graphs()
        A.release_graph_cache(modes[m])
        row[m] = dict(summary(times[m]), peak_MB=peaks[m])
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=[512, 683])
    ap.add_argument("--window", type=int, default=512)
    ap.add_argument("--stride", type=int, default=512)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--case", nargs="+", default=["segmenter", "upernet"], choices=sorted(CASES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    print(f"# devtools/sw_attack_bench.py: B = {args.B}, input {args.size[0]} x {args.size[1]}, window {args.window}, stride "
          f"{args.stride}, fp32, random weights; ms per APGD step (ApgdRun.step, mask-ce-avg, Linf), median / fastest / slowest "
          f"of {args.windows} windows of {args.iters} steps, modes alternating in one process; wrapper = SlidingWindowModel "
          "with forward_lowres (K11c, K11a, K11a' low-res, K11c'), fullres = SlidingWindowModel on model(window) logits, aten "
          "= slice stack + model(window) + zero buffer, += per window, / count under autograd; peak_MB = max_memory_allocated "
          "of one eager forward + input gradient above the inputs and the model", flush=True)
    for name in args.case:
        bench(name, args, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
