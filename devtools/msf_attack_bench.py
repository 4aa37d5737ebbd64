#!/usr/bin/env python3
"""One APGD step through multi-scale + flip, three ways, on random weights:

    python devtools/msf_attack_bench.py [--B 2] [--size 512 512] [--scales 0.5 0.75 1.0 1.25 1.5 1.75] [--no-flip]
                                        [--windows 5] [--iters 3] [--case upernet segmenter]

    wrapper  ``semseg.utils.msf_model.MsfModel(model)``: K10a, ``forward_lowres`` logits, K10b with the model's up-sampling
             inside; backward K10g, K10r', M2 backward, the model, K10a'
    fullres  the same wrapper with the hook hidden: ``model(x_s)`` logits, K10b / K10g / K10r' in full-res mode
    aten     the same protocol as ATen operations under autograd: ``F.interpolate(align_corners=True)``, ``model(x_s)``,
             ``flip``, ``F.interpolate``, ``softmax``, ``+``, then ``log(clamp_min(FLT_MIN))``

Every mode is a model handed to ``semseg.attacker.ApgdRun`` (loss mask-ce-avg, Linf, eps 8/255), which is stepped as
``apgd_train`` steps it (HIP-graph replay from the third step on).  The modes alternate inside one process: four warm-up
steps each, then ``--windows`` windows per mode of ``--iters`` steps between two device events; the figure is the median
window divided by ``--iters``, with the fastest and the slowest window beside it.  Memory: ``max_memory_allocated`` of one
eager forward + input gradient (seeded ``dz``) above what the inputs, the model and the wrapper's two buffers hold.
``max_abs_diff``: the modes' outputs and input gradients against each other on the same input.  A `#` header line, then one
JSON line per case."""
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

CASES = {"segmenter": "ade20k_segmenter.yaml", "upernet": "pascalvoc_convnext.yaml"}
FLT_MIN = float(torch.finfo(torch.float32).tiny)


class NoHook(torch.nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x):
        return self.model(x)


class AtenMsf(torch.nn.Module):
    """the wrapper's protocol in ATen operations"""

    def __init__(self, model, scales, flip):
        super().__init__()
        self.model, self.scales, self.flip = model, scales, flip

    def forward(self, x):
        from semseg.val import msf_scaled_size
        H, W = x.shape[2:]
        score = 0
        for s in self.scales:
            xs = F.interpolate(x, size=msf_scaled_size(s, H, W), mode="bilinear", align_corners=True)
            score = score + F.interpolate(self.model(xs), size=(H, W), mode="bilinear", align_corners=True).softmax(1)
            if self.flip:
                score = score + F.interpolate(self.model(xs.flip(3)).flip(3), size=(H, W), mode="bilinear",
                                              align_corners=True).softmax(1)
        return torch.log(score.clamp_min(FLT_MIN))


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


def forward_backward(m, x, dz):
    from semseg.attacker import _FrozenParameters
    xi = x.detach().clone().requires_grad_(True)
    with _FrozenParameters(m):
        out = m(xi)
    (g,) = torch.autograd.grad(out, [xi], dz)
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
    from semseg.utils.msf_model import MsfModel
    from tools.infer import build_model
    with open(os.path.join(ROOT, "robust-segmentation_amd", "configs", CASES[name])) as f:
        conf = yaml.load(f, Loader=yaml.SafeLoader)
    C = int(conf["EVAL"]["N_CLS"])
    torch.manual_seed(0)
    model = build_model(conf, random_init=True, device=dev)
    for p in model.parameters():
        p.requires_grad_(False)
    scales, flip, B = tuple(args.scales), not args.no_flip, args.B
    H, W = args.size
    gen = torch.Generator().manual_seed(1)
    x = torch.rand(B, 3, H, W, generator=gen).to(dev)
    dz = (torch.rand(B, C, H, W, generator=gen) * 2 - 1).to(dev)
    modes = {"wrapper": MsfModel(model, scales, flip, n_classes=C), "fullres": MsfModel(NoHook(model).eval(), scales, flip),
             "aten": AtenMsf(model, scales, flip).eval()}
    row = dict(case=name, model=conf["MODEL"]["NAME"], B=B, C=C, size=[H, W], scales=list(scales), flip=flip,
               passes=len(scales) * (2 if flip else 1), windows=args.windows, iters=args.iters)
    # same input, same dz: outputs of the three modes against each other, then the eager peak of each
    ref, diffs, peaks = None, {}, {}
    for m, mod in modes.items():
        out, g = forward_backward(mod, x, dz)                    # warm-up: weight-derived caches and the wrapper's buffers
        if ref is None:
            ref = (out.clone(), g)
        else:
            diffs[f"{m}_vs_wrapper"] = dict(z=float((out - ref[0]).abs().max()), grad=float((g - ref[1]).abs().max()))
        del out, g
        peaks[m] = round(peak_of(lambda: forward_backward(mod, x, dz)) / 2 ** 20, 1)
    row["max_abs_diff"] = diffs
    row["max_abs"] = dict(z=float(ref[0].abs().max()), grad=float(ref[1].abs().max()))
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
    ap.add_argument("--B", type=int, default=2)
    ap.add_argument("--size", type=int, nargs=2, default=[512, 512])
    ap.add_argument("--scales", type=float, nargs="+", default=[0.5, 0.75, 1.0, 1.25, 1.5, 1.75])
    ap.add_argument("--no-flip", action="store_true")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--case", nargs="+", default=["upernet", "segmenter"], choices=sorted(CASES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    print(f"# devtools/msf_attack_bench.py: B = {args.B}, input {args.size[0]} x {args.size[1]}, scales {args.scales}, flip "
          f"{not args.no_flip}, fp32, random weights; ms per APGD step (ApgdRun.step, mask-ce-avg, Linf), median / fastest / "
          f"slowest of {args.windows} windows of {args.iters} steps, modes alternating in one process; wrapper = MsfModel with "
          "forward_lowres (K10a, K10b low-res, K10g, K10r', M2 backward, K10a'), fullres = MsfModel on model(x_s) logits, aten = "
          "interpolate + model(x_s) + flip + interpolate + softmax + add + log under autograd; peak_MB = max_memory_allocated "
          "of one eager forward + input gradient above the inputs, the model and the wrapper's buffers", flush=True)
    for name in args.case:
        bench(name, args, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
