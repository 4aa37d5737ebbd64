#!/usr/bin/env python3
"""PSPNet's training criterion in the three modes of ``semseg.models.pspnet.TRAIN_CRITERION``: event-timed forward + backward
of the two-head tail alone, then of the whole training forward + backward of PSPNet-ResNet50.

    python devtools/psp_criterion_bench.py [--B 8] [--size 473] [--C 21] [--windows 9] [--iters 20] [--steps 7]

Tail: two (B, C, h, h) fp32 low-resolution logits tensors (h = (size - 1) / 8 + 1; ``z_y += 6`` on 70 % of the pixels of a
blocky label map, 5 % of the labels ignored), loss = CE(main) + 0.4 CE(aux) with ``nn.CrossEntropyLoss(ignore_index=-1)``:

    torch   P2 (``upsample_ac``) on both heads + nn.CrossEntropyLoss         (the default)
    native  P2 on both heads + T2                                            (``CrossEntropy(native=True)``)
    fused   T2u-ac on the low-resolution logits                              (``.upsampled(..., align_corners=True)``)

The modes alternate inside one process: two warm-up passes each, then ``--windows`` windows per mode of ``--iters`` forward +
backward passes between two device events; the figure is the median window divided by ``--iters``, with the fastest and the
slowest window beside it.  Memory: ``torch.cuda.max_memory_allocated`` over one pass above what the inputs hold.

Model: ``PSPNet(50, C)`` in training mode, B x 3 x size x size, forward + backward with ``loss = main + 0.4 aux`` (no
attack, no optimizer), the modes alternating, two warm-up steps each, ``--steps`` timed steps each between device events;
median, and the peak allocation of one step with the parameter gradients freed before it.  A `#` header line, then one
JSON line per part."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "robust-segmentation_amd")]

import torch  # noqa: E402

MODES = ("torch", "native", "fused")


def make(C, B, S, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    h = (S - 1) // 8 + 1
    yl = torch.randint(0, C, (B, h, h), generator=g, device=dev)
    z = torch.randn(B, C, h, h, generator=g, device=dev) * 3
    z.scatter_add_(1, yl[:, None], ((torch.rand(B, h, h, generator=g, device=dev) < 0.7).float() * 6.0)[:, None])
    y = yl.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :S, :S].contiguous()
    y[torch.rand(B, S, S, generator=g, device=dev) < 0.05] = -1
    return z.requires_grad_(True), y


def window(fn, leaves, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        for t in leaves:
            t.grad = None
        fn().backward()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def peak_of(fn, leaves):
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn().backward()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def summary(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def bench_tail(args, dev):
    from semseg import _native as N
    from semseg.losses import CrossEntropy
    from semseg.models.pspnet import _up_ac_train
    x, y = make(args.C, args.B, args.size, dev, 1)
    a = make(args.C, args.B, args.size, dev, 2)[0]
    size = tuple(y.shape[-2:])
    stock = torch.nn.CrossEntropyLoss(ignore_index=-1)
    crit = CrossEntropy(-1, native=True).to(dev)
    assert N.train_ce_up_supported(x, size, align_corners=True), "no T2u-ac plan for this shape: nothing fused to measure"
    fns = {"torch": lambda: stock(_up_ac_train(x, size), y) + 0.4 * stock(_up_ac_train(a, size), y),
           "native": lambda: crit(_up_ac_train(x, size), y) + 0.4 * crit(_up_ac_train(a, size), y),
           "fused": lambda: (crit.upsampled(x, y, align_corners=True) + 0.4 * crit.upsampled(a, y, align_corners=True))}
    leaves = (x, a)
    with torch.no_grad():
        loss = {m: float(fns[m]()) for m in MODES}
    for m in MODES:
        window(fns[m], leaves, 2)
    times = {m: [] for m in MODES}
    for _ in range(args.windows):
        for m in MODES:
            times[m].append(window(fns[m], leaves, args.iters))
    h = x.shape[-1]
    row = dict(part="tail", B=args.B, C=args.C, low=h, size=args.size, windows=args.windows, iters=args.iters,
               tile=N.train_ce_up_tile(args.C, h, h, args.size, args.size, align_corners=True), loss=loss)
    for m in MODES:
        row[m] = dict(summary(times[m]), peak_MB=round(peak_of(fns[m], leaves) / 2 ** 20, 1))
    row["torch_over_fused"] = round(row["torch"]["median_ms"] / row["fused"]["median_ms"], 3)
    row["native_over_fused"] = round(row["native"]["median_ms"] / row["fused"]["median_ms"], 3)
    print(json.dumps(row), flush=True)


def bench_model(args, dev):
    from semseg.models import PSPNet, pspnet
    torch.manual_seed(0)
    model = PSPNet(50, args.C).to(dev).train()
    g = torch.Generator().manual_seed(3)
    x = torch.rand(args.B, 3, args.size, args.size, generator=g).to(dev)
    y = make(args.C, args.B, args.size, dev, 4)[1]

    def step(mode):
        prev, pspnet.TRAIN_CRITERION = pspnet.TRAIN_CRITERION, mode
        try:
            model.zero_grad(set_to_none=True)
            main, aux, _ = model(x, y)
            loss = main + 0.4 * aux
            loss.backward()
            return loss.detach()
        finally:
            pspnet.TRAIN_CRITERION = prev

    def timed(mode):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        e0.record()
        loss = step(mode)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), torch.cuda.max_memory_allocated(), float(loss)

    for m in MODES:
        for _ in range(2):
            step(m)
    times, peaks, loss = {m: [] for m in MODES}, {m: 0 for m in MODES}, {}
    for _ in range(args.steps):
        for m in MODES:
            t, peak, loss[m] = timed(m)
            times[m].append(t)
            peaks[m] = max(peaks[m], peak)
    row = dict(part="model", model="PSPNet-RN50", B=args.B, C=args.C, size=args.size, steps=args.steps, last_loss=loss)
    for m in MODES:
        row[m] = dict(summary(times[m]), peak_MB=round(peaks[m] / 2 ** 20, 1))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--C", type=int, default=21)
    ap.add_argument("--size", type=int, default=473)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    assert (args.size - 1) % 8 == 0, "PSPNet needs (size - 1) % 8 == 0"
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    print(f"# devtools/psp_criterion_bench.py: B = {args.B}, C = {args.C}, {(args.size - 1) // 8 + 1}^2 -> {args.size}^2, fp32; ms "
          f"per forward + backward, median / fastest / slowest of {args.windows} windows of {args.iters} (tail) and of "
          f"{args.steps} steps (model), modes alternating in one process; torch = P2 + nn.CrossEntropyLoss, native = P2 + T2, "
          "fused = T2u-ac on the low-resolution logits; peak_MB: tail = max_memory_allocated above the inputs, model = "
          "max_memory_allocated of one step", flush=True)
    bench_tail(args, dev)
    if not args.skip_model:
        bench_model(args, dev)


if __name__ == "__main__":
    main()
