#!/usr/bin/env python3
"""PIR-AT outer steps on PSPNet-ResNet50 (tools/train_rob_seg.py's PSPNet recipe: 5-step PGD at eps = 4/255 on the eval
model, then the train-mode forward / backward of main_loss + 0.4 * aux_loss and the SGD step), device path against stock
PyTorch-ROCm (pspnet.USE_NATIVE = False), alternating step by step in one process on two copies of one seeded model:

    python devtools/psp_train_bench.py [--batch 8] [--size 473] [--classes 21] [--steps 10] [--warmup 2] [--t1 1]

Prints one JSON line per mode with the inner attack and the outer train step in ms (median, min, max over the timed
steps), and with ``--t1 1`` one line per T1 shape of layer3 / layer4 at this batch: forward and backward ms (device events
around the three launches of each direction) and the achieved rate on the algorithmic bytes, against 8 TB/s."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "robust-segmentation_amd")]

import torch  # noqa: E402

HBM = 8e12


def _model(C, seed=0):
    from devtools.psp_weights import seeded_state_dict
    from semseg.models import PSPNet
    torch.manual_seed(0)
    m = PSPNet(50, C)
    m.load_state_dict(seeded_state_dict(m.state_dict(), seed), strict=True)
    return m.cuda().train()


def _t1_lines(B, S):
    """T1 alone on the layer3 / layer4 maps (every BatchNorm there: 256 / 512 for bn1 / bn2, 1024 / 2048 for bn3 with the
    residual, and the plain downsample BatchNorm).  Algorithmic bytes: forward = the statistics pass reads x, the apply
    pass reads x [and r] and writes y; backward = the reduction reads g, x [and y], the dx pass reads g, x [and y] and
    writes dx [and g']."""
    from semseg import _native as N
    hw = (S - 1) // 8 + 1
    M = B * hw * hw
    cases = [(256, "relu"), (512, "relu"), (1024, "residual"), (2048, "residual"), (1024, "plain"), (2048, "plain")]
    g = torch.Generator().manual_seed(0)
    for C, mode in cases:
        relu, res = mode != "plain", mode == "residual"
        x = torch.randn(B, C, hw, hw, generator=g).cuda().contiguous(memory_format=torch.channels_last)
        r = torch.randn_like(x) if res else None
        gy = torch.randn_like(x)
        w, b = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")

        def fwd():
            return N.bn_train_forward(x, w, b, rm, rv, None, 1e-5, 0.1, relu, r)

        y, mean, invstd, scale = fwd()

        def bwd():
            return N.bn_train_backward(gy, x, y if relu else None, mean, invstd, scale, relu, res)

        out = {}
        for name, fn in (("fwd", fwd), ("bwd", bwd)):
            for _ in range(3):
                fn()
            reps = 20
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name] = e0.elapsed_time(e1) / reps
        mc = 4 * M * C
        fwd_bytes = mc * (3 + res)
        bwd_bytes = mc * (2 + relu + 3 + relu + res)
        print(json.dumps({"t1": True, "B": B, "M": M, "C": C, "mode": mode,
                          "fwd_ms": round(out["fwd"], 4), "fwd_GBps": round(fwd_bytes / out["fwd"] / 1e6, 1),
                          "fwd_of_8TBps": round(fwd_bytes / (out["fwd"] * 1e-3) / HBM, 3),
                          "bwd_ms": round(out["bwd"], 4), "bwd_GBps": round(bwd_bytes / out["bwd"] / 1e6, 1),
                          "bwd_of_8TBps": round(bwd_bytes / (out["bwd"] * 1e-3) / HBM, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=473)
    ap.add_argument("--classes", type=int, default=21)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--t1", type=int, default=1)
    args = ap.parse_args()

    from semseg.models import pspnet
    from semseg.val import Pgd_Attack_1
    from tools.train_rob_seg import psp_param_groups, set_psp_lr

    B, S, C = args.batch, args.size, args.classes
    assert (S - 1) % 8 == 0
    if args.t1:
        _t1_lines(B, S)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 3, S, S, generator=g).cuda()
    y = torch.randint(0, C, (B, S, S), generator=g).cuda()
    attack = Pgd_Attack_1(epsilon=4.0 / 255, alpha=1e-2, num_iter=5, los="pgd")
    total = args.warmup + args.steps
    runs = {}
    for mode in ("native", "stock"):
        model = _model(C)
        opt = torch.optim.SGD(psp_param_groups(model, 4e-4), 4e-4, momentum=0.9, weight_decay=1e-4)
        runs[mode] = dict(model=model, opt=opt, inner=[], outer=[], loss=None)

    def step(mode, i):
        rr = runs[mode]
        model, opt = rr["model"], rr["opt"]
        pspnet.USE_NATIVE = mode == "native"
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.manual_seed(1000 + i)
        ev[0].record()
        model.eval()
        x_adv = attack.adv_attack(model, x, y)[0]
        model.train()
        ev[1].record()
        opt.zero_grad(set_to_none=True)
        main_loss, aux_loss, _ = model(x_adv, y)
        loss = main_loss + 0.4 * aux_loss
        loss.backward()
        opt.step()
        set_psp_lr(opt, 4e-4, i, total)
        ev[2].record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            rr["inner"].append(ev[0].elapsed_time(ev[1]))
            rr["outer"].append(ev[1].elapsed_time(ev[2]))
        rr["loss"] = loss.item()

    try:
        for i in range(total):
            for mode in ("native", "stock"):
                step(mode, i)
    finally:
        pspnet.USE_NATIVE = True

    def st(v):
        return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}

    for mode, rr in runs.items():
        print(json.dumps({"model": "PSPNet_RN50", "mode": mode, "B": B, "size": S, "classes": C, "inner_pgd_steps": 5,
                          "timed_steps": len(rr["inner"]), "inner_attack_ms": st(rr["inner"]),
                          "outer_train_ms": st(rr["outer"]),
                          "step_ms": st([a + b for a, b in zip(rr["inner"], rr["outer"])]),
                          "last_loss": rr["loss"]}), flush=True)


if __name__ == "__main__":
    main()
