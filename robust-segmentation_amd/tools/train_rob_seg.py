#!/usr/bin/env python3
"""PIR-AT adversarial fine-tuning step (counterpart of tools/train_rob_seg.py:283-363), MI355X-native.

    python -m tools.train_rob_seg --cfg configs/ade20k_convnext.yaml --synthetic 64 --steps 20     # 1 GPU
    torchrun --nproc-per-node 8 -m tools.train_rob_seg --cfg ... --synthetic 512 --steps 50         # DDP/RCCL

One outer step = [N_ITERS-step PGD on the current model (eval mode)] + [forward/backward on the
adversarial batch + optimizer + LR schedule].  What differs from the reference:
  * the inner attack never touches parameter gradients: it differentiates w.r.t. the input only
    (semseg.val.Pgd_Attack_1 -> K2 + K6 kernels), on the un-wrapped ``model.module``; the reference's
    ``loss.backward()`` inside the attack accumulates into ``.grad`` after ``zero_grad`` and, under DDP,
    all-reduces ~240 MB of gradients on EVERY inner step.  Here the only collective
    is DDP's bucketed gradient all-reduce of the outer step, once per step, over RCCL/xGMI;
  * ``Pgd_Attack(epsilon=...)`` of the reference raises TypeError (D1) and ``los="pgd"`` IndexError
    (D2): the runnable "N-step CE PGD" is Pgd_Attack_1, used here for ATTACK=pgd / LOSS_FN=pgd;
  * bf16 autocast (``TRAIN.AMP`` / ``--bf16``) applies to the outer step and to the model forward of
    the inner steps; the attack kernels take bf16 logits natively;
  * data: synthetic (datasets are out of scope).
Optimizer param groups and the warm-up + polynomial LR schedule follow semseg/optimizers.py:13-59 and
semseg/schedulers.py:80-134.  PSPNet (configs/pascalvoc_pspnet.yaml) follows the reference's own recipe instead
(tools/train_rob_seg.py:92-98, 185-204, 338-361): ``PSPNet(50, N_CLS)``, loss = main_loss + 0.4 * aux_loss, SGD over eight
parameter groups (layer0-4, then ppm, cls, aux) and the poly rule set after every step, x10 on the new modules, with no
warm-up (SCHEDULER is ignored).  Its crops satisfy (H - 1) % 8 == 0.  The optional key ``MODEL.CLEAN`` chooses the
backbone's stem: absent or true builds ``PSPNet(50, N_CLS)`` (the deep-base stem, ``clean=True``), false builds
``PSPNet(50, N_CLS, clean=False)``, the torchvision-style stem that takes a pre-trained ImageNet ResNet-50
(configs/pascalvoc_pspnet_pirat.yaml).  The reference decides this from the config's ``ADDENDUM`` instead
(tools/train_rob_seg.py:92-98: clean unless the word "clean" is missing) and would read configs/pascalvoc_pspnet.yaml's
``ADDENDUM: run`` as ``clean=False``; here that file keeps building the deep-base model.
``--native-blocks`` runs the fp32 outer step's ConvNeXt trunk in NHWC on libsea_hip for this run (T3: LayerNorm with
parameter gradients, fused stochastic-depth tail; ``semseg.models.convnext_upernet.TRAIN_NATIVE_BLOCKS``).
``--fused-criterion`` fuses the UperNet branch's final up-sampling into its two cross-entropies for this run (T2u;
``semseg.models.convnext_upernet.TRAIN_FUSED_CRITERION``), and the Segmenter branch's into its one (the model's masks at 1/16
resolution through ``SegMenter.forward(im, lowres=True)``); ``--fused-kernel pow2`` runs them on the single-pass x4 / x16 kernel
(``TRAIN_FUSED_KERNEL``).
On the PSPNet branch ``--native-criterion`` computes the two cross-entropies of the training forward with T2 after the P2
up-samplings, and ``--fused-criterion`` (which wins if both are given) with T2u-ac on the heads' low-resolution logits, for
this run (``semseg.models.pspnet.TRAIN_CRITERION``); ``--fused-kernel`` has no effect there (the single-pass kernel is an
align_corners=False kernel).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist
import yaml
from torch.nn.parallel import DistributedDataParallel as DDP

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from semseg import attacker  # noqa: E402
from semseg.models import convnext_upernet as _convnext  # noqa: E402
from semseg.models import pspnet as _pspnet  # noqa: E402
from semseg.models import PSPNet, UperNetForSemanticSegmentation, create_segmenter  # noqa: E402
from semseg.val import Pgd_Attack, Pgd_Attack_1  # noqa: E402


def psp_clean(model_cfg) -> bool:
    """``MODEL.CLEAN`` of a PSPNet config: absent means true (the deep-base stem); false is the robust 7x7 stem"""
    clean = model_cfg.get("CLEAN", True)
    if not isinstance(clean, bool):
        raise ValueError(f"MODEL.CLEAN must be true or false, got {clean!r}")
    return clean


def group_weight(model):
    """decay / no-decay parameter groups (semseg/optimizers.py:36-59): 1-D params and norms are not decayed."""
    decay, no_decay = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        (no_decay if (p.ndim <= 1 or "norm" in name) else decay).append(p)
    return [dict(params=decay), dict(params=no_decay, weight_decay=0.0)]


def get_optimizer(model, name, lr, weight_decay):
    groups = group_weight(model)
    if name == "AdamW":
        return torch.optim.AdamW(groups, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
    return torch.optim.SGD(groups, lr, momentum=0.9, weight_decay=weight_decay)


def warmup_poly_lambda(power, max_iter, warmup_iter, warmup_ratio, warmup="exp"):
    """LR ratio of WarmupPolyLR (semseg/schedulers.py:80-134)."""
    def ratio(it):
        if it < warmup_iter:
            a = it / warmup_iter
            return warmup_ratio + (1 - warmup_ratio) * a if warmup == "linear" else warmup_ratio ** (1 - a)
        a = (it - warmup_iter) / max(max_iter - warmup_iter, 1)
        return max(1 - a, 0.0) ** power
    return ratio


def psp_param_groups(model, lr):
    """the reference's PSPNet parameter groups (train_rob_seg.py:185-200): layer0 .. layer4, then ppm, cls, aux"""
    mods = [model.layer0, model.layer1, model.layer2, model.layer3, model.layer4, model.ppm, model.cls, model.aux]
    return [dict(params=list(m.parameters()), lr=lr) for m in mods]


PSP_NEW_GROUPS = 5  # groups 5.. (ppm, cls, aux) run at 10x the backbone's rate


def poly_lr(base_lr, it, max_iter, power=0.9):
    """poly_learning_rate of the reference (train_rob_seg.py:38-41)"""
    return base_lr * (1 - float(it) / max_iter) ** power


def set_psp_lr(opt, base_lr, it, max_iter):
    """after step ``it``: every backbone group at poly_lr(it), the new modules at 10x (train_rob_seg.py:356-361)"""
    lr = poly_lr(base_lr, it, max_iter)
    for k, g in enumerate(opt.param_groups):
        g["lr"] = lr if k < PSP_NEW_GROUPS else lr * 10


def build_attack(train_cfg):
    eps = train_cfg["EPS"] / 255.0
    n = int(train_cfg["N_ITERS"])
    if train_cfg["ATTACK"] == "pgd":
        los = train_cfg["LOSS_FN"]
        if los == "pgd":
            atk = Pgd_Attack_1(epsilon=eps, alpha=1e-2, num_iter=n, los="pgd")
        else:
            atk = Pgd_Attack(eps=eps, alpha=1e-2, num_iter=n, los=los)
        return lambda model, img, lbl: atk.adv_attack(model, img, lbl)[0]
    def apgd(model, img, lbl):
        try:
            return attacker.apgd_train(model, img, lbl, norm="Linf", eps=eps, n_iter=n, use_rs=True, loss="ce-avg",
                                       track_loss=None, num_classes=int(train_cfg.get("N_CLS", 21)))[0]  # x_best, as the reference (train_rob_seg.py:336)
        finally:
            # the weights move every outer step: a captured pair is good for this call only, and its activation pool
            # (several GB) must not sit on the model through the training forward / backward
            attacker.release_graph_cache(model)
    return apgd


def build_criterion(cfg, native: bool):
    """--native-criterion: the Segmenter branch's criterion from the config's LOSS.NAME on T2 (csrc/train_loss.hip), with
    the branch's ignore label -1 and no class weights; None without the flag (F.cross_entropy, as before).  The native
    criterion returns its value in fp32 whatever the logits' dtype, as F.cross_entropy does under autocast."""
    if not native:
        return None
    from semseg.losses import get_loss
    return get_loss(cfg.get("LOSS", {}).get("NAME", "CrossEntropy"), -1, None, native=True)


def build_fused_criterion(up_kernel: str = "gather"):
    """--fused-criterion, Segmenter branch: F.cross_entropy(ignore_index=-1) whose ``upsampled`` takes the masks at 1/16
    resolution and interpolates inside its kernels (T2u; ``up_kernel``: semseg.losses)."""
    from semseg.losses import CrossEntropy
    return CrossEntropy(-1, native=True, up_kernel=up_kernel)


def segmenter_loss(ddp, img, lbl, criterion=None, fused=None):
    """The Segmenter branch's outer loss (train_rob_seg.py:346-347).  ``fused`` (build_fused_criterion): the model's
    low-resolution masks go straight into the criterion, no (B, C, H, W) tensor exists; a model that returns None (an input
    that needs padding) takes the unfused line.  ``criterion`` (build_criterion): T2 on the full-resolution logits."""
    if fused is not None:
        low = ddp(img, lowres=True)
        if low is not None:
            return fused.upsampled(low, lbl)
    if criterion is not None:
        return criterion(ddp(img).contiguous(), lbl)
    return torch.nn.functional.cross_entropy(ddp(img), lbl, ignore_index=-1)


def _main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", type=str, default="configs/ade20k_convnext.yaml")
    ap.add_argument("--world_size", type=int, default=None, help="accepted for CLI parity; torchrun's env wins")
    ap.add_argument("--synthetic", type=int, default=64, help="synthetic images per rank")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch_size", type=int, default=None)
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--json", type=str, default=None)
    ap.add_argument("--backend", type=str, default="nccl", help="torch.distributed backend (nccl = RCCL over xGMI)")
    ap.add_argument("--deterministic", action="store_true", help="no MIOpen find-mode benchmarking")
    ap.add_argument("--emulate_ranks", type=int, default=0,
                    help="single process standing in for N data-parallel ranks: every step runs the N ranks' batches "
                         "one after the other from the same weights and averages their gradients (what DDP's "
                         "all-reduce computes); used to check the multi-rank run")
    ap.add_argument("--dump_params", type=str, default=None,
                    help="save a sample of parameter tensors and of their (rank-averaged) gradients of the last step")
    ap.add_argument("--native-criterion", action="store_true",
                    help="Segmenter branch: compute the outer step's criterion with get_loss(cfg LOSS.NAME, -1, None, "
                         "native=True) (T2, csrc/train_loss.hip) instead of F.cross_entropy.  PSPNet branch: the two "
                         "cross-entropies of the model's training forward on T2 (pspnet.TRAIN_CRITERION = native)")
    ap.add_argument("--native-blocks", action="store_true",
                    help="ConvNeXt trunk: train-mode blocks and trainable LayerNorms in NHWC on libsea_hip (T3, fp32; "
                         "csrc/ln_kernels.hip, csrc/block_tail.hip) for this run")
    ap.add_argument("--fused-criterion", action="store_true",
                    help="UperNet and Segmenter branches: the outer step's cross-entropies take the heads' low-resolution "
                         "logits (1/4 and 1/16; Segmenter's masks at 1/16) and interpolate inside the criterion (T2u, "
                         "csrc/train_loss_up.hip) for this run; no full-resolution logits are created.  PSPNet branch: "
                         "the same with align_corners=True on its two x8 heads (pspnet.TRAIN_CRITERION = fused)")
    ap.add_argument("--fused-kernel", choices=("gather", "pow2"), default="gather",
                    help="with --fused-criterion: T2u's kernel.  gather = any ratio, two launches; pow2 = forward and "
                         "gradient in one pass for x4 / x16 (csrc/train_loss_up_pow2.hip)")
    args = ap.parse_args(argv)
    if args.native_blocks:
        _convnext.TRAIN_NATIVE_BLOCKS = True
    if args.fused_criterion:
        _convnext.TRAIN_FUSED_CRITERION = True
        _convnext.TRAIN_FUSED_KERNEL = args.fused_kernel
    if args.fused_criterion or args.native_criterion:      # read by PSPNet's training forward only
        _pspnet.TRAIN_CRITERION = "fused" if args.fused_criterion else "native"
    with open(args.cfg) as f:
        cfg = yaml.load(f, Loader=yaml.SafeLoader)
    train_cfg, model_cfg, data_cfg = cfg["TRAIN"], cfg["MODEL"], cfg["DATASET"]
    C = int(data_cfg["N_CLS"])
    train_cfg["N_CLS"] = C

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(args.backend, rank=rank, world_size=world)
    dev = torch.device("cuda", local % max(torch.cuda.device_count(), 1))
    torch.cuda.set_device(dev)
    torch.backends.cudnn.benchmark = not args.deterministic
    torch.manual_seed(0)

    if model_cfg["NAME"] == "UperNetForSemanticSegmentation":
        model = UperNetForSemanticSegmentation(model_cfg["BACKBONE"], C, None)
    elif model_cfg["NAME"] == "SegMenter":
        from semseg.utils.utils import load_config_segmenter
        mcfg, _ = load_config_segmenter(backbone=model_cfg["BACKBONE"], n_cls=C)
        model = create_segmenter(mcfg, None, model_cfg["BACKBONE"])
    elif model_cfg["NAME"] == "PSPNet":
        model = PSPNet(50, C, clean=psp_clean(model_cfg))
    else:
        raise ValueError(model_cfg["NAME"])
    psp = model_cfg["NAME"] == "PSPNet"
    model = model.to(dev)
    ddp = DDP(model, device_ids=[dev.index]) if world > 1 else model
    core = model  # the attack always runs on the un-wrapped module: no collective inside the inner loop

    virt = max(args.emulate_ranks, 1)  # data-parallel ranks this process stands in for
    bs = args.batch_size or int(train_cfg["BATCH_SIZE"]) // max(world * virt, 1)
    size = int(train_cfg["IMAGE_SIZE"][0])
    # synthetic crops: multiples of 32 keep every feature map integral; PSPNet needs (H - 1) % 8 == 0 instead
    size -= (size - 1) % 8 if psp else size % 32
    n = max(args.synthetic, bs)

    def rank_data(r):
        g = torch.Generator().manual_seed(1234 + r)
        im = torch.rand(n, 3, size, size, generator=g)
        k = -(-size // 32)
        lb = torch.randint(0, C, (n, k, k), generator=g).repeat_interleave(32, 1).repeat_interleave(32, 2)
        return im, lb[:, :size, :size]

    data = [rank_data(rank * virt + v) for v in range(virt)]

    total = args.steps + args.warmup
    base_lr = cfg["OPTIMIZER"]["LR"]
    if psp:
        opt = torch.optim.SGD(psp_param_groups(core, base_lr), base_lr, momentum=0.9,
                              weight_decay=cfg["OPTIMIZER"]["WEIGHT_DECAY"])
        sched = None
    else:
        opt = get_optimizer(ddp, cfg["OPTIMIZER"]["NAME"], base_lr, cfg["OPTIMIZER"]["WEIGHT_DECAY"])
        sched = torch.optim.lr_scheduler.LambdaLR(opt, warmup_poly_lambda(
            cfg["SCHEDULER"]["POWER"], max(total, 2), min(int(cfg["SCHEDULER"]["WARMUP"]), total // 2),
            cfg["SCHEDULER"]["WARMUP_RATIO"]))
    amp = bool(train_cfg["AMP"]) or args.bf16
    attack_fn = build_attack(train_cfg) if train_cfg["ADVERSARIAL"] else None
    criterion = build_criterion(cfg, args.native_criterion)
    if criterion is not None:
        criterion = criterion.to(dev)
    fused = None
    if args.fused_criterion and model_cfg["NAME"] == "SegMenter":
        fused = build_fused_criterion(args.fused_kernel).to(dev)

    def one_step(i):
        idx = [(i * bs + j) % n for j in range(bs)]
        opt.zero_grad(set_to_none=True)
        first = None
        # emulated ranks: every rank starts the step from the same buffers (BatchNorm running statistics feed the
        # eval-mode inner attack), and rank 0's buffers are the ones that survive (DDP broadcasts them)
        buf0 = [b.clone() for b in core.buffers()] if virt > 1 else None
        buf_r0 = None
        for v, (images, labels) in enumerate(data):
            if v > 0:
                if buf_r0 is None:
                    buf_r0 = [b.clone() for b in core.buffers()]
                for b, b0 in zip(core.buffers(), buf0):
                    b.copy_(b0)
            img, lbl = images[idx].to(dev, non_blocking=True), labels[idx].to(dev, non_blocking=True)
            # the random start of the inner attack: one stream per (data-parallel rank, step), whoever runs it
            torch.cuda.manual_seed(1000003 * (rank * virt + v) + i)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                if attack_fn is not None:
                    core.eval()
                    img = attack_fn(core, img, lbl)
                    core.train()
                if psp:
                    main_loss, aux_loss, _ = ddp(img, lbl)
                    loss = main_loss + 0.4 * aux_loss
                elif model_cfg["NAME"] == "UperNetForSemanticSegmentation":
                    loss, _ = ddp(img, lbl)
                else:
                    loss = segmenter_loss(ddp, img, lbl, criterion, fused)
            # DDP all-reduces (averages) the gradient buckets in backward: the step's only collective.  Emulated
            # ranks accumulate loss / virt instead, which is the same average.
            (loss / virt if virt > 1 else loss).backward()
            first = loss.detach() if first is None else first
        if buf_r0 is not None:
            for b, b0 in zip(core.buffers(), buf_r0):
                b.copy_(b0)
        opt.step()
        if psp:
            set_psp_lr(opt, base_lr, i, total)
        else:
            sched.step()
        return first

    for i in range(args.warmup):
        one_step(i)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.warmup, total):
        loss = one_step(i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if rank == 0:
        n_inner = int(train_cfg["N_ITERS"]) if attack_fn is not None else 0
        out = {"model": f"{model_cfg['NAME']}-{model_cfg['BACKBONE']}", "world": world, "batch_per_gpu": bs,
               "image_size": size, "n_cls": C, "bf16": amp, "inner_pgd_steps": n_inner,
               "samples_per_s": world * bs * args.steps / dt,
               "inner_image_iterations_per_s": world * bs * args.steps * n_inner / dt,
               "ms_per_outer_step": dt * 1e3 / args.steps, "last_loss": float(loss)}
        out["native_blocks"] = bool(_convnext.TRAIN_NATIVE_BLOCKS)
        out["fused_criterion"] = bool(_convnext.TRAIN_FUSED_CRITERION)
        out["fused_kernel"] = _convnext.TRAIN_FUSED_KERNEL if _convnext.TRAIN_FUSED_CRITERION else None
        out["psp_criterion"] = _pspnet.TRAIN_CRITERION if psp else None
        print(json.dumps(out))
        if args.json:
            json.dump(out, open(args.json, "w"))
        if args.dump_params:
            named = [(k, p) for k, p in core.named_parameters() if p.grad is not None]
            keep = named[:: max(len(named) // 24, 1)]
            torch.save({"params": {k: p.detach().cpu() for k, p in keep}, "grads": {k: p.grad.detach().cpu() for k, p in keep}},
                       args.dump_params)
    if world > 1:
        dist.destroy_process_group()
    return out if rank == 0 else None


def main(argv=None):
    """`_main` with the process-global switches it sets (MIOpen find mode, ``--native-blocks``, ``--fused-criterion``) restored on exit: a caller
    that runs this in-process (tests do) must not inherit `cudnn.benchmark = True` or the T3 switch.  Returns rank 0's
    result record (the JSON line it prints)."""
    prev, prev_blocks = torch.backends.cudnn.benchmark, _convnext.TRAIN_NATIVE_BLOCKS
    prev_fused, prev_kernel = _convnext.TRAIN_FUSED_CRITERION, _convnext.TRAIN_FUSED_KERNEL
    prev_psp = _pspnet.TRAIN_CRITERION
    try:
        return _main(argv)
    finally:
        torch.backends.cudnn.benchmark = prev
        _convnext.TRAIN_NATIVE_BLOCKS = prev_blocks
        _convnext.TRAIN_FUSED_CRITERION = prev_fused
        _convnext.TRAIN_FUSED_KERNEL = prev_kernel
        _pspnet.TRAIN_CRITERION = prev_psp


if __name__ == "__main__":
    main()
