#!/usr/bin/env python3
"""Golden outputs of the reference's PSPNet-ResNet50 with the robust (``clean=False``) stem (CPU, build container only):

    python devtools/gen_psp_robust_goldens.py

Builds nmndeep/Robust-Segmentation's own ``PSPNet(50, 21, pretrained=False, clean=False)`` (semseg/models/ddcat_psp.py:372-486
with the torchvision-style stem of backbones/resnet_ddcat.py:115-131: the shape that takes a pre-trained ImageNet ResNet-50,
358 state-dict keys) on CPU, loads the seeded weights of devtools/psp_weights.py with ``strict=True``, and writes
tests/golden/g18_psp_robust_<H>x<W>.npz with the fields of g16 (devtools/gen_psp_goldens.py): the input, labels with about
5 % set to -1, the class weights, the eval logits and their argmax, the input gradients of the reference's mask-ce-avg and
mask-ce-bal losses averaged over the pixels of an image and summed over images, the reference's state-dict key list and
the seed.  Only data is written."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("SEA_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path[:0] = [os.path.join(ROOT, "oracle", "shims"), REF, ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SEED = 18
CASES = ((65, 65), (57, 97))


def main():
    os.chdir(REF)
    torch.set_num_threads(4)
    from semseg.attacker import masked_cross_entropy, masked_cross_entropy_balanced
    from semseg.models.ddcat_psp import PSPNet
    from devtools.psp_weights import seeded_state_dict

    net = PSPNet(50, 21, pretrained=False, clean=False)
    sd = net.state_dict()
    net.load_state_dict(seeded_state_dict(sd, SEED), strict=True)
    net.eval()
    for H, W in CASES:
        g = torch.Generator().manual_seed(1800 + H * 7 + W)
        x = torch.rand(1, 3, H, W, generator=g)
        with torch.no_grad():
            logits = net(x)
        pred = logits.argmax(1)
        # labels: the clean prediction with 20 % of the pixels re-drawn and about 5 % ignored
        y = torch.where(torch.rand(pred.shape, generator=g) < 0.2, torch.randint(0, 21, pred.shape, generator=g), pred)
        y[torch.rand(pred.shape, generator=g) < 0.05] = -1
        w = 0.5 + torch.rand(21, generator=g)
        grads = {}
        for name, fn in (("avg", masked_cross_entropy), ("bal", masked_cross_entropy_balanced)):
            xi = x.clone().requires_grad_(True)
            out = net(xi)
            loss = fn(out, y, weights=w)
            loss.view(loss.shape[0], -1).mean(-1).sum().backward()
            grads[name] = xi.grad.detach()
        path = os.path.join(OUT, f"g18_psp_robust_{H}x{W}.npz")
        np.savez_compressed(path, x=x.numpy(), y=y.numpy().astype(np.int16), weights=w.numpy(),
                            logits=logits.numpy(), pred=pred.numpy().astype(np.int16),
                            grad_mask_ce_avg=grads["avg"].numpy(), grad_mask_ce_bal=grads["bal"].numpy(),
                            keys=np.array(list(sd)), seed=np.int64(SEED))
        print(path, os.path.getsize(path), "logit scale", float(logits.abs().max()),
              "grad scale", float(grads["bal"].abs().max()))


if __name__ == "__main__":
    main()
