#!/usr/bin/env python3
"""Golden DeepLabV3-ResNet50 outputs from the reference (CPU, build container only):

    python devtools/gen_deeplab_goldens.py

Builds nmndeep/Robust-Segmentation's own ``DeepLabV3(50, classes=21, pretrained=False)`` (semseg/models/ddcat_psp.py:84-189)
on CPU, loads the seeded weights of devtools/psp_weights.py with ``strict=True``, and writes
tests/golden/g19_deeplab_<H>x<W>.npz with the fields of devtools/gen_psp_goldens.py: the input, labels with about 5 % set
to -1, the class weights, the eval logits and their argmax, the input gradients of the reference's mask-ce-avg and
mask-ce-bal losses (semseg/attacker.py:143-174) averaged over the pixels of an image and summed over images, and the
reference's state-dict key list.  Only data is written; devtools/deeplab_goldens.py holds the file layout (no file
above 1 MiB: the 153 x 153 logits go into sibling files).
  65 x 65   (9 x 9 features): rate 6 is ragged, rates 12 and 18 keep only the centre tap;
  57 x 97   (8 x 13): non-square;
  153 x 153 (20 x 20): the smallest map on which rate 18 has off-centre taps."""
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
SEED = 19
CASES = ((65, 65), (57, 97), (153, 153))


def main():
    os.chdir(REF)
    torch.set_num_threads(4)
    from semseg.attacker import masked_cross_entropy, masked_cross_entropy_balanced
    from semseg.models.ddcat_psp import DeepLabV3
    from devtools import deeplab_goldens as layout
    from devtools.psp_weights import seeded_state_dict

    net = DeepLabV3(50, classes=21, pretrained=False)
    sd = net.state_dict()
    net.load_state_dict(seeded_state_dict(sd, SEED), strict=True)
    net.eval()
    for H, W in CASES:
        g = torch.Generator().manual_seed(1900 + H * 7 + W)
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
        files = layout.save(OUT, H, W, dict(x=x.numpy(), y=y.numpy().astype(np.int16), weights=w.numpy(),
                                            logits=logits.numpy(), pred=pred.numpy().astype(np.int16),
                                            grad_mask_ce_avg=grads["avg"].numpy(), grad_mask_ce_bal=grads["bal"].numpy(),
                                            keys=np.array(list(sd)), seed=np.int64(SEED)))
        print([(os.path.basename(f), os.path.getsize(f)) for f in files], "logit scale", float(logits.abs().max()),
              "grad scale", float(grads["bal"].abs().max()))


if __name__ == "__main__":
    main()
