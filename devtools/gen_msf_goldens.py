#!/usr/bin/env python3
"""Golden multi-scale + flip evaluations from the reference (CPU, build container only):

    python devtools/gen_msf_goldens.py

Runs nmndeep/Robust-Segmentation's own ``semseg.val.evaluate_msf`` (semseg/val.py:330-372) on the tiny seeded models of
oracle/tiny_models.py and writes tests/golden/g15_msf_*.npz: inputs, labels, the ``scaled_logits`` each batch hands to
``Metrics.update`` and the final confusion matrix.  A ``Metrics`` subclass patched into the reference's ``val`` namespace
records both.  The reference then calls ``metrics.compute_pixel_acc()`` expecting two values where its own Metrics returns
three (semseg/metrics.py:49-60) and raises ValueError after all the work is done: that error is caught here and recorded.
Only data is written."""
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
SCALES = (0.5, 0.75, 1.0, 1.25, 1.75)
CASES = (("conv", 5, 45, 61), ("conv", 21, 32, 32), ("pw", 5, 32, 32), ("pw", 21, 29, 37))


class _DS:
    def __init__(self, n_classes, ignore_label):
        self.n_classes, self.ignore_label = n_classes, ignore_label


class _Loader(list):
    dataset = None


def main():
    os.chdir(REF)
    torch.set_num_threads(2)
    import semseg.val as V
    from oracle.tiny_models import PointwiseNet, TinyConvNet, make_labels

    rec = {}

    class RecMetrics(V.Metrics):
        def update(self, pred, target):
            rec.setdefault("scaled", []).append(pred.detach().clone())
            super().update(pred, target)
            rec["hist"] = self.hist.clone()

    V.Metrics = RecMetrics
    V.tqdm = lambda it, *a, **k: it
    for netname, C, H, W in CASES:
        Net = TinyConvNet if netname == "conv" else PointwiseNet
        net = Net(C, seed=C + 3)
        g = torch.Generator().manual_seed(1500 + C + H)
        xs = [torch.rand(2, 3, H, W, generator=g) for _ in range(2)]
        ys = [make_labels(net, x, ignore_frac=0.05, flip_frac=0.1, seed=C + i) for i, x in enumerate(xs)]
        for flip in (False, True):
            rec.clear()
            loader = _Loader(zip(xs, ys))
            loader.dataset = _DS(C, -1)
            err = ""
            try:
                V.evaluate_msf(net, loader, "cpu", SCALES, flip)
            except ValueError as e:       # compute_pixel_acc returns three values (reference defect)
                err = str(e)
            name = f"g15_msf_{netname}_C{C}_{H}x{W}_flip{int(flip)}"
            np.savez_compressed(os.path.join(OUT, name + ".npz"), x=torch.stack(xs).numpy(), y=torch.stack(ys).numpy(),
                                scales=np.asarray(SCALES, np.float64), flip=np.int64(flip), n_classes=np.int64(C),
                                ignore_label=np.int64(-1), seed=np.int64(C + 3), net=np.asarray(netname),
                                scaled_logits=torch.stack(rec["scaled"]).numpy(), hist=rec["hist"].numpy(),
                                ref_error=np.asarray(err))
            print("wrote", name, "|", err)


if __name__ == "__main__":
    main()
