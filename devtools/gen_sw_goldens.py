#!/usr/bin/env python3
"""Golden sliding-window evaluations from the reference (CPU, build container only):

    python devtools/gen_sw_goldens.py

Loads nmndeep/Robust-Segmentation's own ``semseg/utils/segmenter_eval.py`` by path (it imports only torch) and calls its
``resize``, ``sliding_window`` and ``merge_windows`` on the tiny seeded models of oracle/tiny_models.py, one image at a
time as the reference does, and writes tests/golden/g16_sw_*.npz: the input, the labels, the anchors, the stacked window
logits (image-major), ``logit / count`` before the resize (recorded from the reference's own call of ``F.interpolate``
inside ``merge_windows``), the returned probabilities, the confusion matrix of their argmax, and the number of pixels
whose top-2 probabilities differ by less than 1e-5.  For a flip case the mirrored pass is what is recorded and the
confusion matrix is that of plain + mirrored, the sum ``evaluate_sliding`` forms.  Only data is written."""
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("SEA_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path[:0] = [ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
WS = 32
# (net, C, H, W, stride, flip); the label size is the input size
CASES = (("conv", 21, 32, 32, 32, 0), ("pw", 21, 32, 45, 32, 0), ("conv", 5, 48, 61, 16, 0), ("conv", 5, 48, 61, 16, 1),
         ("pw", 5, 50, 70, 24, 0), ("conv", 5, 20, 29, 32, 0), ("conv", 5, 20, 29, 32, 1), ("pw", 21, 20, 29, 32, 0))
TIE = 1e-5


def tie_cap(n_valid):
    return max(4, n_valid // 200)


class _RecordingF:
    """stands in for ``torch.nn.functional`` inside the reference module: keeps the tensor handed to ``interpolate``"""

    def __init__(self, real):
        self._real, self.seen = real, []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def interpolate(self, x, *a, **k):
        self.seen.append(x.detach().clone())
        return self._real.interpolate(x, *a, **k)


def main():
    torch.set_num_threads(2)
    spec = importlib.util.spec_from_file_location("ref_segmenter_eval", os.path.join(REF, "semseg", "utils", "segmenter_eval.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    from oracle.tiny_models import PointwiseNet, TinyConvNet, make_labels

    real_F = R.F
    for netname, C, H, W, stride, flip in CASES:
        net = (TinyConvNet if netname == "conv" else PointwiseNet)(C, seed=C + 5)
        g = torch.Generator().manual_seed(1600 + C + H + W)
        x = torch.rand(2, 3, H, W, generator=g)
        y = make_labels(net, x, ignore_frac=0.05, flip_frac=0.1, seed=C + H)

        def one_pass(im, mirrored):
            """the reference's protocol for ONE image: resize, (mirror), windows, model per window, merge"""
            R.F = real_F
            im = R.resize(im, WS)
            if mirrored:
                im = im.flip(3)
            windows = R.sliding_window(im, bool(mirrored), WS, stride)
            crops = torch.stack(windows.pop("crop"))[:, 0]
            with torch.no_grad():
                windows["seg_maps"] = net(crops)
            rec = _RecordingF(real_F)
            R.F = rec
            probs = R.merge_windows(windows, WS, (H, W))
            R.F = real_F
            assert len(rec.seen) == 1
            return windows, rec.seen[0][0], probs

        seg, avg, probs, plain = [], [], [], []
        for i in range(2):
            windows, a, p = one_pass(x[i:i + 1], flip)
            seg.append(windows["seg_maps"])
            avg.append(a)
            probs.append(p)
            plain.append(one_pass(x[i:i + 1], 0)[2] if flip else p)
        probs, plain = torch.stack(probs), torch.stack(plain)
        score = probs + plain if flip else probs
        anchors = np.asarray(windows["anchors"], np.int64)
        valid = y != -1
        top2 = score.topk(2, dim=1).values
        n_ties = int((((top2[:, 0] - top2[:, 1]) < TIE) & valid).sum())
        assert n_ties <= tie_cap(int(valid.sum())), (netname, C, H, W, n_ties)
        pred = score.argmax(1)
        hist = torch.bincount(y[valid] * C + pred[valid], minlength=C * C).view(C, C)
        name = f"g16_sw_{netname}_C{C}_{H}x{W}_s{stride}_flip{flip}"
        np.savez_compressed(os.path.join(OUT, name + ".npz"), x=x.numpy(), y=y.numpy(), window_size=np.int64(WS),
                            window_stride=np.int64(stride), flip=np.int64(flip), n_classes=np.int64(C),
                            ignore_label=np.int64(-1), seed=np.int64(C + 5), net=np.asarray(netname),
                            shape=np.asarray(windows["shape"], np.int64), anchors=anchors,
                            h_anchors=np.unique(anchors[:, 0]), w_anchors=np.unique(anchors[:, 1]),
                            seg_maps=torch.cat(seg).numpy(), logit_avg=torch.stack(avg).numpy(), probs=probs.numpy(),
                            hist=hist.numpy(), near_ties=np.int64(n_ties),
                            **({"score": score.numpy()} if flip else {}))       # flip 0: the score is `probs`
        print("wrote", name, "| merged", tuple(windows["shape"]), "| windows", len(anchors), "| near ties", n_ties)


if __name__ == "__main__":
    main()
