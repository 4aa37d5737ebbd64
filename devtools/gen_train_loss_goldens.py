#!/usr/bin/env python3
"""Golden values of the reference's training criteria (CPU, build container only):

    python devtools/gen_train_loss_goldens.py

Imports nmndeep/Robust-Segmentation's own ``semseg.losses`` (CrossEntropy, OhemCrossEntropy: semseg/losses.py:6-63)
through the shims of oracle/shims and writes tests/golden/g17_train_loss_<name>.npz: logits ``randn(2, C, 24, 20) * 3``
with ``z_y += 6`` on about 70 % of the pixels, labels with about 5 % ``ignore_label`` (255 in one set, -1 in the other),
with and without class weights, one prediction and a 2-tuple (the C = 151 2-tuples alone are 12 x 10 pixels instead of
24 x 20, which keeps every file under the committed-file limit); the scalar loss and d loss / d preds of the reference.  The logits are rounded
to bf16-representable values and stored as their upper 16 bits (``pred<k>_bf16bits``: float32 = bits << 16).
OhemCrossEntropy in three regimes: threshold mode (n_hard >= n_min), top-k mode (confident logits: few losses exceed
-log 0.7 = 0.3567) and every label ignored (NaN).  Only arrays are written."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("SEA_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path[:0] = [os.path.join(ROOT, "oracle", "shims"), REF]

import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
B = 2
REGIME = {"threshold": 0, "topk": 1, "all_ignored": 2}


def make_inputs(C, ignore, seed, n_preds, confident=False, all_ignored=False):
    H, W = (12, 10) if (C == 151 and n_preds == 2) else (24, 20)
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, C, (B, H, W), generator=g)
    preds = []
    for _ in range(n_preds):
        z = torch.randn(B, C, H, W, generator=g) * 3
        big = 12.0 + 2.5 * float(np.log(C))  # above log sum exp of the other classes: few losses reach -log 0.7
        boost = (torch.rand(B, H, W, generator=g) < (0.995 if confident else 0.7)).float() * (big if confident else 6.0)
        z.scatter_add_(1, y[:, None], boost[:, None])
        preds.append(z.bfloat16().float())  # bf16-exact values: stored as 16-bit patterns, and the bf16 test's input
    y = y.clone()
    y[torch.rand(B, H, W, generator=g) < 0.05] = ignore
    if all_ignored:
        y[:] = ignore
    w = 0.5 + torch.rand(C, generator=g)
    return preds, y, w


def run(mod, preds, y):
    leaves = [p.clone().requires_grad_(True) for p in preds]
    loss = mod(tuple(leaves) if len(leaves) > 1 else leaves[0], y)
    loss.backward()
    return loss.detach(), [p.grad.detach() for p in leaves]


def main():
    torch.set_num_threads(4)
    from semseg import losses as R
    assert os.path.realpath(R.__file__).startswith(os.path.realpath(REF)), R.__file__
    # (C, ignore, weighted, n_preds, kind, regime, confident, all_ignored); the seed of a case is 1700 + its position.  The
    # C = 151 cases added later (2-tuples, and the other two label / weight combinations) are numbered after the rest so
    # that no earlier fixture changes.
    first, later = [], []
    for C in (5, 21, 151):
        for ignore in (255, -1):
            for weighted in (False, True):
                for n_preds in (1, 2):
                    cases = [("ce", "threshold", False, False)]
                    cases += [("ohem", "threshold", False, False), ("ohem", "topk", True, False)]
                    if not weighted and n_preds == 1:
                        cases += [("ohem", "all_ignored", False, True), ("ce", "all_ignored", False, True)]
                    dst = later if C == 151 and (n_preds == 2 or (ignore == 255) == weighted) else first
                    dst += [(C, ignore, weighted, n_preds) + c for c in cases]
    n = 0
    for C, ignore, weighted, n_preds, kind, regime, confident, all_ign in first + later:
        seed = 1700 + n
        preds, y, w = make_inputs(C, ignore, seed, n_preds, confident, all_ign)
        wt = w if weighted else None
        mod = (R.CrossEntropy if kind == "ce" else R.OhemCrossEntropy)(ignore, wt)
        loss, grads = run(mod, preds, y)
        aux = list(mod.aux_weights)[:n_preds]
        n_sel, n_min = [], []
        if kind == "ohem":
            for p in preds:   # the regime the reference takes, and the gap at the cut in top-k mode
                px = torch.nn.functional.cross_entropy(p, y, weight=wt, ignore_index=ignore,
                                                       reduction="none").view(-1)
                nm = int((y != ignore).sum()) // 16
                nh = int((px > mod.thresh).sum())
                took = "all_ignored" if all_ign else ("topk" if nh < nm else "threshold")
                assert took == regime, (kind, C, ignore, weighted, n_preds, regime, took, nh, nm)
                if took == "topk":
                    top = px.topk(nm + 1).values
                    assert top[nm - 1] > top[nm], "tie at the cut: the gradient would be ambiguous"
                n_sel.append(nm if took == "topk" else nh)
                n_min.append(nm)
        if all_ign:
            assert torch.isnan(loss), loss
        else:
            assert torch.isfinite(loss), loss
        name = (f"g17_train_loss_{kind}_C{C}_ign{'m1' if ignore < 0 else ignore}_"
                f"{'w' if weighted else 'u'}_p{n_preds}_{regime}")
        path = os.path.join(OUT, name + ".npz")
        arrays = dict(labels=y.numpy().astype(np.int16), ignore_label=np.int64(ignore),
                      weights=(wt.numpy() if weighted else np.zeros(0, np.float32)),
                      aux_weights=np.asarray(aux, np.float64), ohem=np.int64(kind == "ohem"),
                      regime=np.int64(REGIME[regime]), n_sel=np.asarray(n_sel, np.int64),
                      n_min=np.asarray(n_min, np.int64), loss=loss.numpy(), seed=np.int64(seed))
        for k, (p, gr) in enumerate(zip(preds, grads)):
            bits = (p.numpy().view(np.uint32) >> 16).astype(np.uint16)
            assert np.array_equal((bits.astype(np.uint32) << 16).view(np.float32), p.numpy())
            arrays[f"pred{k}_bf16bits"] = bits
            arrays[f"grad{k}"] = gr.numpy()
        np.savez_compressed(path, **arrays)
        print(f"{name}: regime {regime} loss {float(loss):.6f} n_sel {n_sel} n_min {n_min} "
              f"grad zero-or-nan {[bool(((g == 0) | g.isnan()).all()) for g in grads]} "
              f"grad nan {[bool(g.isnan().any()) for g in grads]} {os.path.getsize(path)} B")
        n += 1
    print(n, "fixtures")


if __name__ == "__main__":
    main()
