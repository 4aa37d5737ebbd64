"""DeepLabV3-ResNet50 on the device: the whole model against the reference's goldens (tests/golden/g19_deeplab_*.npz,
weights from devtools/psp_weights.py), the attack on it in eager and graph mode, and tools.infer on
configs/pascalvoc_deeplabv3.yaml.  (P5 itself and the ASPP module alone: tests/test_aspp_taps_gpu.py.)"""
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

# Whole-model tolerances: PSPNet's constants (tests/test_psp_gpu.py): the same backbone and the same discrete events
# (pre-activations within rounding of zero whose ReLU gate flips, max-pool winners), which set the gradient error on the
# stock path as on the device path.  Measured on MI355X (test_model_matches_the_reference_goldens), device / stock:
#   65x65    max |logit| error / max |logit| 1.01e-6 / 0.91e-6; relative L2 error of the input gradients 2.1e-6 / 0.9e-6
#   57x97    logits 1.29e-6 / 0.95e-6; gradients 1.9e-4 / 1.0e-6 (one discrete event on the device path, none on stock)
#   153x153  logits 1.09e-6 / 0.98e-6; gradients 1.74e-3 / 1.73e-3 (avg), 1.74e-3 / 1.63e-3 (bal)
# argmax agreement outside near-ties 1.0 everywhere; step-0 mask-ce-bal loss at 2 x 3 x 129 x 129: 1.2888128e-2 / 1.2888141e-2.
ERR_FACTOR = 2.0            # device error <= ERR_FACTOR x the stock error
GRAD_FLOOR = 5e-3           # + this, for the input gradients


def _golden(tag):
    from devtools import deeplab_goldens
    H, W = (int(v) for v in tag.split("x"))
    return {k: torch.from_numpy(v) if v.dtype != object and v.dtype.kind in "fiu" else v
            for k, v in deeplab_goldens.load(GOLDEN, H, W).items()}


def _model(seed):
    from devtools.psp_weights import seeded_state_dict
    from semseg.models import DeepLabV3
    m = DeepLabV3(50, classes=21)
    m.load_state_dict(seeded_state_dict(m.state_dict(), seed), strict=True)
    m = m.eval().cuda()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def _img_losses(out, y, w, balanced, pred=None):
    """mask-ce-avg / mask-ce-bal of the reference (attacker.py:143-174), averaged per image.  ``pred``: the prediction that
    decides the mask (default: the argmax of ``out``, as the reference)"""
    mask = (((out.max(1)[1] if pred is None else pred) == y) & (y != -1)).float()
    loss = F.cross_entropy(out, y, reduction="none", ignore_index=-1, weight=w if balanced else None) * mask
    return loss.view(out.shape[0], -1).mean(-1)


class _native:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from semseg.models import deeplabv3
        self.old, deeplabv3.USE_NATIVE = deeplabv3.USE_NATIVE, self.on

    def __exit__(self, *exc):
        from semseg.models import deeplabv3
        deeplabv3.USE_NATIVE = self.old


@pytest.mark.parametrize("tag", ["65x65", "57x97", "153x153"])
def test_model_matches_the_reference_goldens(tag):
    g = _golden(tag)
    model = _model(int(g["seed"]))
    x, y, w = g["x"].cuda(), g["y"].long().cuda(), g["weights"].cuda()
    ref = g["logits"].double()
    scale = ref.abs().max().item()
    pred_ref = g["pred"].long().cuda()
    res = {}
    for on in (True, False):
        with _native(on):
            with torch.no_grad():
                out = model(x)
            errs = {"logits": (out.cpu().double() - ref).abs().max().item() / scale}
            top2 = ref.topk(2, 1).values
            clear = (top2[:, 0] - top2[:, 1]) > 1e-4 * scale                  # outside near-ties
            errs["argmax"] = (out.argmax(1).cpu() == g["pred"].long())[clear].float().mean().item()
            for name, bal in (("avg", False), ("bal", True)):
                xi = x.clone().requires_grad_(True)
                # the mask from the reference's own prediction (= what its gradient used): a near-tie pixel whose
                # argmax flips would otherwise swap a whole pixel's loss in or out of the sum
                (gx,) = torch.autograd.grad(_img_losses(model(xi), y, w, bal, pred_ref).sum(), [xi])
                gr = g[f"grad_mask_ce_{name}"].double()
                errs[name] = ((gx.cpu().double() - gr).norm() / gr.norm()).item()
            res["device" if on else "stock"] = errs
    print(tag, res)
    dev, stock = res["device"], res["stock"]
    assert dev["argmax"] >= 0.999 and stock["argmax"] >= 0.999
    assert dev["logits"] <= ERR_FACTOR * stock["logits"]
    for name in ("avg", "bal"):
        assert dev[name] <= ERR_FACTOR * stock[name] + GRAD_FLOOR


def test_device_path_runs_p5(monkeypatch):
    """the device forward and backward of the whole model go through P5 (no quiet fall-back to the library convolutions)"""
    from semseg import _native as N
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = N.aspp_tap_sum, N.aspp_tap_sum_backward
    monkeypatch.setattr(N, "aspp_tap_sum", lambda *a, **k: (calls.__setitem__("fwd", calls["fwd"] + 1), fwd(*a, **k))[1])
    monkeypatch.setattr(N, "aspp_tap_sum_backward",
                        lambda *a, **k: (calls.__setitem__("bwd", calls["bwd"] + 1), bwd(*a, **k))[1])
    model = _model(19)
    xi = torch.rand(1, 3, 65, 65, generator=torch.Generator().manual_seed(2)).cuda().requires_grad_(True)
    out = model(xi)
    assert out.shape == (1, 21, 65, 65) and calls == {"fwd": 1, "bwd": 0}
    (gx,) = torch.autograd.grad(out.square().sum(), [xi])
    assert calls == {"fwd": 1, "bwd": 1} and torch.isfinite(gx).all() and gx.abs().max().item() > 0


def test_apgd_graph_equals_eager_and_matches_stock():
    # the library convolutions (stem conv1, layer2's strided 3x3) in immediate mode: a fixed solver per shape, whose backward
    # is bitwise repeatable (find mode times the solvers and may keep one that accumulates with atomics; bench.py does the same)
    old_mode = (torch.backends.cudnn.benchmark, torch.backends.miopen.immediate)
    torch.backends.cudnn.benchmark, torch.backends.miopen.immediate = False, True
    try:
        _apgd_checks()
    finally:
        torch.backends.cudnn.benchmark, torch.backends.miopen.immediate = old_mode


def _apgd_checks():
    from semseg import attacker as A
    from semseg.utils.utils import VOC_WTS
    model = _model(19)
    x = torch.rand(2, 3, 129, 129, generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        y = model(x).max(1)[1]
    y[:, :3] = -1
    w = torch.tensor(VOC_WTS).cuda()
    eps = 8.0 / 255
    outs = []
    for graph in (False, True):
        old, A.USE_HIP_GRAPH = A.USE_HIP_GRAPH, graph
        try:
            A.release_graph_cache(model)
            outs.append(A.apgd_train(model, x, y, "Linf", eps, n_iter=12, loss="mask-ce-bal", early_stop=True,
                                     track_loss="ce-avg", num_classes=21, weights=w, return_pred=True))
        finally:
            A.USE_HIP_GRAPH = old
            A.release_graph_cache(model)
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    xba = outs[0][3]
    assert (xba - x).abs().max().item() <= eps + 1e-6 and xba.min().item() >= 0.0 and xba.max().item() <= 1.0
    # step 0: the loss at the clean input, device path against stock PyTorch-ROCm
    losses = {}
    for on in (True, False):
        with _native(on), torch.no_grad():
            losses[on] = _img_losses(model(x), y, w, True)
    print("step-0 losses", losses[True].tolist(), losses[False].tolist())
    assert (losses[True] - losses[False]).abs().max().item() <= 1e-3 * losses[False].abs().max().item() + 1e-6


def _cfg(tmp_path):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "pascalvoc_deeplabv3.yaml")))
    cfg["SAVE_DIR"] = str(tmp_path) + "/"
    p = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(p, "w"))
    return p


def test_infer_runs_deeplabv3_and_evalsea_reads_its_files(tmp_path):
    import random
    from tools import infer
    from tools.worse_only import evalSEA
    s = infer.main(["--cfg", _cfg(tmp_path), "--synthetic", "4", "--n_iter", "6", "--batch_size", "2", "--cleanup", "1"])
    assert s["model"] == "DeepLabV3_RN50" and s["n_images"] == 4
    g = torch.Generator().manual_seed(3)
    images = torch.rand(3, 3, 473, 473, generator=g)
    labels = torch.randint(0, 21, (3, 473, 473), generator=g)
    labels[torch.rand(3, 473, 473, generator=g) < 0.05] = -1
    data = str(tmp_path / "data.pt")
    torch.save({"images": images, "labels": labels}, data)
    s = infer.main(["--cfg", _cfg(tmp_path), "--eps", "8", "--n_iter", "6", "--data", data, "--random_init",
                    "--batch_size", "2", "--cleanup", "0", "--save_argmax"])
    name = "DeepLabV3_RN50"
    for loss in infer.LOSSES:
        lg = torch.load(os.path.join(str(tmp_path), "argmax-logs", f"{name}_{loss}_8.0.pt"))
        assert lg.shape == (3, 473, 473) and lg.dtype == torch.int64
    sd = {"seed": 225, "worst_Acc": 0, "worst_Acc_indiv": 0, "final_miou": 0, "loss-wise_miou": []}
    ev = evalSEA(labels, [], 8.0, 21, "SEA_" + name, str(tmp_path), sd, name)
    ev.worse_case_eval(bs=2, n_batches=-1)
    random.seed(225)
    ev.worst_case_miou()
    assert ev.saveDict["worst_Acc"] == pytest.approx(s["worst_Acc"], rel=1e-6)
    assert ev.saveDict["final_miou"] == s["final_miou"]
