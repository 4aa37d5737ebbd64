"""PSPNet-ResNet50 on the device: the P1 polyphase split / merge, the dilated convolution built on it, the P2
align_corners=True up-sampling (NCHW logits and the PPM's channels_last up-cat), the P3 residual add + ReLU, the whole
model against the reference's goldens (tests/golden/g16_psp_*.npz, weights from devtools/psp_weights.py), the attack on it
in eager and graph mode, and tools.infer on configs/pascalvoc_pspnet.yaml."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

_CL = torch.channels_last
# Whole-model tolerances, set from the first measurement on MI355X (test_model_matches_the_reference_goldens): max |logit|
# error relative to max |logit| 1.1e-6 / 1.3e-6 on the device against 0.92e-6 / 0.97e-6 for stock PyTorch-ROCm fp32
# (65x65 / 57x97); relative L2 error of the input gradients 1.8e-4 / 0.6e-3 to 2.0e-3 on both paths alike.  The gradient
# error is set by discrete events -- pre-activations within rounding of zero whose ReLU gate flips, max-pool winners --
# not by the arithmetic's precision (the stock path's error is as large), so its bound carries an absolute floor.
ERR_FACTOR = 2.0            # device error <= ERR_FACTOR x the stock error
GRAD_FLOOR = 5e-3           # + this, for the input gradients


def _randn(*shape, seed=0, cl=True):
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()
    return t.contiguous(memory_format=_CL) if cl else t


def _unfold_split(x, d):
    """the torch formulation of P1: pad to a multiple of d, (B,C,Hs,d,Ws,d) -> (B*d*d, C, Hs, Ws), phase py*d + px"""
    B, C, H, W = x.shape
    Hs, Ws = -(-H // d), -(-W // d)
    xp = F.pad(x, (0, Ws * d - W, 0, Hs * d - H))
    return xp.reshape(B, C, Hs, d, Ws, d).permute(0, 3, 5, 1, 2, 4).reshape(B * d * d, C, Hs, Ws)


# ------------------------------------------------------------------------------------------------------------ P1
@pytest.mark.parametrize("B,C,H,W,d", [(2, 256, 60, 60, 2), (2, 512, 60, 60, 4), (2, 64, 9, 9, 4), (3, 12, 7, 11, 3)])
def test_polyphase_split_merge(B, C, H, W, d):
    from semseg import _native as N
    x = _randn(B, C, H, W, seed=B + C + d)
    s = N.polyphase_split(x, d)
    assert s.shape == (B * d * d, C, -(-H // d), -(-W // d)) and N.cl_pixel_stride(s) == C
    assert torch.equal(s, _unfold_split(x, d))
    assert torch.equal(N.polyphase_merge(s, (H, W), d), x)                 # identity, ragged tails included
    # adjoint pair: <S x, y> == <x, M y>
    y = _randn(*s.shape, seed=7)
    lhs = (s.double() * y.double()).sum().item()
    rhs = (x.double() * N.polyphase_merge(y, (H, W), d).double()).sum().item()
    assert abs(lhs - rhs) <= 1e-9 * max(1.0, abs(lhs))
    # phase (0, 0) alone = x[::d, ::d]; its adjoint scatters back onto that grid
    s0 = N.polyphase_split(x, d, first_only=True)
    assert torch.equal(s0, x[:, :, ::d, ::d])
    m0 = N.polyphase_merge(s0, (H, W), d, first_only=True)
    want = torch.zeros_like(x)
    want[:, :, ::d, ::d] = x[:, :, ::d, ::d]
    assert torch.equal(m0, want)


@pytest.mark.parametrize("B,C,H,W,d", [(2, 256, 60, 60, 2), (2, 512, 60, 60, 4)])
def test_dilated_conv_matches_fp64(B, C, H, W, d):
    from semseg.models.pspnet import dilated_conv3x3
    x = _randn(B, C, H, W, seed=d)
    w = (torch.randn(C, C, 3, 3, generator=torch.Generator().manual_seed(9 + d)) * (2.0 / (9 * C)) ** 0.5).cuda()
    g = _randn(B, C, H, W, seed=20 + d)
    xi = x.clone().requires_grad_(True)
    y = dilated_conv3x3(xi, w, d, {})
    (gx,) = torch.autograd.grad(y, [xi], g)
    xd = x.cpu().double().requires_grad_(True)
    yd = F.conv2d(xd, w.cpu().double(), padding=d, dilation=d)
    (gxd,) = torch.autograd.grad(yd, [xd], g.cpu().double())
    ef = (y.cpu().double() - yd.detach()).abs().max().item() / yd.abs().max().item()
    eb = (gx.cpu().double() - gxd).abs().max().item() / gxd.abs().max().item()
    print(f"dilated d={d} C={C}: forward {ef:.2e}, input gradient {eb:.2e}")
    assert ef <= 3e-4 and eb <= 3e-4


# ------------------------------------------------------------------------------------------------------------ P2
def test_upsample_x8_is_bitwise_interpolate_and_its_gradient_is_deterministic():
    from semseg import _native as N
    x = _randn(2, 21, 60, 60, seed=3, cl=False) * 4
    ref = F.interpolate(x, size=(473, 473), mode="bilinear", align_corners=True)
    assert torch.equal(N.upsample_ac(x, (473, 473)), ref)
    g = _randn(2, 21, 473, 473, seed=4, cl=False)
    xi = x.clone().requires_grad_(True)
    (want,) = torch.autograd.grad(F.interpolate(xi, size=(473, 473), mode="bilinear", align_corners=True), [xi], g)
    got = N.upsample_ac_backward(g, (60, 60))
    assert (got - want).abs().max().item() <= 1e-6 * want.abs().max().item()
    assert torch.equal(got, N.upsample_ac_backward(g, (60, 60)))


@pytest.mark.parametrize("s", [1, 2, 3, 6])
def test_ppm_upcat_matches_interpolate(s):
    from semseg import _native as N
    t = _randn(2, 512, s, s, seed=s)
    buf = torch.empty(2, 2048 + 512, 60, 60, device="cuda", memory_format=_CL).zero_()
    N.upsample_ac_cl(t, (60, 60), out=buf[:, 2048:])
    ref = F.interpolate(t.contiguous(), size=(60, 60), mode="bilinear", align_corners=True)
    assert (buf[:, 2048:] - ref).abs().max().item() <= 1e-6 * max(1.0, ref.abs().max().item())
    assert not buf[:, :2048].any()                                       # nothing written outside the slice
    gbuf = _randn(2, 2048 + 512, 60, 60, seed=10 + s)
    ti = t.clone().requires_grad_(True)
    (want,) = torch.autograd.grad(F.interpolate(ti, size=(60, 60), mode="bilinear", align_corners=True), [ti],
                                  gbuf[:, 2048:])
    got = N.upsample_ac_cl_backward(gbuf[:, 2048:], (s, s))
    # each input pixel sums up to 3600 / s^2 outputs: both sums are compared with float64, autograd's (atomics) included
    td = t.cpu().double().requires_grad_(True)
    (exact,) = torch.autograd.grad(F.interpolate(td, size=(60, 60), mode="bilinear", align_corners=True), [td],
                                   gbuf[:, 2048:].cpu().double())
    err = (got.cpu().double() - exact).abs().max().item()
    err_autograd = (want.cpu().double() - exact).abs().max().item()
    assert err <= max(2 * err_autograd, 1e-6 * exact.abs().max().item()), (err, err_autograd)
    assert torch.equal(got, N.upsample_ac_cl_backward(gbuf[:, 2048:], (s, s)))


# ------------------------------------------------------------------------------------------------------------ P3
def test_add_relu():
    from semseg import _native as N
    a, r, g = _randn(2, 256, 15, 15, seed=1), _randn(2, 256, 15, 15, seed=2), _randn(2, 256, 15, 15, seed=3)
    y = N.add_relu(a, r)
    assert torch.equal(y, torch.relu(a + r)) and y.is_contiguous(memory_format=_CL)
    assert torch.equal(N.add_relu_backward(g, y), torch.where(y > 0, g, torch.zeros_like(g)))


# ------------------------------------------------------------------------------------------------------------ model
def _golden(tag):
    return {k: torch.from_numpy(v) if v.dtype != object and v.dtype.kind in "fiu" else v
            for k, v in np.load(os.path.join(GOLDEN, f"g16_psp_{tag}.npz")).items()}


def _model(seed):
    from devtools.psp_weights import seeded_state_dict
    from semseg.models import PSPNet
    m = PSPNet(50, 21)
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
        from semseg.models import pspnet
        self.old, pspnet.USE_NATIVE = pspnet.USE_NATIVE, self.on

    def __exit__(self, *exc):
        from semseg.models import pspnet
        pspnet.USE_NATIVE = self.old


@pytest.mark.parametrize("tag", ["65x65", "57x97"])
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
    model = _model(16)
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
    assert (losses[True] - losses[False]).abs().max().item() <= 1e-3 * losses[False].abs().max().item() + 1e-6


def _cfg(tmp_path):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "pascalvoc_pspnet.yaml")))
    cfg["SAVE_DIR"] = str(tmp_path) + "/"
    p = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(p, "w"))
    return p


def test_infer_runs_pspnet_and_evalsea_reads_its_files(tmp_path):
    import random
    from tools import infer
    from tools.worse_only import evalSEA
    s = infer.main(["--cfg", _cfg(tmp_path), "--synthetic", "4", "--n_iter", "6", "--batch_size", "2", "--cleanup", "1"])
    assert s["model"] == "PSPNet_RN50" and s["n_images"] == 4
    g = torch.Generator().manual_seed(3)
    images = torch.rand(3, 3, 473, 473, generator=g)
    labels = torch.randint(0, 21, (3, 473, 473), generator=g)
    labels[torch.rand(3, 473, 473, generator=g) < 0.05] = -1
    data = str(tmp_path / "data.pt")
    torch.save({"images": images, "labels": labels}, data)
    s = infer.main(["--cfg", _cfg(tmp_path), "--eps", "8", "--n_iter", "6", "--data", data, "--random_init",
                    "--batch_size", "2", "--cleanup", "0", "--save_argmax"])
    name = "PSPNet_RN50"
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
