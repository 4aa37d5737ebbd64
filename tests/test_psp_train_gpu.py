"""PIR-AT training of PSPNet-ResNet50 on the device: the T1 train-mode BatchNorm kernels against F.batch_norm, the dilated
train convolution (P1 split -> dense 3x3 -> P1 merge) against F.conv2d, the whole training forward / backward against the
stock model, an eval attack forward after training steps (no stale folded BatchNorm), and tools.train_rob_seg on
configs/pascalvoc_pspnet.yaml."""
import json
import math
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
import yaml

from conftest import PKG

pytestmark = pytest.mark.gpu

_CL = torch.channels_last


def _randn(*shape, seed=0, shift=0.0):
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) + shift
    return t.cuda().contiguous(memory_format=_CL)


def _bn(C, seed):
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(C, generator=g))
        bn.bias.copy_(0.1 * torch.randn(C, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(C, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
    return bn.cuda().train()


def _close(got, want, rel, scale=None):
    scale = want.abs().max().item() if scale is None else scale
    torch.testing.assert_close(got, want, rtol=rel, atol=rel * max(scale, 1e-30))


# ------------------------------------------------------------------------------------------------------------ T1
# every PSPNet channel count; odd M; M = 2 (the PPM's bin-1 branch at B = 2); C % 64 != 0
SHAPES = [(2, 64, 33, 33), (2, 128, 17, 17), (1, 256, 15, 17), (2, 512, 1, 1), (2, 1024, 9, 9), (1, 2048, 7, 9),
          (3, 12, 5, 7)]


def _run_t1(bn, x, r, g, relu):
    from semseg.models.pspnet import _BNTrain
    xi = x.clone().requires_grad_(True)
    ri = None if r is None else r.clone().requires_grad_(True)
    for p in bn.parameters():
        p.grad = None
    y = _BNTrain.apply(xi, bn.weight, bn.bias, ri, bn, relu)
    y.backward(g)
    return y.detach(), xi.grad, bn.weight.grad.clone(), bn.bias.grad.clone(), None if ri is None else ri.grad


@pytest.mark.parametrize("mode", ["plain", "relu", "residual"])
@pytest.mark.parametrize("B,C,H,W", SHAPES)
def test_t1_matches_batch_norm(B, C, H, W, mode):
    seed = B * 7 + C + H
    x = _randn(B, C, H, W, seed=seed, shift=0.5)
    g = _randn(B, C, H, W, seed=seed + 1)
    r = _randn(B, C, H, W, seed=seed + 2) if mode == "residual" else None
    relu = mode != "plain"
    # the reference in float64: torch's own fp32 batch norm (MIOpen here) loses var to cancellation on 2-row maps
    dev, ref = _bn(C, seed), _bn(C, seed).double()
    versions = (dev.running_mean._version, dev.running_var._version)
    got = _run_t1(dev, x, r, g, relu)

    xr = x.double().requires_grad_(True)
    rr = None if r is None else r.double().requires_grad_(True)
    yr = ref(xr)
    if rr is not None:
        yr = yr + rr
    if relu:
        yr = F.relu(yr)
    yr.backward(g.double())
    want = [None if t is None else t.float()
            for t in (yr.detach(), xr.grad, ref.weight.grad, ref.bias.grad, None if rr is None else rr.grad)]
    # dx = scale*(g' - mean(g') - xhat*mean(g'*xhat)) cancels to O(eps / var) of its terms where M is tiny (M = 2: exactly
    # two opposite xhat): both implementations then carry rounding of the size of the terms, so dx is judged on that scale
    var = x.double().permute(1, 0, 2, 3).reshape(C, -1).var(1, unbiased=False)
    terms = (g.double() * (ref.weight.double() / (var + ref.eps).sqrt()).view(1, C, 1, 1)).abs().max().item()
    for k, (a, b) in enumerate(zip(got, want)):
        if b is None:
            assert a is None
        else:
            _close(a, b, 1e-5, max(terms, b.abs().max().item()) if k == 1 else None)
    assert got[0].is_contiguous(memory_format=_CL)
    torch.testing.assert_close(dev.running_mean, ref.running_mean.float(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(dev.running_var, ref.running_var.float(), rtol=1e-5, atol=1e-6)
    assert int(dev.num_batches_tracked) == int(ref.num_batches_tracked) == 1
    assert dev.running_mean._version > versions[0] and dev.running_var._version > versions[1]

    again = _run_t1(_bn(C, seed), x, r, g, relu)                     # bitwise reproducible
    for a, b in zip(got, again):
        assert (a is None and b is None) or torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ P1 + dense conv
@pytest.mark.parametrize("B,C,H,W,d", [(2, 64, 13, 11, 2), (2, 32, 15, 10, 4)])
def test_dilated_train_conv(B, C, H, W, d):
    from semseg.models.pspnet import dilated_conv3x3_train
    x = _randn(B, C, H, W, seed=d)
    w = (torch.randn(48, C, 3, 3, generator=torch.Generator().manual_seed(5)) * (2.0 / (9 * C)) ** 0.5).cuda()
    g = _randn(B, 48, H, W, seed=11)
    xi, wi = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = dilated_conv3x3_train(xi, wi, d)
    y.backward(g)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = F.conv2d(xr, wr, padding=d, dilation=d)
    yr.backward(g)
    _close(y, yr, 1e-5)
    _close(xi.grad, xr.grad, 1e-5)
    _close(wi.grad, wr.grad, 1e-4)


# ------------------------------------------------------------------------------------------------------------ whole model
class _Native:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from semseg.models import pspnet
        self.old, pspnet.USE_NATIVE = pspnet.USE_NATIVE, self.on

    def __exit__(self, *a):
        from semseg.models import pspnet
        pspnet.USE_NATIVE = self.old


def _model(seed=0):
    from devtools.psp_weights import seeded_state_dict
    from semseg.models import PSPNet
    torch.manual_seed(0)
    m = PSPNet(50, 21)
    m.load_state_dict(seeded_state_dict(m.state_dict(), seed), strict=True)
    m.cls[3].p = 0.0
    m.aux[3].p = 0.0
    return m.cuda().train()


def _batch(B=2, S=129):
    g = torch.Generator().manual_seed(3)
    x = torch.rand(B, 3, S, S, generator=g).cuda()
    y = torch.randint(0, 21, (B, S, S), generator=g)
    y[torch.rand(B, S, S, generator=g) < 0.05] = -1
    return x, y.cuda()


def _train_step(model, x, y, native):
    model.zero_grad(set_to_none=True)
    with _Native(native):
        main, aux, _ = model(x, y)
    (main + 0.4 * aux).backward()
    return main.detach(), aux.detach()


def _errors(model, ref):
    """relative L2 error of the whole gradient, the worst relative L2 error of one parameter's gradient, and the worst
    running-statistics error relative to the largest entry of its buffer, of ``model`` against ``ref``"""
    pd, bd = dict(model.named_parameters()), dict(model.named_buffers())
    diffs = {k: (pd[k].grad.double() - p.grad.double(), p.grad.double()) for k, p in ref.named_parameters()}
    whole = (sum(d.norm() ** 2 for d, _ in diffs.values()) / sum(r.norm() ** 2 for _, r in diffs.values())).sqrt().item()
    worst = max(((d.norm() / r.norm().clamp_min(1e-30)).item(), k) for k, (d, r) in diffs.items())
    b_err = max(((bd[k].double() - b.double()).abs().max().item() / b.double().abs().max().clamp_min(1e-30).item(), k)
                for k, b in ref.named_buffers() if not k.endswith("num_batches_tracked"))
    return whole, worst, b_err


def test_train_step_matches_stock():
    """the device path against the same model on stock torch ops.  The yardstick runs in float64: stock fp32 batch norm
    (MIOpen) computes the variance of the PPM's 2-row bin-1 maps by cancellation, which alone moves its loss by ~1e-3
    relative at these weights (its gradients are off by up to 2x on some BatchNorm weights); the stock fp32 errors are
    printed beside the device's."""
    x, y = _batch()
    dev, ref, stock = _model(), _model().double(), _model()
    md, ad = _train_step(dev, x, y, True)
    mr, ar = _train_step(ref, x.double(), y, False)
    ms, as_ = _train_step(stock, x, y, False)
    assert torch.isfinite(md) and torch.isfinite(ad)
    _close(md.double(), mr, 1e-4)
    _close(ad.double(), ar, 1e-4)
    whole, worst, b_err = _errors(dev, ref)
    print(f"\ndevice vs fp64: loss {abs(md.item() / mr.item() - 1):.2e} / {abs(ad.item() / ar.item() - 1):.2e}, "
          f"gradient {whole:.2e}, worst parameter {worst[0]:.2e} ({worst[1]}), running stats {b_err[0]:.2e} ({b_err[1]})")
    sw, sp, sb = _errors(stock, ref)
    print(f"stock fp32 vs fp64: loss {abs(ms.item() / mr.item() - 1):.2e} / {abs(as_.item() / ar.item() - 1):.2e}, "
          f"gradient {sw:.2e}, worst parameter {sp[0]:.2e} ({sp[1]}), running stats {sb[0]:.2e} ({sb[1]})")
    # Measured: loss 4e-8 / 2e-7, gradient 2.3e-2 (dominated by layer0.1.bias: a BatchNorm bias whose ReLU output feeds a
    # convolution and another train-mode BatchNorm, which cancels most of its gradient), running stats 8e-5; stock fp32:
    # 7.8e-4 / 3.5e-5, 1.8, 3e-2.  The device path must stay an order of magnitude closer to float64 than stock fp32 is.
    assert whole <= 0.05 and whole <= 0.1 * sw, (whole, sw)
    assert b_err[0] <= 1e-3 and b_err[0] <= 0.1 * sb[0], (b_err, sb)
    assert all(int(b) == 1 for k, b in dev.named_buffers() if k.endswith("num_batches_tracked"))


def _eval_logits(model, x, native):
    model.eval()
    for p in model.parameters():
        p.requires_grad_(False)
    try:
        with torch.no_grad(), _Native(native):
            return model(x)
    finally:
        for p in model.parameters():
            p.requires_grad_(True)
        model.train()


def test_train_then_attack_sees_fresh_batchnorm():
    x, y = _batch()
    model = _model()
    _eval_logits(model, x, True)                                # builds the eval path's folded-BN / weight caches
    opt = torch.optim.SGD(model.parameters(), lr=1e-2, momentum=0.9)
    for _ in range(2):
        _train_step(model, x, y, True)
        opt.step()
    got = _eval_logits(model, x, True)
    want = _eval_logits(model, x, False)
    err = (got - want).abs().max().item()
    assert err <= 1e-3 * want.abs().max().item(), err


# ------------------------------------------------------------------------------------------------------------ train_rob_seg
def test_train_rob_seg_pspnet(tmp_path):
    from tools import train_rob_seg as T
    from semseg.models import PSPNet
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "pascalvoc_pspnet.yaml")))
    cfg["TRAIN"]["IMAGE_SIZE"] = [129, 129]
    cfg["TRAIN"]["N_ITERS"] = 2
    cfg_path = tmp_path / "psp.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    out, dump = tmp_path / "out.json", tmp_path / "params.pt"
    T.main(["--cfg", str(cfg_path), "--synthetic", "2", "--steps", "3", "--warmup", "0", "--batch_size", "2",
            "--deterministic", "--json", str(out), "--dump_params", str(dump)])
    res = json.load(open(out))
    assert res["model"] == "PSPNet-RN50" and res["image_size"] == 129 and res["inner_pgd_steps"] == 2
    assert math.isfinite(res["last_loss"])
    torch.manual_seed(0)
    init = PSPNet(50, 21).state_dict()
    params = torch.load(dump)["params"]
    changed = [not torch.equal(init[k], v) for k, v in params.items()]
    assert len(changed) >= 20 and sum(changed) >= 0.9 * len(changed), changed

    # the inner attack differentiates w.r.t. the input only
    model = PSPNet(50, 21).cuda().eval()
    x, y = _batch()
    attack = T.build_attack(dict(cfg["TRAIN"], N_CLS=21))
    x_adv = attack(model, x, y)
    assert all(p.grad is None for p in model.parameters())
    assert (x_adv - x).abs().max().item() <= 4 / 255 + 1e-6
