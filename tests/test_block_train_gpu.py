"""T3: the train-mode ConvNeXt block in NHWC on the device -- LayerNorm with parameter gradients (T3a), the fused layer-scale /
stochastic-depth / residual tail (T3b), their wiring into Block / LayerNorm behind TRAIN_NATIVE_BLOCKS, and
tools.train_rob_seg --native-blocks.

Accuracy rule (tests/test_train_loss_gpu.py, README "asserted <= 2 x"): the yardstick is a float64 evaluation of the same
formula on the same inputs; the kernel's largest error against it must be at most twice that of the stock fp32 device
composition, with a floor of one fp32 ulp of the largest magnitude of the compared tensor.  Every pair is printed before it
is asserted; the measured pairs are in DESIGN section 5, T3."""
import copy
import math
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ulp32(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(abs(x))) - 23) if x and math.isfinite(x) else 2.0 ** -149


def yardstick(tag, got, stock, want):
    want = want.double().cpu()
    e_got = float((got.double().cpu() - want).abs().max())
    e_stock = float((stock.double().cpu() - want).abs().max())
    floor = ulp32(float(want.abs().max()))
    print(f"[T3 {tag}] err T3 {e_got:.3e} stock {e_stock:.3e} floor {floor:.2e}")
    assert e_got <= max(2 * e_stock, floor), (tag, e_got, e_stock, floor)


class _Switch:
    """TRAIN_NATIVE_BLOCKS for the duration of a `with`"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from semseg.models import convnext_upernet as M
        self.M, self.old = M, M.TRAIN_NATIVE_BLOCKS
        M.TRAIN_NATIVE_BLOCKS = self.on

    def __exit__(self, *exc):
        self.M.TRAIN_NATIVE_BLOCKS = self.old
        return False


# ------------------------------------------------------------------------------------------------------------ T3a
LN_CASES = [(rows, C) for C in (48, 96, 192, 384, 768, 1024) for rows in (1, 15, 17, 257)] + [(70001, 96)]


@pytest.mark.parametrize("rows,C", LN_CASES, ids=[f"r{r}_c{c}" for r, c in LN_CASES])
def test_layernorm_backward_params(rows, C):
    from semseg import _native as N
    gen = torch.Generator().manual_seed(1000 * C + rows)
    x = torch.randn(rows, C, generator=gen) * 2 + 0.5
    w = torch.rand(C, generator=gen) + 0.5
    b = torch.randn(C, generator=gen)
    g = torch.randn(rows, C, generator=gen)
    eps = 1e-6

    def autograd(xx, ww, bb, gg):
        xx, ww, bb = (t.clone().requires_grad_(True) for t in (xx, ww, bb))
        F.layer_norm(xx, (C,), ww, bb, eps).backward(gg)
        return xx.grad, ww.grad, bb.grad

    _, dw64, db64 = autograd(x.double(), w.double(), b.double(), g.double())
    xd, wd, bd, gd = (t.to(DEV) for t in (x, w, b, g))
    _, dw_s, db_s = autograd(xd, wd, bd, gd)
    _, mean, rstd = N.layernorm(xd, wd, bd, eps)
    dx0 = N.layernorm_backward(gd, xd, wd, mean, rstd)
    dx, dw, db = N.layernorm_backward_params(gd, xd, wd, mean, rstd)
    assert torch.equal(dx, dx0)
    yardstick(f"ln dw rows={rows} C={C}", dw, dw_s, dw64)
    yardstick(f"ln db rows={rows} C={C}", db, db_s, db64)
    dx2, dw2, db2 = N.layernorm_backward_params(gd, xd, wd, mean, rstd)
    assert torch.equal(dx2, dx) and torch.equal(dw2, dw) and torch.equal(db2, db)


def test_layernorm_train_function_returns_all_three_gradients():
    """_LayerNormHipTrain through LayerNorm.forward (both data formats): forward bits of the frozen path, gradients for x, w, b"""
    from semseg import _native as N
    from semseg.models import convnext_upernet as M
    calls = []
    orig = N.layernorm_backward_params
    N.layernorm_backward_params = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        for fmt in ("channels_last", "channels_first"):
            torch.manual_seed(3)
            ln = M.LayerNorm(96, data_format=fmt).to(DEV)
            with torch.no_grad():
                ln.weight.uniform_(0.5, 1.5)
                ln.bias.normal_()
            x = torch.randn((2, 5, 7, 96) if fmt == "channels_last" else (2, 96, 6, 6), device=DEV)
            outs = {}
            for on in (False, True):
                xx = x.clone().requires_grad_(True)
                ln.zero_grad()
                n0 = len(calls)
                with _Switch(on):
                    y = ln(xx)
                    y.square().sum().backward()
                assert (len(calls) - n0) == (1 if on else 0)
                outs[on] = (y.detach(), xx.grad, ln.weight.grad.clone(), ln.bias.grad.clone())
            ln.requires_grad_(False)
            assert torch.equal(outs[True][0], ln(x))          # the frozen path's forward bits
            ln.requires_grad_(True)
            for a, b in zip(outs[True], outs[False]):
                torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)
    finally:
        N.layernorm_backward_params = orig


# ------------------------------------------------------------------------------------------------------------ T3b
TAIL_SHAPES = [(1, 1, 1, 4), (3, 5, 7, 96), (4, 12, 12, 100), (2, 9, 9, 768)]


def _tail_s(kind, B, keep=0.75):
    if kind == "none":
        return None
    s = torch.full((B, 1, 1, 1), 1.0 / keep)
    if kind == "one_dropped":
        s[B // 2] = 0.0
    elif kind == "all_dropped":
        s.zero_()
    return s


@pytest.mark.parametrize("skind", ["none", "all_kept", "one_dropped", "all_dropped"])
@pytest.mark.parametrize("with_gamma", [True, False], ids=["gamma", "nogamma"])
@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=["x".join(map(str, s)) for s in TAIL_SHAPES])
def test_block_tail(shape, with_gamma, skind):
    from semseg import _native as N
    B, H, W, C = shape
    gen = torch.Generator().manual_seed(B * 1000 + C)
    x, y, g = (torch.randn(shape, generator=gen) for _ in range(3))
    gamma = torch.randn(C, generator=gen) if with_gamma else None
    s = _tail_s(skind, B)

    def compose(xx, yy, gm, ss, gg):
        yy = yy.clone().requires_grad_(True)
        gm = None if gm is None else gm.clone().requires_grad_(True)
        t = yy if gm is None else yy * gm
        out = xx + (t if ss is None else t * ss)
        out.backward(gg)
        return out.detach(), yy.grad, None if gm is None else gm.grad

    dbl = lambda t: None if t is None else t.double()
    dev = lambda t: None if t is None else t.to(DEV)
    out64, gy64, gg64 = compose(x.double(), y.double(), dbl(gamma), dbl(s), g.double())
    xd, yd, gd, gmd, sd = dev(x), dev(y), dev(g), dev(gamma), dev(s)
    out_s, gy_s, gg_s = compose(xd, yd, gmd, sd, gd)
    tag = f"tail {'x'.join(map(str, shape))} gamma={with_gamma} s={skind}"
    out = N.block_tail(xd, yd, gmd, sd)
    gy, gg = N.block_tail_backward(gd, yd, gmd, sd, with_gamma)
    yardstick(tag + " out", out, out_s, out64)
    yardstick(tag + " gy", gy, gy_s, gy64)
    if s is not None:
        for b in range(B):
            if float(s[b]) == 0.0:
                assert torch.equal(out[b], xd[b]) and not bool(gy[b].any())
    if with_gamma:
        yardstick(tag + " ggamma", gg, gg_s, gg64)
        gy2, gg2 = N.block_tail_backward(gd, yd, gmd, sd, True)
        assert torch.equal(gg2, gg) and torch.equal(gy2, gy)
        assert N.block_tail_backward(gd, None, gmd, sd, False)[1] is None
    else:
        assert gg is None
    assert torch.equal(N.block_tail(xd, yd, gmd, sd), out)


# ------------------------------------------------------------------------------------------------------------ Block
class _FixedDrop(torch.nn.Module):
    """StochasticDepth with the mask imposed"""

    def __init__(self, mask, keep):
        super().__init__()
        self.mask, self.keep = mask, keep

    def forward(self, x):
        return x * self.mask / self.keep


BLOCK_SEED = 0


@pytest.mark.parametrize("dim", [96, 192])
def test_block_train_mode_matches_float64(dim):
    from semseg.models import convnext_upernet as M
    torch.manual_seed(dim)
    blk = M.Block(dim, drop_path=0.5).to(DEV).train()
    with torch.no_grad():
        for p in blk.parameters():
            p.copy_(torch.randn_like(p) * (0.2 if p.ndim > 1 else 0.5))
        blk.norm.weight.add_(1.0)
        blk.gamma.add_(1.0)
    names = [k for k, _ in blk.named_parameters()]
    x0 = torch.randn(4, dim, 12, 12, device=DEV).contiguous(memory_format=torch.channels_last)
    g = torch.randn(4, dim, 12, 12, device=DEV).contiguous(memory_format=torch.channels_last)

    def run(b, x, gg, on):
        x = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
        b.zero_grad()
        torch.cuda.manual_seed(BLOCK_SEED)
        with _Switch(on):
            out = b(x)
        out.backward(gg)
        return [out.detach(), x.grad] + [p.grad.clone() for p in b.parameters()]

    off = run(blk, x0, g, False)
    on = run(blk, x0, g, True)
    dropped_off = [bool(torch.equal(off[0][i], x0[i])) for i in range(4)]
    dropped_on = [bool(torch.equal(on[0][i], x0[i])) for i in range(4)]
    print(f"[T3 block dim={dim}] dropped images off {dropped_off} on {dropped_on}")
    assert any(dropped_off) and not all(dropped_off), dropped_off
    assert dropped_on == dropped_off

    blk64 = copy.deepcopy(blk).cpu().double().train()
    mask = torch.tensor([0.0 if d else 1.0 for d in dropped_off], dtype=torch.float64).view(4, 1, 1, 1)
    blk64.drop_path = _FixedDrop(mask, 0.5)
    want = run(blk64, x0.cpu().double(), g.cpu().double(), False)
    for name, a, s, w in zip(["out", "dx"] + names, on, off, want):
        assert bool(torch.isfinite(a).all())
        yardstick(f"block dim={dim} {name}", a, s, w)


# ------------------------------------------------------------------------------------------------------------ routing
def test_trunk_routing_and_eval_bits():
    from semseg import _native as N
    from semseg.models import convnext_upernet as M
    torch.manual_seed(0)
    net = M.ConvNeXt("T_CVST").to(DEV)
    n_blocks = sum(len(st) for st in net.stages)
    x = torch.rand(2, 3, 64, 64, device=DEV)
    counts = {"layernorm_backward_params": 0, "block_tail": 0}
    orig = {k: getattr(N, k) for k in counts}

    def counted(k):
        def f(*a, **kw):
            counts[k] += 1
            return orig[k](*a, **kw)
        return f

    def eval_logits():
        net.eval().requires_grad_(False)
        with torch.no_grad():
            out = [f.clone() for f in net(x)]
        net.requires_grad_(True)
        return out

    for k in counts:
        setattr(N, k, counted(k))
    try:
        with _Switch(False):
            before = eval_logits()
        with _Switch(True):
            after = eval_logits()
            assert counts == {"layernorm_backward_params": 0, "block_tail": 0}, counts   # eval mode, frozen weights
            net.train()
            torch.cuda.manual_seed(1)
            sum(f.square().mean() for f in net(x)).backward()
            print(f"[T3 routing] {n_blocks} blocks: {counts}")
            assert counts["block_tail"] >= n_blocks and counts["layernorm_backward_params"] >= n_blocks, counts
            for k, p in net.named_parameters():
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        for a, b in zip(before, after):
            assert torch.equal(a, b)
        for k in counts:
            counts[k] = 0
        net.zero_grad()
        with _Switch(False):
            net.train()
            torch.cuda.manual_seed(1)
            sum(f.square().mean() for f in net(x)).backward()
        assert counts == {"layernorm_backward_params": 0, "block_tail": 0}, counts
    finally:
        for k in counts:
            setattr(N, k, orig[k])


# ------------------------------------------------------------------------------------------------------------ tool
def test_train_rob_seg_native_blocks():
    from semseg.models import convnext_upernet as M
    from tools import train_rob_seg as T
    assert M.TRAIN_NATIVE_BLOCKS is False            # the suite runs with the default
    res = T.main(["--cfg", os.path.join(PKG, "configs", "pascalvoc_convnext.yaml"), "--native-blocks", "--steps", "2",
                  "--warmup", "1", "--batch_size", "2", "--synthetic", "2", "--deterministic"])
    assert M.TRAIN_NATIVE_BLOCKS is False
    assert res["native_blocks"] is True and math.isfinite(res["last_loss"]), res
    # restored, not reset: a run that ends early with the switch already on leaves it on
    with _Switch(True):
        with pytest.raises(FileNotFoundError):
            T.main(["--cfg", os.path.join(PKG, "configs", "no_such_config.yaml"), "--native-blocks"])
        assert M.TRAIN_NATIVE_BLOCKS is True
        M.TRAIN_NATIVE_BLOCKS = False
        with pytest.raises(FileNotFoundError):
            T.main(["--cfg", os.path.join(PKG, "configs", "no_such_config.yaml"), "--native-blocks"])
        assert M.TRAIN_NATIVE_BLOCKS is False
