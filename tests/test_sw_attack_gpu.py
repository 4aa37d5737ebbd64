"""SEA through sliding windows (`-m gpu`): the window cut K11c and its adjoint K11c', the adjoint K11a' of the merge (full-res
and low-res modes) and ``segmenter_eval.SlidingWindowModel`` against CPU restatements in fp32 (bitwise where the operations
are the same) and float64, the unfused device path (M2 backward per window) and the same protocol written in ATen under
autograd; the attacks (eager and HIP-graph replay) and tools.infer through the wrapper.  Window 32: a x16 low-res window is
2 x 2 (every tap clamps), a x4 one 8 x 8."""
import copy
import glob
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
WS = 32
FILES = sorted(glob.glob(os.path.join(GOLDEN, "g16_sw_*.npz")))
# (H, W) merged size, stride: the table of test_sliding_window_gpu.py, ((40, 37), 8) (anchors [0, 8] x [0, 5]: every pixel
# but a border under four windows) and ((56, 50), 8) (anchors [0, 8, 16, 24] x [0, 8, 16, 18]: up to 4 covering per axis)
SHAPES = [((32, 32), 32), ((32, 45), 32), ((48, 61), 16), ((50, 70), 24), ((40, 37), 8), ((56, 50), 8)]
CLASSES = [5, 21, 151]
B = 2


@pytest.fixture(scope="module")
def N():
    from semseg import _native
    _native.lib()
    return _native


def _anchors(H, W, stride, ws=WS):
    from semseg.utils.segmenter_eval import sw_anchors
    return sw_anchors(H, W, ws, stride)


def _windows(ha, wa):
    return [(a, b) for a in ha for b in wa]


# ---------------------------------------------------------------------------------------------------------------- references
def _stack(x, ha, wa, ws=WS):
    """segmenter_eval.inference's cut: image-major stack of slices"""
    return torch.stack([x[:, :, a:a + ws, b:b + ws] for a, b in _windows(ha, wa)], 1).flatten(0, 1)


def _merge(seg, ha, wa, H, W, ws=WS):
    """the reference's loop (zero sum, += per window, count, divide) in seg's dtype, differentiable"""
    n_win = len(ha) * len(wa)
    s = seg.view(seg.shape[0] // n_win, n_win, seg.shape[1], ws, ws)
    logit = torch.zeros(s.shape[0], s.shape[2], H, W, dtype=seg.dtype, device=seg.device)
    count = torch.zeros(1, 1, H, W, dtype=seg.dtype, device=seg.device)
    for k, (a, b) in enumerate(_windows(ha, wa)):
        logit[:, :, a:a + ws, b:b + ws] += s[:, k]
        count[:, :, a:a + ws, b:b + ws] += 1
    return logit / count


def _count(ha, wa, H, W, ws=WS):
    count = torch.zeros(H, W)
    for a, b in _windows(ha, wa):
        count[a:a + ws, b:b + ws] += 1
    return count


def _u_axis(n_in, n_out):
    """the align_corners=False index / lambda rule in float32 (csrc/bilinear_map.h), r = in / out; for the power-of-two
    factors used here every intermediate is exact, fused or not"""
    r = np.float32(n_in) / np.float32(n_out)
    src = (r * (np.arange(n_out, dtype=np.float32) + np.float32(0.5))).astype(np.float32) - np.float32(0.5)
    src = np.maximum(src, np.float32(0)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    lam = (src - i0.astype(np.float32)).astype(np.float64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, lam


def _resize_fp64(v, size):
    (a0, a1, ly), (b0, b1, lx) = _u_axis(v.shape[2], size[0]), _u_axis(v.shape[3], size[1])
    lx, ly = torch.from_numpy(lx), torch.from_numpy(ly)[:, None]
    r0, r1 = v[:, :, a0], v[:, :, a1]
    top = (1 - lx) * r0[..., b0] + lx * r0[..., b1]
    bot = (1 - lx) * r1[..., b0] + lx * r1[..., b1]
    return (1 - ly) * top + ly * bot


def _dot64(a, b):
    return float((a.double().cpu() * b.double().cpu()).sum())


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("Cx", [3, 21])
@pytest.mark.parametrize("shape,stride", SHAPES)
def test_cut_and_its_adjoint(N, shape, stride, Cx):
    H, W = shape
    ha, wa = _anchors(H, W, stride)
    n_win = len(ha) * len(wa)
    g = torch.Generator().manual_seed(Cx * 7 + W + stride)
    x = torch.rand(B, Cx, H, W, generator=g)
    crops = N.sw_cut(x.to(DEV), WS, ha, wa)
    assert tuple(crops.shape) == (B * n_win, Cx, WS, WS)
    assert torch.equal(crops.cpu(), _stack(x, ha, wa))
    d = torch.rand(B * n_win, Cx, WS, WS, generator=g) * 2 - 1            # magnitude ~1
    want32 = torch.zeros(B, Cx, H, W)
    want64 = torch.zeros(B, Cx, H, W, dtype=torch.float64)
    dv = d.view(B, n_win, Cx, WS, WS)
    for k, (a, b) in enumerate(_windows(ha, wa)):                          # anchor order, ha outer, wa inner
        want32[:, :, a:a + WS, b:b + WS] += dv[:, k]
        want64[:, :, a:a + WS, b:b + WS] += dv[:, k].double()
    d_dev = d.to(DEV)
    got = N.sw_cut_backward(d_dev, WS, ha, wa, (H, W))
    err = (got.cpu().double() - want64).abs().max().item()
    print(f"Cx={Cx} {shape} stride {stride}: {n_win} windows, cut backward max |err vs fp64| {err:.2e}")
    assert torch.equal(got.cpu(), want32)
    # 1e-6 on the first five shapes (at most 6 covering windows, at (48, 61)).  The sixth has 16: there the bound is the
    # fp32 worst case, every one of the n - 1 adds rounds a partial sum of magnitude <= n by at most half an ulp,
    # (n - 1) * n * 2^-24 = 1.4e-5
    n_cover = int(_count(ha, wa, H, W).max())
    assert n_cover <= 6 or shape == (56, 50)
    assert err <= (1e-6 if n_cover <= 6 else (n_cover - 1) * n_cover * 2.0 ** -24)
    assert torch.equal(N.sw_cut_backward(d_dev, WS, ha, wa, (H, W)), got)   # no atomics: bitwise reproducible


# ---------------------------------------------------------------------------------------------------------------- 2
def _fullres_case(N, C, ha, wa, H, W, seed):
    n_win = len(ha) * len(wa)
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(B, C, H, W, generator=gen) * 3
    seg = torch.randn(B * n_win, C, WS, WS, generator=gen).requires_grad_(True)
    (want,) = torch.autograd.grad(_merge(seg, ha, wa, H, W), [seg], g)      # CPU fp32 autograd through logit / count
    got = N.sw_merge_backward(g.to(DEV), WS, ha, wa, (WS, WS))
    assert tuple(got.shape) == tuple(seg.shape)
    n_diff = int((got.cpu() != want).sum())
    print(f"C={C} ({H}, {W}) anchors {ha} x {wa}: {n_diff} elements differ from CPU autograd")
    assert torch.equal(got.cpu(), want)
    assert torch.equal(N.sw_merge_backward(g.to(DEV), WS, ha, wa, (WS, WS)), got)


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("shape,stride", SHAPES)
def test_merge_backward_fullres_is_cpu_autograd_bit_for_bit(N, C, shape, stride):
    ha, wa = _anchors(*shape, stride)
    _fullres_case(N, C, ha, wa, *shape, seed=C * 13 + shape[1] + stride)


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_merge_backward_fullres_on_the_golden_anchors(N, path):
    g = np.load(path)
    H, W = (int(v) for v in g["shape"])
    _fullres_case(N, int(g["n_classes"]), g["h_anchors"].tolist(), g["w_anchors"].tolist(), H, W, seed=H * W)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("r", [4, 16])
@pytest.mark.parametrize("shape,stride", SHAPES)
def test_merge_backward_lowres_vs_fp64_and_the_unfused_path(N, C, r, shape, stride):
    """error against the float64 adjoint, bounded by twice the error of the parent's unfused device path (the window's
    g / count, then M2's backward) + 1e-7 max|want|; and <sw_merge(v), g> == <v, sw_merge_backward(g)>"""
    H, W = shape
    ha, wa = _anchors(H, W, stride)
    n_win, hl = len(ha) * len(wa), WS // r
    gen = torch.Generator().manual_seed(C * 5 + r + W + stride)
    g = torch.randn(B, C, H, W, generator=gen) * 3
    low = torch.zeros(B * n_win, C, hl, hl, dtype=torch.float64, requires_grad=True)
    (want,) = torch.autograd.grad(_merge(_resize_fp64(low, (WS, WS)), ha, wa, H, W), [low], g.double())
    g_dev = g.to(DEV)
    got = N.sw_merge_backward(g_dev, WS, ha, wa, (hl, hl))
    assert tuple(got.shape) == (B * n_win, C, hl, hl)
    quot = g_dev / _count(ha, wa, H, W).to(DEV)
    unfused = N.upsample_bilinear_backward(_stack(quot, ha, wa).contiguous(), (hl, hl))
    err_new = (got.cpu().double() - want).abs().max().item()
    err_unf = (unfused.cpu().double() - want).abs().max().item()
    scale = want.abs().max().item()
    print(f"C={C} x{r} {shape} stride {stride}: max |err vs fp64| fused {err_new:.3e}, unfused {err_unf:.3e}, "
          f"max |want| {scale:.3e}")
    assert err_new <= 2 * err_unf + 1e-7 * scale
    assert torch.equal(N.sw_merge_backward(g_dev, WS, ha, wa, (hl, hl)), got)
    v = (torch.randn(B * n_win, C, hl, hl, generator=gen) * 3).to(DEV)
    lhs, rhs = _dot64(N.sw_merge(v, WS, ha, wa, shape), g_dev), _dot64(v, got)
    print(f"    <merge(v), g> {lhs:.9e}   <v, merge_backward(g)> {rhs:.9e}")
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))


# ---------------------------------------------------------------------------------------------------------------- 4
def _aten_protocol(net, x, ha, wa, ws=WS):
    """the wrapper's protocol in ATen operations under autograd: slice stack, model, zero buffer + `+=`, / count"""
    return _merge(net(_stack(x, ha, wa, ws)), ha, wa, x.shape[2], x.shape[3], ws)


def _nets(name, C):
    from oracle.tiny_models import PointwiseNet, TinyConvNet
    return (TinyConvNet if name == "conv" else PointwiseNet)(C, seed=C + 3)


@pytest.mark.parametrize("net_name,C,batch", [("pw", 21, 3), ("pw", 5, None), ("conv", 5, None), ("conv", 21, None)])
@pytest.mark.parametrize("shape,stride", [((32, 45), 32), ((48, 61), 16), ((40, 37), 8)])
def test_wrapper_vs_the_aten_composition(N, net_name, C, batch, shape, stride):
    from semseg.utils.segmenter_eval import SlidingWindowModel
    H, W = shape
    ha, wa = _anchors(H, W, stride)
    cpu_net = _nets(net_name, C)
    net = copy.deepcopy(cpu_net).to(DEV)
    gen = torch.Generator().manual_seed(C + W + stride)
    x = torch.rand(B, 3, H, W, generator=gen)
    dl = torch.randn(B, C, H, W, generator=gen)
    x64 = x.double().requires_grad_(True)
    (want,) = torch.autograd.grad(_aten_protocol(copy.deepcopy(cpu_net).double(), x64, ha, wa), [x64], dl.double())
    xd = x.to(DEV).requires_grad_(True)
    wrapped = SlidingWindowModel(net, WS, stride, batch)
    out = wrapped(xd)
    (got,) = torch.autograd.grad(out, [xd], dl.to(DEV))
    xa = x.to(DEV).requires_grad_(True)
    out_aten = _aten_protocol(net, xa, ha, wa)
    (got_aten,) = torch.autograd.grad(out_aten, [xa], dl.to(DEV))
    d_out = (out - out_aten).abs().max().item()
    err_new = (got.cpu().double() - want).abs().max().item()
    err_aten = (got_aten.cpu().double() - want).abs().max().item()
    scale = want.abs().max().item()
    print(f"{net_name} C={C} {shape} stride {stride}: max |logits - ATen| {d_out:.2e}; input gradient max |err vs fp64| "
          f"wrapper {err_new:.3e}, ATen on the device {err_aten:.3e}, max |want| {scale:.3e}")
    assert tuple(out.shape) == (B, C, H, W)
    if net_name == "pw":                      # explicit element-wise arithmetic: no library freedom
        assert torch.equal(out, out_aten)
    else:
        assert d_out <= 1e-6
    assert err_new <= 2 * err_aten + 1e-7 * scale


class _UpM2(torch.autograd.Function):
    """a model's own final up-sampling on the device, as the real models do it: M2 forward, M2 backward"""

    @staticmethod
    def forward(ctx, low, size):
        from semseg import _native
        ctx.in_size = tuple(low.shape[2:])
        return _native.upsample_bilinear(low.contiguous(), size)

    @staticmethod
    def backward(ctx, g):
        from semseg import _native
        return _native.upsample_bilinear_backward(g.contiguous(), ctx.in_size), None


class _LowresNet(torch.nn.Module):
    """PointwiseNet on the r x r average-pooled image, up-sampled by r: a miniature of the models with a
    ``forward_lowres`` hook (a tuple whose first entry is the logits before the final up-sampling)"""

    def __init__(self, C, r):
        super().__init__()
        from oracle.tiny_models import PointwiseNet
        self.net, self.r = PointwiseNet(C, seed=C + r), r
        self.eval()

    def forward_lowres(self, x):
        return (self.net(torch.nn.functional.avg_pool2d(x, self.r)),)

    def forward(self, x):
        low = self.forward_lowres(x)[0]
        size = tuple(x.shape[2:])
        return _UpM2.apply(low, size) if x.is_cuda else _resize_fp64(low, size)


@pytest.mark.parametrize("C", [21, 151])
@pytest.mark.parametrize("r", [4, 16])
@pytest.mark.parametrize("shape,stride,batch", [((48, 61), 16, None), ((40, 37), 8, 3)])
def test_wrapper_lowres_route_vs_the_aten_composition(N, C, r, shape, stride, batch, monkeypatch):
    """a model with the hook: the wrapper feeds ``forward_lowres`` logits to K11a / K11a' in low-res mode; the composition
    runs the model's own up-sampling per window, then zero buffer, `+=`, / count"""
    from semseg import _native
    from semseg.utils.segmenter_eval import SlidingWindowModel
    H, W = shape
    ha, wa = _anchors(H, W, stride)
    cpu_net = _LowresNet(C, r)
    net = copy.deepcopy(cpu_net).to(DEV)
    gen = torch.Generator().manual_seed(C + r + W)
    x = torch.rand(B, 3, H, W, generator=gen)
    dl = torch.randn(B, C, H, W, generator=gen)
    x64 = x.double().requires_grad_(True)
    (want,) = torch.autograd.grad(_aten_protocol(copy.deepcopy(cpu_net).double(), x64, ha, wa), [x64], dl.double())
    seen = []
    real = _native.sw_merge_backward

    def spy(g, ws, h_anchors, w_anchors, logits_size):
        seen.append(tuple(logits_size))
        return real(g, ws, h_anchors, w_anchors, logits_size)

    monkeypatch.setattr(_native, "sw_merge_backward", spy)
    xd = x.to(DEV).requires_grad_(True)
    out = SlidingWindowModel(net, WS, stride, batch)(xd)
    (got,) = torch.autograd.grad(out, [xd], dl.to(DEV))
    assert seen == [(WS // r, WS // r)], seen                       # the low-res adjoint ran
    xa = x.to(DEV).requires_grad_(True)
    out_aten = _aten_protocol(net, xa, ha, wa)
    (got_aten,) = torch.autograd.grad(out_aten, [xa], dl.to(DEV))
    err_new = (got.cpu().double() - want).abs().max().item()
    err_aten = (got_aten.cpu().double() - want).abs().max().item()
    scale = want.abs().max().item()
    print(f"low-res hook C={C} x{r} {shape} stride {stride}: max |logits - ATen| {(out - out_aten).abs().max().item():.2e}; "
          f"input gradient max |err vs fp64| wrapper {err_new:.3e}, ATen on the device {err_aten:.3e}, max |want| {scale:.3e}")
    assert tuple(out.shape) == (B, C, H, W)
    assert torch.equal(out, out_aten)         # K11a's in-kernel up-sampling has M2's bits; the rest is element-wise
    assert err_new <= 2 * err_aten + 1e-7 * scale


# ---------------------------------------------------------------------------------------------------------------- 5
def _attack_setup(wrap, shape, seed):
    """images, labels (the wrapper's clean prediction, a tenth flipped to a random class, a twentieth ignored) and weights"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, *shape, generator=gen).to(DEV)
    w = torch.rand(21, generator=gen).to(DEV)
    with torch.no_grad():
        y = wrap(x).max(1)[1].cpu()
    y = torch.where(torch.rand(y.shape, generator=gen) < 0.1, torch.randint(0, 21, y.shape, generator=gen), y)
    y = torch.where(torch.rand(y.shape, generator=gen) < 0.05, torch.full_like(y, -1), y)
    return x, y.to(DEV), w


@pytest.mark.parametrize("net_name", ["pw", "conv"])
def test_one_window_is_the_bare_model(N, net_name):
    from semseg import attacker as A
    from semseg.utils.segmenter_eval import SlidingWindowModel
    net = _nets(net_name, 21).to(DEV)
    wrap = SlidingWindowModel(net, WS, 16)
    x, y, w = _attack_setup(wrap, (WS, WS), 41)
    dl = torch.randn(B, 21, WS, WS, generator=torch.Generator().manual_seed(5)).to(DEV)
    outs = []
    for m in (net, wrap):
        xi = x.clone().requires_grad_(True)
        o = m(xi)
        outs.append((o.detach(), torch.autograd.grad(o, [xi], dl)[0]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    runs = [A.apgd_train(m, x, y, "Linf", 8.0 / 255, n_iter=14, loss="mask-ce-avg", early_stop=True, track_loss="ce-avg",
                         num_classes=21, weights=w, return_pred=True) for m in (net, wrap)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    A.release_graph_cache(net)
    A.release_graph_cache(wrap)


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("loss", ["mask-ce-avg", "js-avg"])
def test_graph_replay_is_bitwise_the_eager_loop(N, loss, monkeypatch, capfd):
    from semseg import attacker as A
    from semseg.utils.segmenter_eval import SlidingWindowModel
    net = _nets("pw", 21).to(DEV)
    wrap = SlidingWindowModel(net, WS, 16)
    x, y, w = _attack_setup(wrap, (48, 61), 43)
    eps = 8.0 / 255
    captures = []
    real = A.ApgdRun._capture

    def counting(self, i):
        r = real(self, i)
        captures.append(self.own.graphs is not None)
        return r

    monkeypatch.setattr(A.ApgdRun, "_capture", counting)
    outs = []
    for graph in (False, True):
        monkeypatch.setattr(A, "USE_HIP_GRAPH", graph)
        A.release_graph_cache(wrap)
        outs.append(A.apgd_train(wrap, x, y, "Linf", eps, n_iter=14, loss=loss, early_stop=True, track_loss="ce-avg",
                                 num_classes=21, weights=w, return_pred=True))
        if not graph:
            assert captures == []
    A.release_graph_cache(wrap)
    assert captures == [True], captures                              # the second run captured its pair and replayed it
    assert "continuing with the eager loop" not in capfd.readouterr().err
    assert len(outs[0]) == 5
    for a, b in zip(outs[0][:4], outs[1][:4]):
        assert torch.equal(a, b)
    assert torch.equal(outs[0][4], outs[1][4])
    assert (outs[1][3] - x).abs().max().item() <= eps * (1 + 1e-6)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_apgd_largereps_through_the_wrapper(N):
    from semseg import attacker as A
    from semseg.utils.segmenter_eval import SlidingWindowModel
    net = _nets("conv", 21).to(DEV)
    wrap = SlidingWindowModel(net, WS, 16, batch_size=4)
    x, y, w = _attack_setup(wrap, (40, 53), 47)
    eps = 8.0 / 255
    with torch.no_grad():
        clean = ((wrap(x).max(1)[1] == y) & (y != -1)).flatten(1).sum(1).float() / float(y[0].numel())
    x_adv, _, acc, pred = A.apgd_largereps(wrap, x, y, w, eps=eps, n_iter=15, loss="mask-ce-avg", num_classes=21,
                                           track_loss="ce-avg", return_pred=True)
    A.release_graph_cache(wrap)
    print(f"clean pixel accuracy {clean.tolist()}, after the attack {acc.tolist()}")
    assert tuple(x_adv.shape) == tuple(x.shape) and tuple(acc.shape) == (B,) and tuple(pred.shape) == (B, 40, 53)
    assert (x_adv - x).abs().max().item() <= eps * (1 + 1e-6)
    assert bool((acc <= clean).all())


# ---------------------------------------------------------------------------------------------------------------- 8
def test_surface(N):
    from semseg.utils.segmenter_eval import SlidingWindowModel
    net = _nets("pw", 5).to(DEV)
    wrap = SlidingWindowModel(net, WS, 16)
    with pytest.raises(ValueError):
        wrap(torch.rand(1, 3, 20, 40, device=DEV))                   # smaller than the window: no resizing here
    with pytest.raises(ValueError):
        wrap(torch.rand(1, 3, 40, 31, device=DEV))
    with pytest.raises(ValueError):
        SlidingWindowModel(net, 32, 33)
    assert not hasattr(wrap, "forward_lowres")
    assert wrap.training is False
    net.train()
    assert wrap.training is True
    wrap.eval()
    assert net.training is False and wrap.training is False
    assert [n for n, _ in wrap.named_buffers()] == ["model.W", "model.b"]


# ---------------------------------------------------------------------------------------------------------------- 9
def test_infer_tool_through_windows(N, tmp_path):
    from tools import infer
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "pascalvoc_convnext.yaml")))
    cfg["SAVE_DIR"] = str(tmp_path) + "/"
    cfg_path = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(cfg_path, "w"))
    g = torch.Generator().manual_seed(9)
    images = torch.rand(4, 3, 64, 96, generator=g)
    labels = torch.randint(0, 21, (4, 64, 96), generator=g)
    labels[torch.rand(4, 64, 96, generator=g) < 0.05] = -1
    data = str(tmp_path / "data.pt")
    torch.save({"images": images, "labels": labels}, data)
    args = ["--cfg", cfg_path, "--eps", "8", "--n_iter", "12", "--data", data, "--random_init", "--batch_size", "2",
            "--window", "64", "--stride", "32", "--cleanup", "0", "--save_argmax", "--deterministic"]
    name = "UperNet_ConvNeXt-T_CVST"
    results = []
    for tag in ("a", "b"):
        s = infer.main(args + ["--json", str(tmp_path / f"{tag}.json")])
        assert os.path.exists(tmp_path / f"{tag}.json")
        assert os.path.exists(os.path.join(str(tmp_path), f"worse_SEA_{name}_{cfg['EVAL']['NAME']}_8.0.pt"))
        logs = [torch.load(os.path.join(str(tmp_path), "argmax-logs", f"{name}_{l}_8.0.pt")) for l in infer.LOSSES]
        for lg in logs:
            assert lg.shape == (4, 64, 96) and lg.dtype == torch.int64
            assert torch.equal(lg == -1, labels == -1)
        results.append((s, logs))
    (s1, l1), (s2, l2) = results
    assert s1["n_images"] == 4 and 0.0 <= s1["worst_Acc"] <= min(s1["worst_Acc_indiv"]) + 1e-9
    for k in ("clean", "worst_Acc", "final_miou", "worst_Acc_indiv", "loss-wise_miou"):
        assert s1[k] == s2[k], (k, s1[k], s2[k])
    for a, b in zip(l1, l2):
        assert torch.equal(a, b)
