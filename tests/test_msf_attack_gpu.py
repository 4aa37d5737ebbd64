"""SEA through multi-scale + flip (`-m gpu`): the adjoint K10r' of the align_corners=True resize (input form K10a' and
mirrored-source form) against a CPU fp32 restatement in the documented order (bitwise) and float64; K10g + K10r' (+ M2's
backward) = the backward of one K10b pass against float64 CPU autograd with fp32 ATen on the CPU as the yardstick;
``semseg.utils.msf_model.MsfModel`` against ``evaluate_msf``'s score buffer (bitwise) and the float64 protocol; the attacks
(eager and HIP-graph replay) and tools.infer through the wrapper."""
import copy
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from conftest import PKG

from semseg.utils.msf_model import MsfModel          # without the feature this file fails here

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
B = 2
FLT_MIN = float(torch.finfo(torch.float32).tiny)
U = 2.0 ** -24                                         # unit roundoff of fp32


@pytest.fixture(scope="module")
def N():
    from semseg import _native
    _native.lib()
    return _native


def _ulp4(want):
    """4 ulp of the largest magnitude of ``want``"""
    return 4.0 * float(np.spacing(np.float32(want.abs().max().item())))


# ---------------------------------------------------------------------------------------------------------------- 1: K10r'
def _ac_axis(n_in, n_out):
    """ATen's align_corners=True rule in float32, as csrc/msf_map.h: i0, i1 and the two tap weights 1 - lam, lam (fp32)"""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    src = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    lam = np.clip((src - i0.astype(np.float32)).astype(np.float32), np.float32(0), np.float32(1)).astype(np.float32)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (np.float32(1) - lam).astype(np.float32), lam


PAIRS = [((32, 64), (64, 96)), ((64, 96), (64, 96)), ((128, 192), (64, 96)), ((96, 128), (40, 56)), ((32, 32), (40, 56)),
         ((8, 8), (1, 5))]
MODES = ["plain", "mirrored_source", "plain_and_mirrored_destination"]
PLANES = 2 * 21


@functools.lru_cache(maxsize=None)
def _k10r_reference(src, dst, mode):
    """gradients (PLANES, H, W) uniform in [-1, 1] and the adjoint in the documented order: fp32 (the kernel's operations),
    float64 (exact sums of the forward's fp32 tap weights times g), sum of |term| and the number of terms per element.
    Computed once per (grids, mode); the 3-plane cases read its first planes."""
    (h, w), (H, W) = src, dst
    rng = np.random.default_rng(h * 1000 + w + 7 * H + MODES.index(mode))
    g = rng.uniform(-1, 1, (PLANES, H, W)).astype(np.float32)
    gf = rng.uniform(-1, 1, (PLANES, H, W)).astype(np.float32) if mode == MODES[2] else None
    a0, a1, wy0, wy1 = _ac_axis(h, H)
    b0, b1, wx0, wx1 = _ac_axis(w, W)
    src_flip = mode == MODES[1]
    out32 = np.zeros((PLANES, h, w), np.float32)
    out64 = np.zeros((PLANES, h, w), np.float64)
    abs64 = np.zeros((PLANES, h, w), np.float64)
    nterm = np.zeros((h, w), np.int64)
    for mirrored, grad in ((False, g), (True, gf)):                # all plain terms first, then the mirrored ones
        if grad is None:
            continue
        for Y in range(H):                                          # Y ascending, then X ascending
            for X in range(W):
                gv = grad[:, Y, W - 1 - X if mirrored else X]
                gv64 = gv.astype(np.float64)
                for i, wy in ((a0[Y], wy0[Y]), (a1[Y], wy1[Y])):    # row tap 0 before row tap 1
                    for j, wx in ((b0[X], wx0[X]), (b1[X], wx1[X])):     # column tap 0 before column tap 1
                        c = w - 1 - j if src_flip else j
                        out32[:, i, c] += (wy * wx) * gv            # numpy float32 scalars: every operation rounds to fp32
                        t = (float(wy) * float(wx)) * gv64
                        out64[:, i, c] += t
                        abs64[:, i, c] += np.abs(t)
                        nterm[i, c] += 1
    return g, gf, out32, out64, abs64, nterm


def _k10r_device(N, g, gf, in_size, src_flip):
    """(1, P, H, W) device gradients -> (1, P, h, w)"""
    if not src_flip:
        return N.msf_resize_input_backward(g, gf, in_size)
    _, P, H, W = g.shape
    out = torch.empty(1, P, *in_size, device=DEV)
    rc = N.lib().sea_msf_resize_bwd(g.data_ptr(), None, out.data_ptr(), P, in_size[0], in_size[1], H, W, 1,
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return out


@pytest.mark.parametrize("planes", [3, PLANES])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("src,dst", PAIRS)
def test_resize_adjoint(N, src, dst, mode, planes):
    g, gf, out32, out64, abs64, nterm = _k10r_reference(src, dst, mode)
    P, (h, w), (H, W) = planes, src, dst
    g_d = torch.from_numpy(g[:P]).to(DEV)[None].contiguous()
    gf_d = None if gf is None else torch.from_numpy(gf[:P]).to(DEV)[None].contiguous()
    src_flip = mode == MODES[1]
    got_d = _k10r_device(N, g_d, gf_d, src, src_flip)
    assert tuple(got_d.shape) == (1, P, h, w)
    got = got_d[0].cpu().numpy()
    n_diff = int((got != out32[:P]).sum())
    err = np.abs(got.astype(np.float64) - out64[:P])
    bound = (nterm + 1)[None] * U * abs64[:P]
    unref = nterm == 0
    print(f"K10r' {src}->{dst} {mode} planes={P}: {n_diff} elements differ from the CPU fp32 restatement, max |err vs fp64| "
          f"{err.max():.3e} (max bound {bound.max():.3e}), terms per element {nterm.min()}..{nterm.max()}, "
          f"{int(unref.sum())} unreferenced source elements")
    assert n_diff == 0
    assert bool((err <= bound).all())
    assert bool((got[:, unref] == 0).all())
    # <R x, g> == <x, R^T g> with K10a's own output as R x
    x = torch.rand(1, P, h, w, generator=torch.Generator().manual_seed(P + h + W)).to(DEV)
    y, yf = N.msf_resize_input(x.flip(3).contiguous() if src_flip else x, dst, flip=gf is not None)
    lhs = float((y.double() * g_d.double()).sum())
    if gf is not None:
        lhs += float((yf.double() * gf_d.double()).sum())
    rhs = float((x.double() * got_d.double()).sum())
    slack = float((torch.from_numpy(bound)[None].to(DEV) * x.double().abs()).sum())
    print(f"    <R x, g> {lhs:.9e}   <x, R^T g> {rhs:.9e}   |difference| {abs(lhs - rhs):.2e}   bound {slack:.2e}")
    assert abs(lhs - rhs) <= slack
    assert torch.equal(_k10r_device(N, g_d, gf_d, src, src_flip), got_d)          # no atomics: bitwise reproducible


# ---------------------------------------------------------------------------------------------------------------- 2: one pass
def _pass_aten(logits, d, scaled, label, flip, dtype):
    """the gradient of sum(d * softmax(resize_ac(flip?(up(logits))))) with respect to the logits, CPU autograd in ``dtype``"""
    lg = logits.to(dtype).requires_grad_(True)
    up = lg if tuple(lg.shape[2:]) == tuple(scaled) else F.interpolate(lg, size=scaled, mode="bilinear", align_corners=False)
    if flip:
        up = up.flip(3)
    p = F.interpolate(up, size=label, mode="bilinear", align_corners=True).softmax(1)
    (g,) = torch.autograd.grad(p, [lg], d.to(dtype))
    return g


@pytest.mark.parametrize("C", [5, 21, 151, 192])
@pytest.mark.parametrize("r", [1, 4, 16])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("scaled", [(32, 64), (64, 96), (128, 192)])
@pytest.mark.parametrize("label", [(64, 96), (40, 56)])
def test_pass_backward_vs_fp64(N, C, r, flip, scaled, label):
    """K10g + K10r' (+ M2 backward for low-res logits).  Device max |err| <= 2 x the max |err| of fp32 ATen on the CPU (both
    against float64 CPU autograd), floor 4 ulp of the largest gradient: HIP's expf and the LDS reduction order differ from
    ATen's."""
    gen = torch.Generator().manual_seed(C * 11 + r + scaled[0] + label[1] + int(flip))
    logits = torch.randn(B, C, scaled[0] // r, scaled[1] // r, generator=gen) * 3
    d = torch.rand(B, C, *label, generator=gen) * 2 - 1
    want = _pass_aten(logits, d, scaled, label, flip, torch.float64)
    err_aten = (_pass_aten(logits, d, scaled, label, flip, torch.float32).double() - want).abs().max().item()
    lg_d, d_d = logits.to(DEV), d.to(DEV)
    ws = torch.empty(B, C, *label, device=DEV)
    got = N.msf_accumulate_backward(lg_d, d_d, scaled, flip=flip, workspace=ws)
    assert tuple(got.shape) == tuple(logits.shape)
    err = (got.cpu().double() - want).abs().max().item()
    floor = _ulp4(want)
    print(f"pass backward C={C} x{r} flip={flip} {scaled}->{label}: max |err vs fp64| device {err:.3e}, fp32 ATen (CPU) "
          f"{err_aten:.3e}, max |want| {want.abs().max().item():.3e}, floor {floor:.3e}")
    assert err <= max(2 * err_aten, floor)
    assert torch.equal(N.msf_accumulate_backward(lg_d, d_d, scaled, flip=flip), got)      # own workspace, same bits


def test_pass_backward_refuses_193_classes(N):
    with pytest.raises(N.SeaNativeError):
        N.msf_accumulate_backward(torch.zeros(1, 193, 32, 32, device=DEV), torch.zeros(1, 193, 40, 56, device=DEV), (32, 32))
    z = torch.zeros(1, 193, 32, 32, device=DEV)
    d = torch.zeros(1, 193, 40, 56, device=DEV)
    rc = N.lib().sea_msf_accumulate_bwd(z.data_ptr(), d.data_ptr(), torch.empty_like(d).data_ptr(),
                                        torch.empty_like(z).data_ptr(), 1, 193, 32, 32, 32, 32, 40, 56, 0, None)
    assert rc == 1


# ---------------------------------------------------------------------------------------------------------------- 3: wrapper
SIX = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)


def _nets(name, C):
    from oracle.tiny_models import PointwiseNet, TinyConvNet
    return (TinyConvNet if name == "conv" else PointwiseNet)(C, seed=C + 3)


def _aten_msf(net, x, scales, flip):
    """the protocol of evaluate_msf in ATen operations under autograd, then z = log(max(score, FLT_MIN))"""
    from semseg.val import msf_scaled_size
    H, W = x.shape[2:]
    score = 0
    for s in scales:
        xs = F.interpolate(x, size=msf_scaled_size(s, H, W), mode="bilinear", align_corners=True)
        score = score + F.interpolate(net(xs), size=(H, W), mode="bilinear", align_corners=True).softmax(1)
        if flip:
            score = score + F.interpolate(net(xs.flip(3)).flip(3), size=(H, W), mode="bilinear",
                                          align_corners=True).softmax(1)
    return torch.log(score.clamp_min(FLT_MIN))


def _aten_grad(cpu_net, x, r, scales, flip, dtype):
    xi = x.to(dtype).requires_grad_(True)
    (g,) = torch.autograd.grad(_aten_msf(copy.deepcopy(cpu_net).to(dtype), xi, scales, flip), [xi], r.to(dtype))
    return g


class _Recorder:
    """patches semseg.val.Metrics with a subclass that keeps every score tensor handed to update()"""

    def __init__(self, monkeypatch):
        import semseg.val as V
        self.scores = []
        rec = self

        class RecMetrics(V.Metrics):
            def update(self, pred, target):
                rec.scores.append(pred.detach().clone())
                super().update(pred, target)

        monkeypatch.setattr(V, "Metrics", RecMetrics)


@pytest.mark.parametrize("net_name", ["conv", "pw"])
@pytest.mark.parametrize("C", [5, 21])
@pytest.mark.parametrize("scales,flip", [((0.5, 1.0, 1.75), True), (SIX, False)])
@pytest.mark.parametrize("shape", [(64, 96), (40, 56)])
def test_wrapper_score_and_gradient(N, net_name, C, scales, flip, shape, monkeypatch):
    import semseg.val as V
    cpu_net = _nets(net_name, C)
    net = copy.deepcopy(cpu_net).to(DEV)
    gen = torch.Generator().manual_seed(C + shape[1] + len(scales))
    x = torch.rand(B, 3, *shape, generator=gen)
    r = torch.rand(B, C, *shape, generator=gen) * 2 - 1
    y = torch.randint(0, C, (B, *shape), generator=gen)
    wrap = MsfModel(net, scales, flip)
    # the buffer of evaluate_msf's loop, bit for bit
    rec = _Recorder(monkeypatch)
    V._evaluate_msf_metrics(net, [(x.to(DEV), y.to(DEV))], DEV, scales, flip, n_classes=C, ignore_label=-1)
    score = wrap.score(x.to(DEV))
    assert tuple(score.shape) == (B, C, *shape) and not score.requires_grad
    assert torch.equal(score, rec.scores[0])
    score = score.clone()
    with torch.no_grad():
        z = wrap(x.to(DEV))
    ref = torch.log(score.clamp_min(FLT_MIN))
    ulps = ((z - ref).abs().cpu().numpy() / np.spacing(np.abs(ref.cpu().numpy()))).max()
    assert ulps <= 2
    # the input gradient of sum(z * r)
    want = _aten_grad(cpu_net, x, r, scales, flip, torch.float64)
    err_aten = (_aten_grad(cpu_net, x, r, scales, flip, torch.float32).double() - want).abs().max().item()
    xd = x.to(DEV).requires_grad_(True)
    out = wrap(xd)
    (got,) = torch.autograd.grad(out, [xd], r.to(DEV))
    err = (got.cpu().double() - want).abs().max().item()
    floor = _ulp4(want)
    print(f"wrapper {net_name} C={C} scales {scales} flip={flip} {shape}: z within {ulps:.1f} ulp of log(score); input gradient "
          f"max |err vs fp64| device {err:.3e}, fp32 ATen (CPU) {err_aten:.3e}, max |want| {want.abs().max().item():.3e}")
    assert tuple(out.shape) == (B, C, *shape)
    assert err <= max(2 * err_aten, floor)
    out2 = wrap(xd)
    (again,) = torch.autograd.grad(out2, [xd], r.to(DEV))
    assert torch.equal(again, got)                        # bitwise reproducible


def test_wrapper_buffers_keep_their_addresses(N):
    net = _nets("pw", 5).to(DEV)
    wrap = MsfModel(net, (0.5, 1.0), True)
    x = torch.rand(B, 3, 64, 96, device=DEV)
    p0 = wrap.score(x).data_ptr()
    wrap.score(torch.rand(1, 3, 64, 96, device=DEV))      # a ragged last batch in between
    with torch.no_grad():
        wrap(x)
    assert wrap.score(x).data_ptr() == p0
    assert list(wrap.buffers()) == list(net.buffers())    # the wrapper's own buffers are not module state
    assert not hasattr(wrap, "forward_lowres")
    with pytest.raises(ValueError):
        wrap(torch.rand(3, 64, 96, device=DEV))
    with pytest.raises(ValueError):
        MsfModel(_nets("pw", 193).to(DEV), (1.0,), False)(torch.rand(1, 3, 32, 32, device=DEV))


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
    """PointwiseNet on the r x r average-pooled image, up-sampled by r: a miniature of the models with a ``forward_lowres``
    hook (a tuple whose first entry is the logits before the final up-sampling)"""

    def __init__(self, C, r):
        super().__init__()
        from oracle.tiny_models import PointwiseNet
        self.net, self.r = PointwiseNet(C, seed=C + r), r
        self.eval()

    def forward_lowres(self, x):
        return (self.net(F.avg_pool2d(x, self.r)),)

    def forward(self, x):
        low = self.forward_lowres(x)[0]
        size = tuple(x.shape[2:])
        return _UpM2.apply(low, size) if x.is_cuda else F.interpolate(low, size=size, mode="bilinear", align_corners=False)


class _Hidden(torch.nn.Module):
    """the same model without its hook"""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.eval()

    def forward(self, x):
        return self.inner(x)


@pytest.mark.parametrize("C", [21, 151])
@pytest.mark.parametrize("r", [4, 16])
@pytest.mark.parametrize("shape", [(64, 96), (40, 56)])
def test_wrapper_lowres_hook_vs_hidden_hook(N, C, r, shape, monkeypatch):
    """a model with the hook: K10b and its adjoint run in low-res mode; the same gradient as through the model's own
    up-sampling and full-res mode, both measured against the float64 protocol"""
    from semseg import _native
    scales, flip = (0.5, 1.0, 1.75), True
    cpu_net = _LowresNet(C, r)
    net = copy.deepcopy(cpu_net).to(DEV)
    gen = torch.Generator().manual_seed(C + r + shape[1])
    x = torch.rand(B, 3, *shape, generator=gen)
    rr = torch.rand(B, C, *shape, generator=gen) * 2 - 1
    want = _aten_grad(cpu_net, x, rr, scales, flip, torch.float64)
    seen = []
    real = _native.msf_accumulate_backward

    def spy(logits, dscore, scaled_size, flip=False, workspace=None):
        seen.append(tuple(logits.shape[2:]) != tuple(scaled_size))
        return real(logits, dscore, scaled_size, flip=flip, workspace=workspace)

    monkeypatch.setattr(_native, "msf_accumulate_backward", spy)
    grads, outs = [], []
    for model in (net, _Hidden(net)):
        xd = x.to(DEV).requires_grad_(True)
        out = MsfModel(model, scales, flip)(xd)
        grads.append(torch.autograd.grad(out, [xd], rr.to(DEV))[0])
        outs.append(out.detach())
    assert seen == [True] * 6 + [False] * 6, seen
    err_hook, err_hidden = ((g.cpu().double() - want).abs().max().item() for g in grads)
    floor = _ulp4(want)
    print(f"low-res hook C={C} x{r} {shape}: max |z - z(hidden hook)| {(outs[0] - outs[1]).abs().max().item():.2e}; input gradient "
          f"max |err vs fp64| with the hook {err_hook:.3e}, hook hidden {err_hidden:.3e}, max |want| "
          f"{want.abs().max().item():.3e}")
    assert err_hook <= max(2 * err_hidden, floor)


# ---------------------------------------------------------------------------------------------------------------- 4: attacks
EPS = 8.0 / 255
C_ATT = 5


@pytest.fixture(scope="module")
def attack_case(N):
    net = _nets("conv", C_ATT).to(DEV)
    wrap = MsfModel(net, (0.5, 1.0, 1.75), True)
    gen = torch.Generator().manual_seed(53)
    x = torch.rand(B, 3, 64, 96, generator=gen).to(DEV)
    w = torch.rand(C_ATT, generator=gen).to(DEV)
    y = wrap.score(x).max(1)[1].cpu()
    y = torch.where(torch.rand(y.shape, generator=gen) < 0.1, torch.randint(0, C_ATT, y.shape, generator=gen), y)
    y = torch.where(torch.rand(y.shape, generator=gen) < 0.05, torch.full_like(y, -1), y)
    return wrap, x, y.to(DEV), w


def _run(A, wrap, x, y, w, loss):
    return A.apgd_train(wrap, x, y, "Linf", EPS, n_iter=12, loss=loss, num_classes=C_ATT, weights=w, return_pred=True)


@pytest.mark.parametrize("loss", ["mask-ce-avg", "js-avg"])
def test_attack_through_the_ensemble(N, attack_case, loss, monkeypatch, capfd):
    from semseg import attacker as A
    wrap, x, y, w = attack_case
    captures = []
    real = A.ApgdRun._capture

    def counting(self, i):
        res = real(self, i)
        captures.append(self.own.graphs is not None)
        return res

    monkeypatch.setattr(A.ApgdRun, "_capture", counting)
    outs = []
    for graph in (False, True, True):
        monkeypatch.setattr(A, "USE_HIP_GRAPH", graph)
        if len(outs) < 2:
            A.release_graph_cache(wrap)
        outs.append(_run(A, wrap, x, y, w, loss))
        if not graph:
            assert captures == []
    # the loss at the start point: what step 0 records before any update
    monkeypatch.setattr(A, "USE_HIP_GRAPH", False)
    run = A.ApgdRun(wrap, x, y, EPS, 12, loss, None, False, C_ATT, w, x.clone())
    run.start()
    loss_start = run.st.loss_best.clone()
    run.release_graphs()
    A.release_graph_cache(wrap)
    assert captures == [True], captures                   # the second run captured its pair, the third replayed it
    assert "continuing with the eager loop" not in capfd.readouterr().err
    eager, graph, again = outs
    assert len(eager) == 5
    for a, b, c in zip(eager, graph, again):
        assert torch.equal(a, b)                          # HIP-graph replay is bitwise the eager loop
        assert torch.equal(b, c)                          # two runs are bitwise equal
    x_best, acc, loss_best, x_best_adv, pred = graph
    for xa in (x_best, x_best_adv):
        assert (xa - x).abs().max().item() <= EPS * (1 + 1e-6)
        assert xa.min().item() >= 0.0 and xa.max().item() <= 1.0
    assert bool((loss_best >= loss_start).all()), (loss_best.tolist(), loss_start.tolist())
    valid = y != -1
    acc_of = lambda xs: (((wrap.score(xs).max(1)[1] == y) & valid).flatten(1).sum(1).float() / valid.flatten(1).sum(1)).cpu()
    clean, adv = acc_of(x), acc_of(x_best_adv)
    print(f"{loss}: loss at the start {loss_start.tolist()}, best {loss_best.tolist()}; ensemble accuracy clean {clean.tolist()}, "
          f"at x_best_adv {adv.tolist()}")
    assert bool((adv <= clean).all())
    assert torch.equal(wrap.score(x_best_adv).max(1)[1].to(pred.dtype), pred)     # the attack's own argmax is the ensemble's


def test_infer_tool_through_the_ensemble(N, tmp_path):
    from tools import infer
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "pascalvoc_convnext.yaml")))
    cfg["SAVE_DIR"] = str(tmp_path) + "/"
    cfg_path = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(cfg_path, "w"))
    args = ["--cfg", cfg_path, "--eps", "8", "--n_iter", "12", "--synthetic", "4", "--image_size", "128", "--batch_size", "2",
            "--msf-scales", "0.5,1.0", "--msf-flip", "--cleanup", "0", "--save_argmax", "--deterministic",
            "--json", str(tmp_path / "a.json")]
    s = infer.main(args)
    name = "UperNet_ConvNeXt-T_CVST"
    assert os.path.exists(tmp_path / "a.json")
    assert os.path.exists(os.path.join(str(tmp_path), f"worse_SEA_{name}_{cfg['EVAL']['NAME']}_8.0.pt"))
    for l in infer.LOSSES:
        lg = torch.load(os.path.join(str(tmp_path), "argmax-logs", f"{name}_{l}_8.0.pt"))
        assert lg.shape == (4, 128, 128) and lg.dtype == torch.int64
    assert s["n_images"] == 4 and 0.0 <= s["worst_Acc"] <= min(s["worst_Acc_indiv"]) + 1e-9
    for bad in (["--msf-flip"], ["--msf-scales", "0.5,1.0", "--window", "64"], ["--msf-scales", "0.5,-1"]):
        with pytest.raises(SystemExit):
            infer.main(["--cfg", cfg_path, "--synthetic", "4"] + bad)
