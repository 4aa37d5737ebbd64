"""T2u-ac on the device (`-m gpu`): ``CrossEntropy`` / ``OhemCrossEntropy`` ``.upsampled(..., align_corners=True)`` with
``native=True`` on low-resolution logits, against float64 and against the unfused device path, at every shape of
tests/test_train_loss_up_ac_cpu.py; selection, footprint, reproducibility, graph capture, edge semantics, the fallback, and
PSPNet's training forward behind ``pspnet.TRAIN_CRITERION`` / the tool's flags.

Accuracy rule: tests/test_train_loss_up_gpu.py's, as it stands (``ulp32``, ``run``, ``errors`` and ``module_factory`` are
imported from there).  The yardstick is float64 on CPU (``F.interpolate(..., align_corners=True)`` of the double tensor,
then the plain module in double).  The comparator is the unfused path on the device: ``N.upsample_ac`` (P2) + the module
with ``native=False``, fp32, same tensors.  The fused path's loss error is at most max(2 x the comparator's, the loss floor),
its gradient error (with respect to the LOW-resolution tensor, max-abs over elements) at most max(2 x the comparator's, one
fp32 ulp of the largest gradient element).  Every pair is printed before it is asserted."""
import json
import math
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
import yaml

from conftest import PKG
from test_train_loss_up_ac_cpu import SHAPES, assert_selection_unambiguous, exact_weights, interp, shape_of
from test_train_loss_up_cpu import AUX_SEED, B, make, recipe
from test_train_loss_up_gpu import CASES, errors, module_factory, run, ulp32

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = list(SHAPES)


def up_device(p, y):
    from semseg.models.pspnet import _UpsampleAC      # N.upsample_ac with its gradient, N.upsample_ac_backward
    return _UpsampleAC.apply(p, tuple(y.shape[-2:]))


def three_results(mk, preds, y):
    """(float64 yardstick, unfused device path, fused device path) of the module mk(native, device, double)"""
    m64 = mk(False, None, True)
    want = run(lambda p, t: m64(tuple(interp(q, t) for q in p) if isinstance(p, tuple) else interp(p, t), t),
               [p.double() for p in preds], y)
    ms = mk(False, DEV, False)
    stock = run(lambda p, t: ms(tuple(up_device(q, t) for q in p) if isinstance(p, tuple) else up_device(p, t), t),
                [p.to(DEV) for p in preds], y.to(DEV))
    mf = mk(True, DEV, False)
    fused = run(lambda p, t: mf.upsampled(p, t, align_corners=True), [p.to(DEV) for p in preds], y.to(DEV))
    return want, stock, fused, mf


def loss_floor(mk, preds, y, aux_weights, total):
    """tests/test_train_loss_up_gpu.py: loss_floor, on the align_corners=True interpolation"""
    if len(preds) == 1:
        return 0.5 * ulp32(total)
    bound = 0.5 * ulp32(total) * (len(preds) - 1)
    m64 = mk(False, None, True)
    for p, a in zip(preds, aux_weights):
        lk = float(m64(interp(p.double(), y), y))
        bound += a * 0.5 * ulp32(lk) + (0.5 * ulp32(a * lk) if a != 1.0 else 0.0)
    return bound


def assert_rule(tag, e_f, e_s, floors):
    print(f"[T2u-ac {tag}] loss err fused {e_f[0]:.3e} unfused {e_s[0]:.3e} | grad err fused {e_f[1]:.3e} unfused "
          f"{e_s[1]:.3e} | floors {floors[0]:.2e} {floors[1]:.2e}")
    assert e_f[0] <= max(2 * e_s[0], floors[0]), (e_f, e_s, floors)
    assert e_f[1] <= max(2 * e_s[1], floors[1]), (e_f, e_s, floors)


def check_accuracy(mk, preds, y, tag, aux_weights=(1.0,)):
    want, stock, fused, mf = three_results(mk, preds, y)
    gmax = max(float(g.abs().max()) for g in want[1])
    floors = (loss_floor(mk, preds, y, aux_weights, float(want[0])), ulp32(gmax))
    assert_rule(tag, errors(fused, want), errors(stock, want), floors)
    return want, fused, mf


def assert_same_footprint(g, g0, shape):
    """The gradient is non-zero at exactly the low-resolution elements the yardstick's selected pixels touch.  Where the scale
    (n_in - 1) / (n_out - 1) is a power of two (or 0) the source coordinates and weights are exact in fp32 and in float64
    alike, and the two sets are compared as they are.  Elsewhere tests/test_train_loss_up_gpu.py's rule: elements whose
    gradient is below 2^-20 of the largest one in BOTH results may be zero in one of them."""
    if exact_weights(shape):
        assert torch.equal(g != 0, g0 != 0)
        return
    tol = 2.0 ** -20 * float(g0.abs().max())
    differ = (g != 0) != (g0 != 0)
    assert bool(((g.abs() <= tol) & (g0.abs() <= tol))[differ].all()), int(differ.sum())


@pytest.mark.parametrize("ignore", [255, -1])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", NAMES)
def test_accuracy_selection_and_footprint(name, case, ignore):
    from semseg import _native as N
    kind, weighted, thresh, tup = CASES[case]
    shape = shape_of(name)
    assert N.train_ce_up_tile(*shape, align_corners=True) > 0          # (the fused kernels run, not the fallback)
    low, y, weights = recipe(shape, ignore)
    preds = [low, recipe(shape, ignore, seed=AUX_SEED)[0]] if tup else [low]
    mk = module_factory(kind, ignore, weights if weighted else None, thresh)
    aux = tuple(float(a) for a in mk(False, None, False).aux_weights[:len(preds)])
    sel = None
    if kind == "ohem":   # the selection must be unambiguous in the yardstick alone, before anything is compared
        sel = [assert_selection_unambiguous(p, y, ignore, thresh) for p in preds]
    want, fused, mf = check_accuracy(mk, preds, y, f"{name} {case} ignore {ignore}", aux)
    for g, g0 in zip(fused[1], want[1]):
        assert_same_footprint(g, g0, shape)
    if kind == "ohem":   # the device words of the LAST prediction of the call
        n_min, n_sel, mode = sel[-1]
        w = N.train_words_dict(mf.last_words)
        assert (w["n_min"], w["n_sel"], w["mode"], w["err"]) == (n_min, n_sel, mode, 0), (w, sel[-1])
        if case == "ohem_topk":
            assert mode == 1


def test_ratio_one_agrees_with_t2():
    """h x w -> h x w: the interpolation is the identity, T2u-ac solves T2's problem.  Both under the accuracy rule against
    the same float64 result; here T2's error is the comparator."""
    shape = shape_of("ratio1_C21")
    low, y, weights = recipe(shape)
    for kind in ("ce", "ohem"):
        wts = weights if kind == "ce" else None
        if kind == "ohem":
            assert_selection_unambiguous(low, y, 255, 0.7)
        want = run(make(kind, 255, wts).double(), [low.double()], y)
        wd = None if wts is None else wts.to(DEV)
        t2 = run(make(kind, 255, wd, native=True), [low.to(DEV)], y.to(DEV))
        mod = make(kind, 255, wd, native=True)
        t2u = run(lambda p, t: mod.upsampled(p, t, align_corners=True), [low.to(DEV)], y.to(DEV))
        floors = (0.5 * ulp32(float(want[0])), ulp32(float(want[1][0].abs().max())))
        assert_rule(f"ratio 1 {kind} (comparator: T2)", errors(t2u, want), errors(t2, want), floors)


@pytest.mark.parametrize("ohem", [False, True], ids=["ce", "ohem"])
@pytest.mark.parametrize("name", ["halo_C21", "x8_C151", "frac_C21"])
def test_two_runs_give_the_same_bits(name, ohem):
    from semseg import _native as N
    low, y, weights = recipe(shape_of(name))
    low, y, weights = low.to(DEV), y.to(DEV), weights.to(DEV)
    g = torch.full((), 0.75, device=DEV)
    outs = []
    for _ in range(2):
        loss, loss_px, words = N.train_ce_up_forward(low, y.shape[-2:], y, weights, 255, 0.3566749, ohem,
                                                     align_corners=True)
        dlow = N.train_ce_up_backward(low, y.shape[-2:], y, weights, 255, ohem, loss_px, words, g, align_corners=True)
        outs.append((loss, loss_px, dlow))
    assert torch.isfinite(outs[0][0]) and bool((outs[0][2] != 0).any())
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # ... and they are not the align_corners=False bits
    other = N.train_ce_up_forward(low, y.shape[-2:], y, weights, 255, 0.3566749, ohem)[0]
    assert not torch.equal(other, outs[0][0])


def test_forward_backward_in_a_captured_graph():
    """No host synchronisation: forward, select and backward are captured and replayed on new logits written into the same
    buffer (tests/test_train_loss_up_gpu.py's capture test at PSPNet's x8 relation, 17 -> 129; top-k regime)."""
    from semseg import _native as N
    C, h, S = 21, 17, 129
    gen = torch.Generator(device=DEV).manual_seed(5)
    z0 = torch.randn(B, C, h, h, generator=gen, device=DEV) * 2
    z1 = (z0 + 0.25 * torch.randn(z0.shape, device=DEV, generator=gen)).contiguous()
    y = torch.randint(0, C, (B, S, S), generator=gen, device=DEV)
    y[torch.rand(B, S, S, generator=gen, device=DEV) < 0.05] = -1
    mod = make("ohem", -1, native=True, thresh=1e-9).to(DEV)
    static = z0.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(mod.upsampled(static, y, align_corners=True), static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_c = mod.upsampled(static, y, align_corners=True)
        grad_c, = torch.autograd.grad(loss_c, static)
        words_c = mod.last_words
    with torch.no_grad():
        static.copy_(z1)
    graph.replay()
    torch.cuda.synchronize()
    w = N.train_words_dict(words_c)
    assert w["mode"] == 1 and w["n_sel"] == w["n_min"] > 0, w
    leaf = z1.clone().requires_grad_(True)
    loss_e = mod.upsampled(leaf, y, align_corners=True)
    grad_e, = torch.autograd.grad(loss_e, leaf)
    assert torch.isfinite(loss_e) and torch.equal(loss_c, loss_e.detach()) and torch.equal(grad_c, grad_e)
    leaf0 = z0.clone().requires_grad_(True)
    assert not torch.equal(mod.upsampled(leaf0, y, align_corners=True).detach(), loss_e.detach())   # the replay saw z1


@pytest.mark.parametrize("kind", ["ce", "ohem"])
def test_batch_with_every_label_ignored(kind):
    """as tests/test_train_loss_up_gpu.py asserts for align_corners=False: NaN loss, gradient all zeros (no NaN in it)"""
    low, y, _ = recipe(shape_of("x8_C21"), ignore=-1)
    y[:] = -1
    mod = make(kind, -1, native=True)
    leaf = low.to(DEV).requires_grad_(True)
    loss = mod.upsampled(leaf, y.to(DEV), align_corners=True)
    loss.backward()
    assert torch.isnan(loss) and bool((leaf.grad == 0).all())


@pytest.mark.parametrize("kind", ["ce", "ohem"])
def test_class_count_without_a_plan_takes_p2_plus_t2(kind):
    """C = 193 is above the ceiling: ``upsampled`` is P2 + T2, bit for bit, and meets the accuracy rule"""
    from semseg import _native as N
    shape = (193, 5, 8, 33, 57)
    low, y, _ = recipe(shape)
    assert not N.train_ce_up_supported(low, y.shape[-2:], align_corners=True)
    if kind == "ohem":
        assert_selection_unambiguous(low, y, 255, 0.7)
    mk = module_factory(kind, 255, None, 0.7)
    want, fused, mf = check_accuracy(mk, [low], y, f"C = 193 {kind} (P2 + T2)")
    b = run(lambda p, t: mf(up_device(p, t), t), [low.to(DEV)], y.to(DEV))
    assert torch.isfinite(fused[0]) and torch.equal(fused[0], b[0]) and torch.equal(fused[1][0], b[1][0])
    with pytest.raises(N.SeaNativeError):
        N.train_ce_up_forward(low.to(DEV), y.shape[-2:], y.to(DEV), None, 255, align_corners=True)


def test_pow2_kernel_choice_takes_the_gather_with_align_corners():
    """H = 4 h: ``up_kernel="pow2"`` has a single-pass kernel for align_corners=False; with align_corners=True it must not run"""
    from semseg.losses import CrossEntropy
    low, y, _ = recipe((21, 5, 7, 20, 28))
    low, y = low.to(DEV), y.to(DEV)
    a = CrossEntropy(255, native=True, up_kernel="pow2").upsampled(low, y, align_corners=True)
    b = CrossEntropy(255, native=True).upsampled(low, y, align_corners=True)
    c = CrossEntropy(255, native=True, up_kernel="pow2").upsampled(low, y)
    assert torch.isfinite(a) and torch.equal(a, b) and not torch.equal(a, c)


# ------------------------------------------------------------------------------------------------------------ PSPNet
class _Mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from semseg.models import pspnet
        self.old, pspnet.TRAIN_CRITERION = pspnet.TRAIN_CRITERION, self.mode

    def __exit__(self, *a):
        from semseg.models import pspnet
        pspnet.TRAIN_CRITERION = self.old


def _hooked_step(model, x, y, mode):
    """one training forward + backward in ``mode``; returns the losses, the third element, the two heads' low-resolution
    logits with their gradients, and the input shapes of the P2 up-samplings of logits the forward made"""
    kept = {}

    def keep(key):
        def hook(module, args, out):
            out.retain_grad()
            kept[key] = out
        return hook

    from semseg.models import pspnet
    ups, real_up = [], pspnet._up_ac_train

    def counting_up(t, size):                 # every P2 up-sampling of logits in the training forward goes through here
        ups.append(tuple(t.shape))
        return real_up(t, size)

    hooks = [model.cls[4].register_forward_hook(keep("main")), model.aux[4].register_forward_hook(keep("aux"))]
    pspnet._up_ac_train = counting_up
    try:
        model.zero_grad(set_to_none=True)
        with _Mode(mode):
            main, aux, third = model(x, y)
        (main + 0.4 * aux).backward()
    finally:
        pspnet._up_ac_train = real_up
        for hk in hooks:
            hk.remove()
    lows = {k: (v.detach().clone(), v.grad.detach().clone()) for k, v in kept.items()}
    return main.detach(), aux.detach(), third, lows, ups


def _distance(model, ref):
    """relative L2 distance of the whole parameter gradient of ``model`` from that of ``ref``"""
    pd = dict(model.named_parameters())
    num = sum((pd[k].grad.double() - p.grad.double()).norm() ** 2 for k, p in ref.named_parameters())
    den = sum(p.grad.double().norm() ** 2 for k, p in ref.named_parameters())
    return float((num / den).sqrt())


def _head_errors(res, key, y, weight=None, ignore=-1):
    """(loss error, gradient error) of one head of one ``_hooked_step`` result against float64 computed on the CPU from the
    low-resolution logits that very step hooked, and the rule's floors"""
    scale = 1.0 if key == "main" else 0.4
    low = res[3][key][0].double().cpu().requires_grad_(True)
    l64 = F.cross_entropy(interp(low, y), y, None if weight is None else weight.double().cpu(), ignore_index=ignore)
    (scale * l64).backward()
    want = (l64.detach(), [low.grad])
    got = (res[0 if key == "main" else 1].double().cpu(), [res[3][key][1].double().cpu()])
    return errors(got, want), (0.5 * ulp32(float(want[0])), ulp32(float(low.grad.abs().max())))


class _Repeatable:
    """The library convolutions restricted to their deterministic solvers, so that two forwards from the same weights give
    the same bits.  (Immediate mode alone, which tests/test_psp_gpu.py uses, is repeatable in a fresh process but not after
    find-mode runs of the same shapes earlier in the process, as tests/test_psp_train_gpu.py makes them: measured.)"""

    def __enter__(self):
        self.old = (torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic)
        torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True

    def __exit__(self, *a):
        torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = self.old


def test_pspnet_training_forward_in_the_three_modes():
    from test_psp_train_gpu import _batch, _model, _train_step
    x, y = _batch()
    size = tuple(y.shape[-2:])
    models = {m: _model() for m in ("torch", "native", "fused")}
    with _Repeatable():
        res = {m: _hooked_step(models[m], x, y, m) for m in models}
    # the forward before the criterion is the same deterministic code
    for m in ("native", "fused"):
        for k in ("main", "aux"):
            assert torch.equal(res[m][3][k][0], res["torch"][3][k][0]), (m, k)
    assert res["fused"][2] is None
    for m in ("torch", "native"):
        assert torch.is_tensor(res[m][2]) and tuple(res[m][2].shape) == (2, 21) + size
    # mode fused up-samples nothing (no full-resolution logits, and not the P2 + T2 fallback); the other two modes up-sample
    # each head once, from its low resolution
    low_shape = tuple(res["torch"][3]["main"][0].shape)
    assert low_shape == (2, 21, 17, 17)
    assert res["fused"][4] == [] and res["torch"][4] == [low_shape] * 2 and res["native"][4] == [low_shape] * 2
    # losses and head gradients against float64 computed on the CPU from the hooked logits; comparator: mode torch
    yc = y.cpu()
    for k in ("main", "aux"):
        e_t, _ = _head_errors(res["torch"], k, yc)
        for m in ("native", "fused"):
            e_m, floors = _head_errors(res[m], k, yc)
            assert_rule(f"PSPNet {k} head, mode {m} (unfused: mode torch)", e_m, e_t, floors)
    # the whole parameter gradient: a new mode is no farther from the old one than the old one is from the truth
    ref = _model().double()
    _train_step(ref, x.double(), y, False)
    d_truth = _distance(models["torch"], ref)
    d_native, d_fused = _distance(models["native"], models["torch"]), _distance(models["fused"], models["torch"])
    print(f"[T2u-ac PSPNet] parameter gradient, relative L2: torch vs float64 {d_truth:.3e} | native vs torch {d_native:.3e} "
          f"| fused vs torch {d_fused:.3e}")
    assert d_native <= d_truth and d_fused <= d_truth, (d_native, d_fused, d_truth)
    for m in ("native", "fused"):
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in models[m].parameters())
        bufs = dict(models[m].named_buffers())
        for name, b in models["torch"].named_buffers():
            assert torch.equal(bufs[name], b), (m, name)


def test_pspnet_other_criteria_keep_the_torch_line():
    from test_psp_train_gpu import _batch, _model
    x, y = _batch()
    model = _model()
    outs = {}
    for crit in (nn.CrossEntropyLoss(ignore_index=-1, label_smoothing=0.1),
                 nn.CrossEntropyLoss(ignore_index=-1, reduction="sum")):
        model.criterion = crit
        for m in ("torch", "native", "fused"):
            with _Mode(m), _Repeatable(), torch.no_grad():
                outs[m] = model(x, y)
        for m in ("native", "fused"):
            assert torch.is_tensor(outs[m][2])
            for a, b in zip(outs[m], outs["torch"]):
                assert torch.isfinite(a).all() and torch.equal(a, b), (m, crit)


def test_pspnet_criterion_weight_and_ignore_index_are_honoured():
    """class weights and ignore_index 255 on the model's criterion: each mode against float64 from the logits it hooked"""
    from test_psp_train_gpu import _batch, _model
    x, y = _batch()
    y = torch.where(y < 0, torch.full_like(y, 255), y)
    wts = (torch.rand(21, generator=torch.Generator().manual_seed(7)) + 0.5)
    model = _model()
    model.criterion = nn.CrossEntropyLoss(weight=wts.cuda(), ignore_index=255)
    with _Repeatable():
        res = {m: _hooked_step(model, x, y, m) for m in ("torch", "native", "fused")}
    yc = y.cpu()
    for k in ("main", "aux"):
        e_t, _ = _head_errors(res["torch"], k, yc, wts, 255)
        for m in ("native", "fused"):
            e_m, floors = _head_errors(res[m], k, yc, wts, 255)
            assert_rule(f"PSPNet weighted {k} head, mode {m} (unfused: mode torch)", e_m, e_t, floors)


@pytest.mark.parametrize("flag,mode", [("--native-criterion", "native"), ("--fused-criterion", "fused")])
def test_train_rob_seg_pspnet_flags(tmp_path, flag, mode):
    from semseg.models import PSPNet, pspnet
    from tools import train_rob_seg as T
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "pascalvoc_pspnet.yaml")))
    cfg["TRAIN"]["IMAGE_SIZE"] = [129, 129]
    cfg["TRAIN"]["N_ITERS"] = 2
    cfg_path = tmp_path / "psp.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    out, dump = tmp_path / "out.json", tmp_path / "params.pt"
    rec = T.main(["--cfg", str(cfg_path), "--synthetic", "2", "--steps", "2", "--warmup", "0", "--batch_size", "2",
                  "--deterministic", "--json", str(out), "--dump_params", str(dump), flag, "--fused-kernel", "pow2"])
    res = json.load(open(out))
    assert res == rec and res["psp_criterion"] == mode and res["model"] == "PSPNet-RN50"
    assert math.isfinite(res["last_loss"])
    assert pspnet.TRAIN_CRITERION == "torch"
    torch.manual_seed(0)
    init = PSPNet(50, 21).state_dict()
    params = torch.load(dump)["params"]
    changed = [not torch.equal(init[k], v) for k, v in params.items()]
    assert len(changed) >= 20 and sum(changed) >= 0.9 * len(changed), changed
