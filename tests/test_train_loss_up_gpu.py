"""T2u on the device (`-m gpu`): ``CrossEntropy`` / ``OhemCrossEntropy`` ``.upsampled()`` with ``native=True`` on
low-resolution logits, against float64 and against the unfused device path, at every shape of
tests/test_train_loss_up_cpu.py; selection, ties, edge semantics, reproducibility, graph capture, fallback and the UperNet
wiring behind ``SEA_TRAIN_FUSED_LOSS``.

Accuracy rule: tests/test_train_loss_gpu.py's, as it stands.  The yardstick is float64 on CPU (``F.interpolate`` of the double
tensor, then the plain module in double).  The comparator is the unfused path on the device: ``_up`` (M2) + the module with
``native=False``, fp32, same tensors.  The fused path's loss error is at most max(2 x the comparator's, the loss floor), its
gradient error (with respect to the LOW-resolution tensor, max-abs over elements) at most max(2 x the comparator's, one fp32
ulp of the largest gradient element).  Loss floor: half an fp32 ulp of the loss; for a tuple ``loss_floor`` of that file (half
an ulp per prediction times its weight, per product with a weight other than 1, per addition).  Every pair is printed before
it is asserted; the measured pairs are in DESIGN section 7."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_train_loss_up_cpu import AUX_SEED, B, SHAPES, assert_selection_unambiguous, interp, make, recipe, shape_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = list(SHAPES)
# kind -> (module kind, class weights, OHEM probability threshold, tuple)
CASES = {"ce": ("ce", False, None, False), "ce_w": ("ce", True, None, False), "ohem_0.7": ("ohem", False, 0.7, False),
         "ohem_0.05": ("ohem", False, 0.05, False), "ohem_topk": ("ohem", False, 1e-9, False),
         "ce_tuple": ("ce", True, None, True), "ohem_tuple": ("ohem", False, 0.7, True)}


def ulp32(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(abs(x))) - 23) if x and math.isfinite(x) else 2.0 ** -149


def up_device(p, y):
    from semseg.models.convnext_upernet import _up
    return _up(p, y.shape[-2:])


def run(fn, preds, y):
    leaves = [p.clone().requires_grad_(True) for p in preds]
    loss = fn(tuple(leaves) if len(leaves) > 1 else leaves[0], y)
    loss.backward()
    return loss.detach().double().cpu(), [p.grad.double().cpu() for p in leaves]


def three_results(mk, preds, y):
    """(float64 yardstick, unfused device path, fused device path) of the module mk(native, device, double)"""
    m64 = mk(False, None, True)
    want = run(lambda p, t: m64(tuple(interp(q, t) for q in p) if isinstance(p, tuple) else interp(p, t), t),
               [p.double() for p in preds], y)
    ms = mk(False, DEV, False)
    stock = run(lambda p, t: ms(tuple(up_device(q, t) for q in p) if isinstance(p, tuple) else up_device(p, t), t),
                [p.to(DEV) for p in preds], y.to(DEV))
    mf = mk(True, DEV, False)
    fused = run(mf.upsampled, [p.to(DEV) for p in preds], y.to(DEV))
    return want, stock, fused, mf


def errors(got, want):
    (l, gs), (l0, gs0) = got, want
    return abs(float(l) - float(l0)), max(float((g - g0).abs().max()) for g, g0 in zip(gs, gs0))


def loss_floor(mk, preds, y, aux_weights, total):
    """tests/test_train_loss_gpu.py: loss_floor, from the float64 losses of the single predictions"""
    if len(preds) == 1:
        return 0.5 * ulp32(total)
    bound = 0.5 * ulp32(total) * (len(preds) - 1)
    m64 = mk(False, None, True)
    for p, a in zip(preds, aux_weights):
        lk = float(m64(interp(p.double(), y), y))
        bound += a * 0.5 * ulp32(lk) + (0.5 * ulp32(a * lk) if a != 1.0 else 0.0)
    return bound


def check_accuracy(mk, preds, y, tag, aux_weights=(1.0,)):
    want, stock, fused, mf = three_results(mk, preds, y)
    e_s, e_f = errors(stock, want), errors(fused, want)
    gmax = max(float(g.abs().max()) for g in want[1])
    floors = (loss_floor(mk, preds, y, aux_weights, float(want[0])), ulp32(gmax))
    print(f"[T2u {tag}] loss err T2u {e_f[0]:.3e} unfused {e_s[0]:.3e} | grad err T2u {e_f[1]:.3e} unfused {e_s[1]:.3e} "
          f"| floors {floors[0]:.2e} {floors[1]:.2e}")
    assert e_f[0] <= max(2 * e_s[0], floors[0]), (e_f, e_s, floors)
    assert e_f[1] <= max(2 * e_s[1], floors[1]), (e_f, e_s, floors)
    return want, fused, mf


def assert_same_footprint(g, g0, shape):
    """The gradient is non-zero at exactly the low-resolution elements the yardstick's selected pixels touch.  With integer
    ratios the bilinear weights are exact in fp32 and in float64 alike, and the two sets are compared as they are.  With a
    fractional ratio a source coordinate that is an integer in exact arithmetic (5/17 * 8.5 - 0.5 = 2) rounds to either side
    in either precision: a weight of 0 in one is a weight of one rounding of the coordinate (2^-22 at coordinates below 4) in
    the other, so elements whose gradient is below 2^-20 of the largest one in BOTH results may be zero in one of them."""
    _, h, w, H, W = shape
    if H % h == 0 and W % w == 0:
        assert torch.equal(g != 0, g0 != 0)
        return
    tol = 2.0 ** -20 * float(g0.abs().max())
    differ = (g != 0) != (g0 != 0)
    assert bool(((g.abs() <= tol) & (g0.abs() <= tol))[differ].all()), int(differ.sum())


def module_factory(kind, ignore, weights, thresh):
    def mk(native, device, double):
        w = weights
        if w is not None and device is not None:
            w = w.to(device)
        m = make(kind, ignore, w, native=native, thresh=0.7 if thresh is None else thresh)
        return m.double() if double else m
    return mk


@pytest.mark.parametrize("ignore", [255, -1])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", NAMES)
def test_accuracy_selection_and_footprint(name, case, ignore):
    from semseg import _native as N
    kind, weighted, thresh, tup = CASES[case]
    shape = shape_of(name)
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
        if case in ("ohem_0.7", "ohem_0.05") and name != "clamped_C21":
            assert mode == 0


def test_ratio_one_agrees_with_t2():
    """h x w -> h x w: the interpolation is the identity, T2u solves T2's problem.  Both under the accuracy rule against the
    same float64 result (asserted for T2u above); here T2's error is the comparator."""
    shape = shape_of("ratio1_C21")
    low, y, weights = recipe(shape)
    for kind in ("ce", "ohem"):
        wts = weights if kind == "ce" else None     # (the recipe's OHEM selection is checked without class weights)
        if kind == "ohem":
            assert_selection_unambiguous(low, y, 255, 0.7)
        want = run(make(kind, 255, wts).double(), [low.double()], y)
        wd = None if wts is None else wts.to(DEV)
        t2 = run(make(kind, 255, wd, native=True), [low.to(DEV)], y.to(DEV))
        t2u = run(make(kind, 255, wd, native=True).upsampled, [low.to(DEV)], y.to(DEV))
        e2, eu = errors(t2, want), errors(t2u, want)
        floors = (0.5 * ulp32(float(want[0])), ulp32(float(want[1][0].abs().max())))
        print(f"[T2u ratio 1 {kind}] loss err T2u {eu[0]:.3e} T2 {e2[0]:.3e} | grad err T2u {eu[1]:.3e} T2 {e2[1]:.3e} "
              f"| floors {floors[0]:.2e} {floors[1]:.2e}")
        assert eu[0] <= max(2 * e2[0], floors[0]) and eu[1] <= max(2 * e2[1], floors[1])


def test_exact_ties_are_taken_in_ascending_pixel_index():
    """All-zero logits: every valid pixel's loss is ln 21, the regime is top-k, and the selected pixels are the first n_min
    valid ones in ascending flat index (T2's rule)."""
    from semseg import _native as N
    shape = shape_of("x4_C21")
    _, y, _ = recipe(shape)
    low = torch.zeros(B, *shape[:3])
    valid = (y != 255).view(-1)
    n_min = int(valid.sum()) // 16
    mask = torch.zeros_like(valid)
    mask[valid.nonzero().view(-1)[:n_min]] = True
    mask = mask.view(y.shape)

    def masked(p, t, up):     # the criterion with the selection given
        px = F.cross_entropy(up(p, t), t, ignore_index=255, reduction="none")
        return (px * mask.to(px)).sum() / n_min

    want = run(lambda p, t: masked(p, t, interp), [low.double()], y)
    stock = run(lambda p, t: masked(p, t, up_device), [low.to(DEV)], y.to(DEV))
    mod = make("ohem", 255, native=True, thresh=1e-9)
    leaf = low.to(DEV).requires_grad_(True)
    loss = mod.upsampled(leaf, y.to(DEV))
    loss.backward()
    w = N.train_words_dict(mod.last_words)
    assert (w["mode"], w["n_min"], w["n_sel"], w["err"]) == (1, n_min, n_min, 0), w
    assert w["take"] == n_min and abs(w["t"] - math.log(21)) <= ulp32(math.log(21)), w
    # the selected pixels, from the loss plane the select marked
    _, loss_px, _ = N.train_ce_up_forward(leaf.detach(), y.shape[-2:], y.to(DEV), None, 255, float(mod.thresh), True)
    assert torch.equal((loss_px != -1).view(y.shape).cpu() & (y != 255), mask)
    fused = (loss.detach().double().cpu(), [leaf.grad.double().cpu()])
    e_s, e_f = errors(stock, want), errors(fused, want)
    floors = (0.5 * ulp32(float(want[0])), ulp32(float(want[1][0].abs().max())))
    print(f"[T2u ties] loss err T2u {e_f[0]:.3e} unfused {e_s[0]:.3e} | grad err T2u {e_f[1]:.3e} unfused {e_s[1]:.3e} "
          f"| floors {floors[0]:.2e} {floors[1]:.2e}")
    assert e_f[0] <= max(2 * e_s[0], floors[0]) and e_f[1] <= max(2 * e_s[1], floors[1])
    assert torch.equal(fused[1][0] != 0, want[1][0] != 0)


@pytest.mark.parametrize("kind", ["ce", "ohem"])
def test_one_image_with_every_label_ignored(kind):
    shape = shape_of("halo_C21")
    low, y, weights = recipe(shape)
    y[1] = 255
    mk = module_factory(kind, 255, weights if kind == "ce" else None, 0.7)
    if kind == "ohem":
        assert_selection_unambiguous(low, y, 255, 0.7)
    want, fused, _ = check_accuracy(mk, [low], y, f"image 1 ignored {kind}")
    assert bool((fused[1][0][1] == 0).all()) and bool((fused[1][0][0] != 0).any())


@pytest.mark.parametrize("kind", ["ce", "ohem"])
def test_batch_with_every_label_ignored(kind):
    """what the g17 fixtures record for torch: NaN loss, gradient all zeros (no NaN in it)"""
    low, y, _ = recipe(shape_of("x4_C21"), ignore=-1)
    y[:] = -1
    mod = make(kind, -1, native=True)
    leaf = low.to(DEV).requires_grad_(True)
    loss = mod.upsampled(leaf, y.to(DEV))
    loss.backward()
    assert torch.isnan(loss) and bool((leaf.grad == 0).all())


def test_out_of_range_label_is_ignored_and_flagged():
    from semseg import _native as N
    shape = shape_of("halo_C21")
    low, y, _ = recipe(shape)
    bad = y.clone()
    bad[0, 0, 0], bad[1, 17, 33], bad[1, 35, 35] = 21, -5, 1 << 40
    y[0, 0, 0] = y[1, 17, 33] = y[1, 35, 35] = 255
    mod = make("ce", 255, native=True)
    a = mod.upsampled(low.to(DEV), y.to(DEV))
    assert N.train_words_dict(mod.last_words)["err"] == 0
    b = mod.upsampled(low.to(DEV), bad.to(DEV))
    assert N.train_words_dict(mod.last_words)["err"] == 1
    assert torch.isfinite(a) and torch.equal(a, b)


@pytest.mark.parametrize("ohem", [False, True], ids=["ce", "ohem"])
@pytest.mark.parametrize("name", ["halo_C21", "x4_C151", "x16_C40"])
def test_two_runs_give_the_same_bits(name, ohem):
    from semseg import _native as N
    low, y, weights = recipe(shape_of(name))
    low, y, weights = low.to(DEV), y.to(DEV), weights.to(DEV)
    g = torch.full((), 0.75, device=DEV)
    outs = []
    for _ in range(2):
        loss, loss_px, words = N.train_ce_up_forward(low, y.shape[-2:], y, weights, 255, 0.3566749, ohem)
        dlow = N.train_ce_up_backward(low, y.shape[-2:], y, weights, 255, ohem, loss_px, words, g)
        outs.append((loss, loss_px, dlow))
    assert torch.isfinite(outs[0][0]) and bool((outs[0][2] != 0).any())
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_forward_backward_in_a_captured_graph():
    """No host synchronisation: forward, select and backward are captured and replayed on new logits written into the same
    buffer (tests/test_train_loss_gpu.py's capture test, on low-resolution logits; top-k regime)."""
    from semseg import _native as N
    C, h, S = 21, 32, 128
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
        torch.autograd.grad(mod.upsampled(static, y), static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_c = mod.upsampled(static, y)
        grad_c, = torch.autograd.grad(loss_c, static)
        words_c = mod.last_words
    with torch.no_grad():
        static.copy_(z1)
    graph.replay()
    torch.cuda.synchronize()
    w = N.train_words_dict(words_c)
    assert w["mode"] == 1 and w["n_sel"] == w["n_min"] > 0, w
    leaf = z1.clone().requires_grad_(True)
    loss_e = mod.upsampled(leaf, y)
    grad_e, = torch.autograd.grad(loss_e, leaf)
    assert torch.isfinite(loss_e) and torch.equal(loss_c, loss_e.detach()) and torch.equal(grad_c, grad_e)
    leaf0 = z0.clone().requires_grad_(True)
    assert not torch.equal(mod.upsampled(leaf0, y).detach(), loss_e.detach())   # the replay did see the new logits


@pytest.mark.parametrize("kind", ["ce", "ohem"])
def test_class_count_without_a_kernel_takes_up_plus_t2(kind):
    """C = 200 is above T2u's ceiling: ``upsampled`` is ``_up`` + T2, bit for bit"""
    from semseg import _native as N
    low, y, _ = recipe((200, 5, 7, 20, 28))
    assert not N.train_ce_up_supported(low, y.shape[-2:])
    mod = make(kind, 255, native=True)
    a = run(mod.upsampled, [low.to(DEV)], y.to(DEV))
    b = run(lambda p, t: mod(up_device(p, t), t), [low.to(DEV)], y.to(DEV))
    assert torch.isfinite(a[0]) and torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0])
    with pytest.raises(N.SeaNativeError):
        N.train_ce_up_forward(low.to(DEV), y.shape[-2:], y.to(DEV), None, 255)


def test_non_contiguous_low_resolution_logits_are_made_contiguous():
    low, y, _ = recipe(shape_of("x4_C21"))
    wide = torch.zeros(B, 21, 5, 14)
    wide[..., ::2] = low
    mod = make("ce", 255, native=True)
    a = run(mod.upsampled, [low.to(DEV)], y.to(DEV))
    leaf = wide.to(DEV).requires_grad_(True)
    loss = mod.upsampled(leaf[..., ::2], y.to(DEV))
    loss.backward()
    assert torch.equal(loss.detach().double().cpu(), a[0]) and torch.equal(leaf.grad[..., ::2].double().cpu(), a[1][0])


def test_upernet_training_forward_behind_the_switch():
    """SEA_TRAIN_FUSED_LOSS on: forward(input, lbl) in train mode is CE_up(main) + 0.4 CE_up(aux) on the heads' low-resolution
    outputs (x4 and x16), returns (loss, None), reaches the same parameters, and max_memory_allocated over forward + backward
    is lower by at least two full-resolution logits tensors, 2 * B*C*H*W*4 bytes = 37.8 MiB here (a floor: at the criterion
    the unfused step holds the returned logits and two log-soft-max results at once).

    The memory comparison runs with the parameter gradients RESIDENT (zeroed in place before the step, as a training loop
    that accumulates or calls zero_grad(set_to_none=False) has them), so that the step's peak is where the activations are
    all alive, at the criterion: measured 845.2 MiB unfused, 798.7 MiB fused, 46.4 MiB saved.  With the gradients freed
    before the step (set_to_none=True) this 2 x 3 x 128 x 128 step creates 230 MiB of parameter gradients during the
    backward and peaks at its END (700.0 MiB unfused; about 590 after the forward), where the log-soft-max
    tensors are long gone and only the logits tensor that forward returned is still alive: 682.1 MiB fused, 17.9 MiB = one
    tensor saved, which no criterion can raise.  Those figures are printed too."""
    from semseg.models import convnext_upernet as M
    C, S = 151, 128
    torch.manual_seed(0)
    model = M.UperNetForSemanticSegmentation("ConvNeXt-T_CVST", C, None).to(DEV).train()
    rates = [m for m in model.modules() if isinstance(m, M.StochasticDepth)]
    assert rates
    for m in rates:
        m.p = 0.0
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(B, 3, S, S, generator=gen).to(DEV)
    y = torch.randint(0, C, (B, S, S), generator=gen)
    y[torch.rand(B, S, S, generator=gen) < 0.1] = -1
    y = y.to(DEV)
    kept = {}

    def keep(key):
        def hook(module, args, out):      # (returns None: the output goes on unchanged)
            out.retain_grad()
            kept[key] = out
        return hook

    hooks = [model.decode_head.register_forward_hook(keep("main")), model.auxiliary_head.register_forward_hook(keep("aux"))]

    def step(on, resident=False):
        """one forward + backward; returns (loss, what forward returned second as a shape or None, parameters with a
        finite gradient, max_memory_allocated over the step).  Nothing of the step but these stays alive."""
        prev = M.TRAIN_FUSED_CRITERION
        M.TRAIN_FUSED_CRITERION = on
        try:
            if resident:
                for p in model.parameters():
                    if p.grad is not None:
                        p.grad.zero_()
            else:
                model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            loss, second = model(x, y)
            loss.backward()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated()
        finally:
            M.TRAIN_FUSED_CRITERION = prev
        got = {k for k, p in model.named_parameters() if p.grad is not None and bool(torch.isfinite(p.grad).all())}
        return loss.detach(), None if second is None else tuple(second.shape), got, peak

    try:
        step(False)                                   # warm-up: library workspaces and find-mode allocations
        loss_off, second_off, params_off, free_off = step(False)
        step(True)
        loss_on, second_on, params_on, free_on = step(True)
        main, aux = kept["main"], kept["aux"]
        g_main, g_aux = main.grad.clone(), aux.grad.clone()
    finally:
        for hk in hooks:
            hk.remove()
    kept.clear()
    assert second_on is None and second_off == (B, C, S, S)
    assert params_on == params_off and len(params_on) > 100
    assert main.shape == (B, C, S // 4, S // 4) and aux.shape == (B, C, S // 16, S // 16)   # x4 and x16 in one step
    # the same loss and head gradients, recomputed standalone from the hooked tensors of that forward
    crit = make("ce", -1, native=True)
    lm = main.detach().float().contiguous().requires_grad_(True)
    la = aux.detach().float().contiguous().requires_grad_(True)
    alone = crit.upsampled(lm, y) + 0.4 * crit.upsampled(la, y)
    alone.backward()
    assert torch.isfinite(loss_on) and torch.equal(loss_on, alone.detach())
    assert torch.equal(g_main, lm.grad) and torch.equal(g_aux, la.grad)
    torch.testing.assert_close(loss_on, loss_off, rtol=1e-5, atol=0)
    del main, aux, g_main, g_aux, lm, la, alone
    # memory, gradients resident (left by the steps above)
    peak_off = step(False, resident=True)[3]
    peak_on = step(True, resident=True)[3]
    need = 2 * B * C * S * S * 4
    mib = 2.0 ** 20
    print(f"[T2u model] loss fused {float(loss_on):.9g} unfused {float(loss_off):.9g} | max_memory_allocated, gradients "
          f"resident: unfused {peak_off / mib:.1f} MiB fused {peak_on / mib:.1f} MiB, saved {(peak_off - peak_on) / mib:.1f} "
          f"MiB (required >= {need / mib:.1f}) | gradients freed before the step: unfused {free_off / mib:.1f} fused "
          f"{free_on / mib:.1f}, saved {(free_off - free_on) / mib:.1f} MiB")
    assert peak_off - peak_on >= need, (peak_off, peak_on, need)
    assert free_on < free_off
