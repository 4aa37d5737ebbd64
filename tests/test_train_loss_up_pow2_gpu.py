"""T2u's single-pass kernel for x4 / x16 on the device (`-m gpu`): ``CrossEntropy(native=True, up_kernel="pow2").upsampled()``
against float64 and against the unfused device path at every shape of tests/test_train_loss_up_pow2_cpu.py, edge semantics,
batch independence, reproducibility, graph capture, the OHEM pass-through, and the UperNet and Segmenter wiring.

Accuracy rule: tests/test_train_loss_up_gpu.py's ``check_accuracy``, as it stands (float64 on the CPU is the yardstick, ``_up`` +
the plain module on the device the comparator; error of loss and of the low-resolution gradient at most max(2 x the
comparator's, the floor)).  Every pair is printed before it is asserted; the worst pair per shape is in DESIGN section 7."""
import pytest
import torch

from test_train_loss_up_cpu import AUX_SEED, B, interp, make, recipe
from test_train_loss_up_gpu import check_accuracy, run, three_results, ulp32
from test_train_loss_up_pow2_cpu import POW2_SHAPES

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = {"ce": (False, False), "ce_w": (True, False), "ce_tuple": (True, True)}     # class weights, 2-tuple


def pow2_factory(ignore, weights=None):
    """``mk(native, device, double)`` of check_accuracy: the module under test carries up_kernel="pow2"; the yardstick and
    the comparator are plain modules, for which the argument changes nothing"""
    from semseg.losses import CrossEntropy

    def mk(native, device, double):
        w = weights
        if w is not None and device is not None:
            w = w.to(device)
        m = CrossEntropy(ignore, w, native=native, up_kernel="pow2")
        return m.double() if double else m
    return mk


def gather_bits(ignore, weights, preds, y):
    m = make("ce", ignore, None if weights is None else weights.to(DEV), native=True)
    return run(m.upsampled, [p.to(DEV) for p in preds], y.to(DEV))


@pytest.mark.parametrize("ignore", [255, -1])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", list(POW2_SHAPES))
def test_accuracy_and_footprint(name, case, ignore):
    from semseg import _native as N
    weighted, tup = CASES[case]
    shape = POW2_SHAPES[name]
    low, y, weights = recipe(shape, ignore)
    preds = [low, recipe(shape, ignore, seed=AUX_SEED)[0]] if tup else [low]
    wts = weights if weighted else None
    mk = pow2_factory(ignore, wts)
    if not N.train_ce_up_pow2_supported(low, y.shape[-2:]):     # a shape the predicate declines goes where "gather" sends it
        a = run(mk(True, DEV, False).upsampled, [p.to(DEV) for p in preds], y.to(DEV))
        b = gather_bits(ignore, wts, preds, y)
        assert torch.isfinite(a[0]) and torch.equal(a[0], b[0]) and all(torch.equal(g, g0) for g, g0 in zip(a[1], b[1]))
        return
    aux = tuple(float(a) for a in mk(False, None, False).aux_weights[:len(preds)])
    assert aux == ((1.0, 0.4) if tup else (1.0,))
    want, fused, mf = check_accuracy(mk, preds, y, f"pow2 {name} {case} ignore {ignore}", aux)
    assert N.train_words_dict(mf.last_words)["err"] == 0
    for g, g0 in zip(fused[1], want[1]):     # integer ratios: the bilinear weights are exact, the two sets are compared as they are
        assert bool((g0 != 0).any()) and torch.equal(g != 0, g0 != 0)


def test_pow2_is_another_kernel_than_the_gather():
    """The switch does switch: same problem, both within the accuracy rule of the same yardstick, different bits (the two
    kernels round differently), and the pow2 call leaves no full-resolution loss plane behind."""
    from semseg import _native as N
    shape = POW2_SHAPES["x4_C151"]
    low, y, weights = recipe(shape)
    a = run(pow2_factory(255, weights)(True, DEV, False).upsampled, [low.to(DEV)], y.to(DEV))
    b = gather_bits(255, weights, [low], y)
    assert abs(float(a[0]) - float(b[0])) <= 4 * ulp32(float(b[0]))
    assert not torch.equal(a[1][0], b[1][0])
    loss, raw, words = N.train_ce_up_pow2_forward(low.to(DEV), y.shape[-2:], y.to(DEV), weights.to(DEV), 255)
    assert raw.shape == low.shape and raw.dtype == torch.float64 and loss.dim() == 0 and words.numel() == 8
    w = N.train_words_dict(words)
    assert w["n_valid"] == int((y != 255).sum()) and w["err"] == 0
    assert abs(w["sum_w"] - float(weights.double()[y[y != 255]].sum())) <= 1e-9 * w["sum_w"]


@pytest.mark.parametrize("name", ["x4_C21", "x4_C151", "x16_C40", "long_x4_C5", "long_x16_C5"])
def test_raw_of_an_image_does_not_depend_on_its_batch_partner_and_two_runs_agree(name):
    from semseg import _native as N
    low, y, weights = recipe(POW2_SHAPES[name])
    low, y, weights = low.to(DEV), y.to(DEV), weights.to(DEV)
    size = y.shape[-2:]
    outs = [N.train_ce_up_pow2_forward(low, size, y, weights, 255) for _ in range(2)]
    assert torch.isfinite(outs[0][0]) and bool((outs[0][1] != 0).any())
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    g = torch.full((), 0.75, device=DEV)
    d0, d1 = (N.train_ce_up_pow2_backward(o[1], o[2], g) for o in outs)
    assert torch.equal(d0, d1) and bool((d0 != 0).any())
    for i in range(B):
        alone = N.train_ce_up_pow2_forward(low[i:i + 1].contiguous(), size, y[i:i + 1].contiguous(), weights, 255)
        assert torch.equal(alone[1][0], outs[0][1][i]), i


def test_one_image_with_every_label_ignored():
    shape = POW2_SHAPES["x4_C21"]
    low, y, weights = recipe(shape)
    y[1] = 255
    want, fused, _ = check_accuracy(pow2_factory(255, weights), [low], y, "pow2 image 1 ignored")
    assert torch.isfinite(fused[0])
    assert bool((fused[1][0][1] == 0).all()) and bool((fused[1][0][0] != 0).any())


def test_batch_with_every_label_ignored():
    """what the g17 fixtures record for torch: NaN loss, gradient all zeros (no 0 * inf in it)"""
    from semseg import _native as N
    low, y, _ = recipe(POW2_SHAPES["x4_C21"], ignore=-1)
    y[:] = -1
    mod = pow2_factory(-1)(True, DEV, False)
    leaf = low.to(DEV).requires_grad_(True)
    loss = mod.upsampled(leaf, y.to(DEV))
    loss.backward()
    assert torch.isnan(loss) and bool((leaf.grad == 0).all())
    w = N.train_words_dict(mod.last_words)
    assert w["n_valid"] == 0 and w["sum_w"] == 0.0


def test_out_of_range_label_is_ignored_and_flagged():
    from semseg import _native as N
    shape = POW2_SHAPES["x4_C151"]
    low, y, _ = recipe(shape)
    bad = y.clone()
    bad[0, 0, 0], bad[1, 17, 33], bad[1, 35, 35] = 151, -5, 1 << 40
    y[0, 0, 0] = y[1, 17, 33] = y[1, 35, 35] = 255
    mod = pow2_factory(255)(True, DEV, False)
    a = run(mod.upsampled, [low.to(DEV)], y.to(DEV))
    assert N.train_words_dict(mod.last_words)["err"] == 0
    b = run(mod.upsampled, [low.to(DEV)], bad.to(DEV))
    assert N.train_words_dict(mod.last_words)["err"] == 1
    assert torch.isfinite(a[0]) and torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0])


def test_non_contiguous_low_resolution_logits_are_made_contiguous():
    low, y, _ = recipe(POW2_SHAPES["x4_C21"])
    wide = torch.zeros(B, 21, 5, 14)
    wide[..., ::2] = low
    mod = pow2_factory(255)(True, DEV, False)
    a = run(mod.upsampled, [low.to(DEV)], y.to(DEV))
    leaf = wide.to(DEV).requires_grad_(True)
    loss = mod.upsampled(leaf[..., ::2], y.to(DEV))
    loss.backward()
    assert torch.equal(loss.detach().double().cpu(), a[0]) and torch.equal(leaf.grad[..., ::2].double().cpu(), a[1][0])
    assert bool((leaf.grad[..., 1::2] == 0).all())


def test_forward_backward_in_a_captured_graph():
    """No host synchronisation: forward and backward are captured and replayed on new logits written into the same buffer"""
    C, h, S = 21, 32, 128
    gen = torch.Generator(device=DEV).manual_seed(5)
    z0 = torch.randn(B, C, h, h, generator=gen, device=DEV) * 2
    z1 = (z0 + 0.25 * torch.randn(z0.shape, device=DEV, generator=gen)).contiguous()
    y = torch.randint(0, C, (B, S, S), generator=gen, device=DEV)
    y[torch.rand(B, S, S, generator=gen, device=DEV) < 0.05] = -1
    mod = pow2_factory(-1)(True, DEV, False)
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
    with torch.no_grad():
        static.copy_(z1)
    graph.replay()
    torch.cuda.synchronize()
    leaf = z1.clone().requires_grad_(True)
    loss_e = mod.upsampled(leaf, y)
    grad_e, = torch.autograd.grad(loss_e, leaf)
    assert torch.isfinite(loss_e) and torch.equal(loss_c, loss_e.detach()) and torch.equal(grad_c, grad_e)
    leaf0 = z0.clone().requires_grad_(True)
    assert not torch.equal(mod.upsampled(leaf0, y).detach(), loss_e.detach())   # the replay did see the new logits


@pytest.mark.parametrize("name", ["x4_C21", "x16_C40"])
def test_ohem_ignores_the_argument(name):
    from semseg.losses import OhemCrossEntropy
    low, y, _ = recipe(POW2_SHAPES[name])
    a = run(OhemCrossEntropy(255, native=True, up_kernel="pow2").upsampled, [low.to(DEV)], y.to(DEV))
    b = run(make("ohem", 255, native=True).upsampled, [low.to(DEV)], y.to(DEV))
    assert torch.isfinite(a[0]) and torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0])


@pytest.mark.parametrize("kernel", ["pow2", "gather"])
def test_upernet_training_forward_with_the_kernel_switch(kernel):
    """TRAIN_FUSED_CRITERION on, TRAIN_FUSED_KERNEL = kernel: the fused forward's loss and both heads' gradients are the bits
    of the standalone ``upsampled`` calls with that kernel (main head x4 and auxiliary head x16 in one step); for "gather"
    the standalone module is built without the argument, as before the switch existed."""
    from semseg.losses import CrossEntropy
    from semseg.models import convnext_upernet as M
    C, S = 151, 128
    torch.manual_seed(0)
    model = M.UperNetForSemanticSegmentation("ConvNeXt-T_CVST", C, None).to(DEV).train()
    for m in model.modules():
        if isinstance(m, M.StochasticDepth):
            m.p = 0.0
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(B, 3, S, S, generator=gen).to(DEV)
    y = torch.randint(0, C, (B, S, S), generator=gen)
    y[torch.rand(B, S, S, generator=gen) < 0.1] = -1
    y = y.to(DEV)
    kept = {}

    def keep(key):
        def hook(module, args, out):
            out.retain_grad()
            kept[key] = out
        return hook

    hooks = [model.decode_head.register_forward_hook(keep("main")), model.auxiliary_head.register_forward_hook(keep("aux"))]
    prev = M.TRAIN_FUSED_CRITERION, M.TRAIN_FUSED_KERNEL
    M.TRAIN_FUSED_CRITERION, M.TRAIN_FUSED_KERNEL = True, kernel
    try:
        assert M._fused_criterion().up_kernel == kernel
        loss, second = model(x, y)
        loss.backward()
    finally:
        M.TRAIN_FUSED_CRITERION, M.TRAIN_FUSED_KERNEL = prev
        for hk in hooks:
            hk.remove()
    main, aux = kept["main"], kept["aux"]
    assert second is None and main.shape == (B, C, S // 4, S // 4) and aux.shape == (B, C, S // 16, S // 16)
    crit = CrossEntropy(-1, native=True, up_kernel="pow2") if kernel == "pow2" else CrossEntropy(-1, native=True)
    lm = main.detach().float().contiguous().requires_grad_(True)
    la = aux.detach().float().contiguous().requires_grad_(True)
    alone = crit.upsampled(lm, y) + 0.4 * crit.upsampled(la, y)
    alone.backward()
    assert torch.isfinite(loss) and torch.equal(loss.detach(), alone.detach())
    assert torch.equal(main.grad, lm.grad) and torch.equal(aux.grad, la.grad)
    assert bool((lm.grad != 0).any()) and bool((la.grad != 0).any())


# ---- Segmenter ------------------------------------------------------------------------------------------------------------
SEG_SIZE = 16        # the smallest multiple of the patch size: one patch, a 1 x 1 map of masks up-sampled x16
SEG_C = 151


@pytest.fixture(scope="module")
def segmenter():
    from real_models import build_model
    model = build_model("segmenter", "vit_small_patch16_224", SEG_C).to(DEV).eval()
    gen = torch.Generator().manual_seed(3)
    im = torch.rand(B, 3, SEG_SIZE, SEG_SIZE, generator=gen).to(DEV)
    y = torch.randint(0, SEG_C, (B, SEG_SIZE, SEG_SIZE), generator=gen)
    y[torch.rand(B, SEG_SIZE, SEG_SIZE, generator=gen) < 0.1] = -1
    return model, im, y.to(DEV)


def load_tool():
    import importlib.util
    import os
    from conftest import PKG
    spec = importlib.util.spec_from_file_location("train_rob_seg_pow2_gpu", os.path.join(PKG, "tools", "train_rob_seg.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_segmenter_lowres_argument(segmenter):
    model, im, _ = segmenter
    with torch.no_grad():
        full = model(im)
        low = model(im, lowres=True)
        hook, size = model.forward_lowres(im)
        assert torch.equal(model(im, lowres=False), full) and torch.equal(model.forward(im), full)
        assert model(im[:, :, :SEG_SIZE - 3, :SEG_SIZE - 5], lowres=True) is None      # would need padding
    assert full.shape == (B, SEG_C, SEG_SIZE, SEG_SIZE) and size == (SEG_SIZE, SEG_SIZE)
    assert low.shape == (B, SEG_C, SEG_SIZE // 16, SEG_SIZE // 16) and torch.equal(low, hook)
    from semseg.models.convnext_upernet import _up
    assert torch.equal(_up(low, (SEG_SIZE, SEG_SIZE)), full)     # forward(im) is the up-sampled hook, as before


def test_segmenter_branch_of_the_tool_with_the_fused_pow2_criterion(segmenter):
    """``segmenter_loss`` with fused + pow2: a finite loss whose bits and whose gradient with respect to the low-resolution
    masks are those of the standalone criterion on the hooked masks; that criterion against the unfused branch (``_up`` +
    F.cross_entropy(ignore_index=-1) = the comparator of the accuracy rule) and float64; and over forward + backward the
    fused branch peaks at least two (B, C, H, W) fp32 tensors below the unfused one (logits and log-soft-max are alive
    together there)."""
    from semseg import _native as N
    model, im, y = segmenter
    tool = load_tool()
    fused = tool.build_fused_criterion("pow2").to(DEV)
    kept = {}

    def hook(module, args, out):
        out.retain_grad()
        kept["low"] = out

    def step(fused_crit, whole=True):
        """forward + backward of the branch; whole=False stops the backward at the low-resolution masks, so that the peak is
        the criterion's and not that of the parameter gradients the ViT's backward creates (2.4 MB for one MLP weight, more
        than a (B, C, H, W) tensor at this size)"""
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        loss = tool.segmenter_loss(model, im, y, None, fused_crit)
        if whole:
            loss.backward()
        else:
            torch.autograd.grad(loss, kept["low"])
        torch.cuda.synchronize()
        return loss.detach(), torch.cuda.max_memory_allocated() - base

    hk = model.decoder.register_forward_hook(hook)
    try:
        step(None)                        # warm-up: library workspaces
        loss_off, _ = step(None)
        step(fused)
        loss_on, _ = step(fused)
        low = kept["low"]
        g_low = low.grad.clone()
    finally:
        hk.remove()
    kept.clear()
    assert low.shape == (B, SEG_C, SEG_SIZE // 16, SEG_SIZE // 16) and N.train_ce_up_pow2_supported(low, y.shape[-2:])
    leaf = low.detach().float().contiguous().requires_grad_(True)
    alone = fused.upsampled(leaf, y)
    alone.backward()
    assert torch.isfinite(loss_on) and torch.equal(loss_on, alone.detach()) and torch.equal(g_low, leaf.grad)
    assert bool((g_low != 0).any())
    torch.testing.assert_close(loss_on, loss_off, rtol=1e-5, atol=0)
    # the accuracy rule on the model's masks: comparator = the unfused branch's arithmetic
    check_accuracy(pow2_factory(-1), [low.detach().float().cpu()], y.cpu(), "pow2 segmenter masks")
    del low, g_low, leaf, alone
    hk = model.decoder.register_forward_hook(hook)
    try:
        peak_off = step(None, whole=False)[1]
        peak_on = step(fused, whole=False)[1]
    finally:
        hk.remove()
        kept.clear()
    need = 2 * B * SEG_C * SEG_SIZE * SEG_SIZE * 4
    print(f"[pow2 segmenter] loss fused {float(loss_on):.9g} unfused {float(loss_off):.9g} | peak above the resident set over "
          f"forward + backward: unfused {peak_off} B, fused {peak_on} B, saved {peak_off - peak_on} B (required >= {need})")
    assert peak_off - peak_on >= need, (peak_off, peak_on, need)
    # an input that needs padding: the model declines, the branch takes the unfused line
    odd = im[:, :, :SEG_SIZE - 3, :SEG_SIZE - 5].contiguous()
    yo = y[:, :SEG_SIZE - 3, :SEG_SIZE - 5].contiguous()
    with torch.no_grad():
        a = tool.segmenter_loss(model, odd, yo, None, fused)
        b = tool.segmenter_loss(model, odd, yo, None, None)
    assert torch.isfinite(a) and torch.equal(a, b)
