"""T2 on the device (`-m gpu`): ``CrossEntropy`` / ``OhemCrossEntropy`` with ``native=True`` against the g17 fixtures of
the reference, against the stock device criterion, at the training size, and inside a captured graph.

Accuracy rule (the project's convention for M8, README "asserted <= 2 x"): the yardstick is the float64 result of the
same inputs on CPU; T2's error against it must be at most twice the stock device criterion's (``native=False``, same
tensors on the GPU).  Floors: for the gradient one fp32 ulp of the largest gradient element; for the loss the rounding
bound of the fp32 arithmetic that returns it (a stock result that happens to be the correctly rounded one has error ~0,
and twice that could not be met by any fp32 output).  One prediction: half an fp32 ulp of the loss.  A tuple is
``sum(w_k * loss_k)`` in fp32 on fp32 ``loss_k`` (the module's arithmetic, asserted bit for bit below), so each
``loss_k`` brings half an ulp of its own times ``w_k``, each product with ``w_k != 1`` half an ulp of the product and each
addition half an ulp of the total: ``loss_floor``.  With bf16 logits the class weights are bf16 too (the stock criterion
wants one dtype), so the float64 yardstick takes the bf16-rounded weights: they are inputs like the logits.  Every pair
is printed before it is asserted; the measured pairs are in DESIGN section 7."""
import math
import os

import pytest
import torch

from test_train_loss_cpu import FILES, load_case, make_module, run_module

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
IDS = [os.path.basename(f)[15:-4] for f in FILES]


def ulp32(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(abs(x))) - 23) if x and math.isfinite(x) else 2.0 ** -149


def f64_result(case):
    """the criterion in float64 on CPU (the plain module: same selection rule, double arithmetic)"""
    mod = make_module(case, native=False).double()
    return run_module(mod, [p.double() for p in case["preds"]], case["labels"])


def device_result(case, native, dtype):
    mod = make_module(case, native=native, device=DEV).to(DEV)
    preds = [p.to(DEV, dtype) for p in case["preds"]]
    if dtype != torch.float32:
        mod = mod.to(dtype)
    loss, grads = run_module(mod, preds, case["labels"].to(DEV))
    return loss.double().cpu(), [g.double().cpu() for g in grads]


def errors(got, want):
    (l, gs), (l0, gs0) = got, want
    return abs(float(l) - float(l0)), max(float((g - g0).abs().max()) for g, g0 in zip(gs, gs0))


def loss_floor(case, total):
    """rounding bound of the fp32 value the module returns, from the float64 losses of the single predictions"""
    if len(case["preds"]) == 1:
        return 0.5 * ulp32(total)
    bound = 0.5 * ulp32(total) * (len(case["preds"]) - 1)
    for p, a in zip(case["preds"], case["aux"]):
        lk = float(f64_result(dict(case, preds=[p]))[0])
        bound += a * 0.5 * ulp32(lk) + (0.5 * ulp32(a * lk) if a != 1.0 else 0.0)
    return bound


def check_accuracy(case, dtype, tag):
    if dtype == torch.bfloat16 and case["weights"] is not None:
        case = dict(case, weights=case["weights"].bfloat16().float())
    want = f64_result(case)
    stock = errors(device_result(case, False, dtype), want)
    t2_out = device_result(case, True, dtype)
    t2 = errors(t2_out, want)
    ref = errors(t2_out, (case["loss"].double(), [g.double() for g in case["grads"]]))
    gmax = max(float(g.abs().max()) for g in want[1])
    floors = (loss_floor(case, float(want[0])), ulp32(gmax))
    print(f"[T2 {tag}] loss err T2 {t2[0]:.3e} stock {stock[0]:.3e} | grad err T2 {t2[1]:.3e} stock {stock[1]:.3e} "
          f"| floors {floors[0]:.2e} {floors[1]:.2e} | vs reference fixture {ref[0]:.3e} {ref[1]:.3e}")
    assert t2[0] <= max(2 * stock[0], floors[0]), (t2, stock, floors)
    assert t2[1] <= max(2 * stock[1], floors[1]), (t2, stock, floors)


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_fixture_fp32(path):
    from semseg import _native as N
    case = load_case(path)
    if case["regime"] == 2:
        # every label ignored.  The fixture says what torch does for these inputs: NaN loss, gradient all zeros (no NaN)
        assert torch.isnan(case["loss"]) and all(bool((g == 0).all()) for g in case["grads"])
        loss, grads = device_result(case, True, torch.float32)
        assert torch.isnan(loss) and all(bool((g == 0).all()) for g in grads)
    else:
        check_accuracy(case, torch.float32, os.path.basename(path)[15:-4] + " fp32")
    if case["ohem"]:
        # regime and selected-pixel count, read back from the device words AFTER the step (here only)
        labels = case["labels"].to(DEV)
        for k, p in enumerate(case["preds"]):
            mod = make_module(case, native=True, device=DEV).to(DEV)
            leaf = p.to(DEV).requires_grad_(True)
            mod(leaf, labels).backward()
            w = N.train_words_dict(mod.last_words)
            assert w["err"] == 0 and w["n_min"] == case["n_min"][k]
            assert w["mode"] == (1 if case["regime"] == 1 else 0), (w, case["regime"])
            assert w["n_sel"] == case["n_sel"][k], (w, case["n_sel"])
            # a selected pixel has a loss > 0, so it is not ignored and its gradient p - onehot is not zero: the
            # gradient is non-zero at exactly n_sel pixels, none of them ignored
            touched = (leaf.grad != 0).any(1)
            assert int(touched.sum()) == case["n_sel"][k]
            assert not bool((touched & (labels == case["ignore"])).any())


@pytest.mark.parametrize("path", [f for f in FILES if "all_ignored" not in f],
                         ids=[i for i in IDS if "all_ignored" not in i])
def test_fixture_bf16(path):
    case = load_case(path)   # the fixtures' logits are bf16-representable: the float64 yardstick is that of the bf16 inputs
    for p in case["preds"]:
        assert torch.equal(p.bfloat16().float(), p)
    check_accuracy(case, torch.bfloat16, os.path.basename(path)[15:-4] + " bf16")


def test_out_of_range_label_is_ignored_and_flagged():
    from semseg import _native as N
    from semseg.losses import CrossEntropy
    g = torch.Generator().manual_seed(3)
    z = torch.randn(1, 5, 8, 8, generator=g).to(DEV)
    y = torch.randint(0, 5, (1, 8, 8), generator=g)
    bad = y.clone()
    bad[0, 0, 0], bad[0, 3, 3] = 7, -5
    y[0, 0, 0] = y[0, 3, 3] = 255
    mod = CrossEntropy(255, native=True)
    a = mod(z, y.to(DEV))
    assert N.train_words_dict(mod.last_words)["err"] == 0
    b = mod(z, bad.to(DEV))
    assert N.train_words_dict(mod.last_words)["err"] == 1
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [21, 40])
@pytest.mark.parametrize("kind", ["ce", "ohem"])
def test_odd_pixel_count_takes_the_scalar_kernels(kind, C, dtype):
    """H*W = 7 * 9 = 63 is odd (as PSPNet's 473 x 473 is): one pixel per lane in the forward, in the register backward
    (C <= 32) and in the streaming backward (C > 32).  Same accuracy rule as the fixtures."""
    g = torch.Generator().manual_seed(100 + C)
    y = torch.randint(0, C, (2, 7, 9), generator=g)
    z = torch.randn(2, C, 7, 9, generator=g) * 3
    z.scatter_add_(1, y[:, None], ((torch.rand(2, 7, 9, generator=g) < 0.7).float() * 6.0)[:, None])
    y[torch.rand(2, 7, 9, generator=g) < 0.1] = -1
    case = dict(ohem=kind == "ohem", ignore=-1, weights=0.5 + torch.rand(C, generator=g), labels=y, aux=[1.0],
                preds=[z.bfloat16().float()], loss=torch.zeros(()), grads=[torch.zeros_like(z)])
    check_accuracy(case, dtype, f"odd {kind} C{C} {dtype}")


def test_ohem_ties_at_the_cut_are_taken_in_ascending_pixel_index():
    """Constructed ties: three kinds of pixel (label 0, logits (a, 0, 0, 0, 0), loss log(1 + 4 exp(-a)) = 0.284 / 0.181 /
    0.001, all below -log 0.7 so the regime is top-k).  101 pixels of the first kind, 300-odd of the second spread over all
    three blocks of the select (6144 pixels, chunks of 2048), n_min = 384: the cut falls inside the second kind, whose
    losses are identical bit for bit, and the 283 with the lowest flat index are the ones taken."""
    from semseg import _native as N
    from semseg.losses import OhemCrossEntropy
    n = 64 * 96
    idx = torch.arange(n)
    kind_a, kind_b = idx % 61 == 0, (idx % 20 == 1) & (idx % 61 != 0)
    a = torch.full((n,), 7.0)
    a[kind_b], a[kind_a] = 3.0, 2.5
    z = torch.zeros(1, 5, n)
    z[0, 0] = a
    z = z.view(1, 5, 64, 96).to(DEV).requires_grad_(True)
    y = torch.zeros(1, 64, 96, dtype=torch.int64, device=DEV)
    mod = OhemCrossEntropy(255, native=True)
    loss = mod(z, y)
    loss.backward()
    w = N.train_words_dict(mod.last_words)
    n_a, n_min = int(kind_a.sum()), n // 16
    take = n_min - n_a
    assert 1 < take < int(kind_b.sum()), (take, int(kind_b.sum()))
    assert w["mode"] == 1 and w["n_min"] == n_min and w["n_sel"] == n_min and w["take"] == take, w
    want = kind_a.clone()
    want[idx[kind_b][:take]] = True
    assert idx[kind_b][take - 1] > 2 * 2048        # the taken ties span all three blocks of the select
    touched = (z.grad != 0).any(1).view(-1).cpu()
    assert torch.equal(touched, want)
    la, lb = math.log1p(4 * math.exp(-2.5)), math.log1p(4 * math.exp(-3.0))
    assert abs(float(loss.detach()) - (n_a * la + take * lb) / n_min) <= 2 * ulp32(la)
    assert abs(w["t"] - lb) <= ulp32(lb)


def synthetic(C, B=8, S=512, seed=0, confident=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    y = torch.randint(0, C, (B, S, S), generator=g, device=DEV)
    z = torch.randn(B, C, S, S, generator=g, device=DEV) * 3
    frac, boost = (0.995, 12.0 + 2.5 * math.log(C)) if confident else (0.7, 6.0)
    z.scatter_add_(1, y[:, None], ((torch.rand(B, S, S, generator=g, device=DEV) < frac).float() * boost)[:, None])
    y[torch.rand(B, S, S, generator=g, device=DEV) < 0.05] = -1
    return z, y


@pytest.mark.parametrize("C", [21, 151])
@pytest.mark.parametrize("kind", ["ce", "ohem"])
def test_training_size_reproducible_zero_at_ignored_and_tuple(C, kind):
    from semseg.losses import CrossEntropy, OhemCrossEntropy
    z, y = synthetic(C)
    w = (0.5 + torch.rand(C, generator=torch.Generator().manual_seed(1))).to(DEV)
    mod = (CrossEntropy if kind == "ce" else OhemCrossEntropy)(-1, w, native=True).to(DEV)

    def single(logits, scale=None):
        leaf = logits.detach().requires_grad_(True)
        loss = mod(leaf, y)
        (loss if scale is None else scale * loss).backward()
        return loss.detach(), leaf.grad

    l1, g1 = single(z)
    l2, g2 = single(z)
    assert torch.isfinite(l1) and torch.equal(l1, l2) and torch.equal(g1, g2)
    assert bool((g1.movedim(1, -1)[y == -1] == 0).all())
    assert bool((g1 != 0).any())
    del g2
    # tuple input: the weighted sum of single calls, bit for bit
    del l2
    z2 = (z * 0.5).contiguous()
    a0, a1 = mod.aux_weights[:2]
    la, ga = single(z, a0)
    lb, gb = single(z2, a1)
    leaves = (z.detach().requires_grad_(True), z2.detach().requires_grad_(True))
    lt = mod(leaves, y)
    lt.backward()
    assert torch.equal(lt.detach(), a0 * la + a1 * lb)
    assert torch.equal(leaves[0].grad, ga) and torch.equal(leaves[1].grad, gb)


def test_ohem_topk_at_the_training_size():
    """top-k regime at 8 x 512 x 512 (1024 select blocks of 2048 pixels): regime, count, the stock criterion's value."""
    from semseg import _native as N
    from semseg.losses import OhemCrossEntropy
    z, y = synthetic(21, confident=True)
    mod = OhemCrossEntropy(-1, native=True)
    leaf = z.detach().requires_grad_(True)
    loss = mod(leaf, y)
    loss.backward()
    w = N.train_words_dict(mod.last_words)
    assert w["mode"] == 1 and w["n_sel"] == w["n_min"] == int((y != -1).sum()) // 16, w
    assert int((leaf.grad != 0).any(1).sum()) == w["n_sel"]
    stock = OhemCrossEntropy(-1)(z, y)
    print(f"[T2 top-k 8x21x512x512] loss T2 {float(loss):.9g} stock {float(stock):.9g} words {w}")
    torch.testing.assert_close(loss, stock, rtol=1e-5, atol=0)
    leaf2 = z.detach().requires_grad_(True)
    loss2 = mod(leaf2, y)
    loss2.backward()
    assert torch.equal(loss, loss2) and torch.equal(leaf.grad, leaf2.grad)


def test_strided_logits_are_refused_channels_last_goes_to_torch():
    from semseg import _native as N
    from semseg.losses import CrossEntropy
    z, y = synthetic(5, B=2, S=16)
    mod = CrossEntropy(-1, native=True)
    with pytest.raises(N.SeaNativeError):
        mod(z[:, :, :, ::2], y[:, :, ::2].contiguous())
    cl = z.contiguous(memory_format=torch.channels_last)
    torch.testing.assert_close(mod(cl, y), mod(z, y), rtol=1e-5, atol=0)


def test_ohem_topk_forward_backward_in_a_captured_graph():
    """No host synchronisation: the whole step is captured and replayed on new logits written into the same buffer."""
    from semseg import _native as N
    from semseg.losses import OhemCrossEntropy
    C = 21
    z0, y = synthetic(C, B=2, S=128, seed=5, confident=True)
    z1, _ = synthetic(C, B=2, S=128, seed=5, confident=True)
    z1 = (z1 + 0.25 * torch.randn(z1.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))).contiguous()
    mod = OhemCrossEntropy(-1, native=True).to(DEV)
    static = z0.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(mod(static, y), static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_c = mod(static, y)
        grad_c, = torch.autograd.grad(loss_c, static)
        words_c = mod.last_words
    with torch.no_grad():
        static.copy_(z1)
    graph.replay()
    torch.cuda.synchronize()
    w = N.train_words_dict(words_c)
    assert w["mode"] == 1 and w["n_sel"] == w["n_min"] > 0, w
    leaf = z1.clone().requires_grad_(True)
    loss_e = mod(leaf, y)
    grad_e, = torch.autograd.grad(loss_e, leaf)
    assert N.train_words_dict(mod.last_words)["mode"] == 1
    assert torch.isfinite(loss_e) and torch.equal(loss_c, loss_e.detach()) and torch.equal(grad_c, grad_e)
    leaf0 = z0.clone().requires_grad_(True)
    assert not torch.equal(mod(leaf0, y).detach(), loss_e.detach())   # the replay did see the new logits
