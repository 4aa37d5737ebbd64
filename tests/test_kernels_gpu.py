"""Parity of the HIP kernels (through the C ABI of libsea_hip.so) with the CPU oracle and with the
golden vectors generated from the reference.  Needs a real MI355X: run with `-m gpu`.

Bars: integer / index / byte results bit-exact; element-wise L-inf arithmetic bit-exact; float
losses within 1e-4 (the tolerance of BASELINE.json's north_star), asserted tighter where the
arithmetic allows.
"""
import pytest
import torch

from conftest import load_golden
from oracle import sea_oracle as O

pytestmark = pytest.mark.gpu

LOSS_ATOL = 1e-4  # north_star tolerance on float losses


@pytest.fixture(scope="module")
def N():
    from semseg import _native
    _native.lib()  # raises if the extension is missing: no silent fallback
    return _native


def dev(t):
    return t.cuda() if isinstance(t, torch.Tensor) else t


# ------------------------------------------------------------------------------------------------ K1/K5/K6
def test_linf_kernels_golden_bit_exact(N):
    g = load_golden("g2_linf")
    for ci in range(5):
        p = lambda k: g[f"c{ci}_{k}"]  # noqa: E731
        out = N.apgd_linf_step(dev(p("x")), dev(p("x_adv")), dev(p("x_old")), dev(p("grad")), dev(p("step")),
                               p("eps"), p("a"))
        assert torch.equal(out.cpu(), p("out"))
        assert torch.equal(N.linf_random_start(dev(p("x")), dev(p("u")), p("eps")).cpu(), p("rs"))
        assert torch.equal(N.linf_project(dev(p("zz")), dev(p("x")), p("eps")).cpu(), p("proj"))
        d = N.pgd_linf_step(dev(p("x")), dev(p("delta")), dev(p("grad")), p("alpha"), p("eps"))
        assert torch.equal(d.cpu(), p("delta_out"))


@pytest.mark.parametrize("shape", [(2, 3, 16, 16), (3, 3, 33, 31), (1, 3, 7, 5), (8, 3, 512, 512)])
def test_linf_kernels_vs_oracle(N, shape):
    g = torch.Generator().manual_seed(sum(shape))
    eps, a = 8.0 / 255, 0.75
    x = torch.rand(shape, generator=g)
    x_old = (x + eps * (2 * torch.rand(shape, generator=g) - 1)).clamp(0, 1)
    x_adv = (x + eps * (2 * torch.rand(shape, generator=g) - 1)).clamp(0, 1)
    grad = torch.randn(shape, generator=g)
    grad[torch.rand(shape, generator=g) < 0.1] = 0
    step = 2 * eps / (2.0 ** torch.arange(shape[0]).float())
    ref = O.apgd_linf_step(x, x_adv, x_old, grad, step, eps, a)
    out = N.apgd_linf_step(dev(x), dev(x_adv), dev(x_old), dev(grad), dev(step), eps, a)
    assert torch.equal(out.cpu(), ref)
    # properties that hold at any size: inside the eps-ball and the image box
    assert (out.cpu() - x).abs().max() <= eps + 1e-7 and out.min() >= 0 and out.max() <= 1
    u = torch.rand(shape, generator=g)
    assert torch.equal(N.linf_random_start(dev(x), dev(u), eps).cpu(), O.linf_random_start(x, u, eps))
    z = x + (x_adv - x) * 2.5
    pr = N.linf_project(dev(z), dev(x), eps)
    assert torch.equal(pr.cpu(), O.linf_project(z, x, eps))
    assert torch.equal(N.linf_project(pr, dev(x), eps), pr)  # idempotent
    delta = (torch.rand(shape, generator=g) * 2 - 1) * eps
    xin = torch.empty(shape, device="cuda")
    d = N.pgd_linf_step(dev(x), dev(delta), dev(grad), 1e-2, eps, x_in_out=xin, clamp_input=False)
    dref = O.pgd_linf_step(x, delta, grad, 1e-2, eps)
    assert torch.equal(d.cpu(), dref) and torch.equal(xin.cpu(), x + dref)


@pytest.mark.parametrize("hw", [(9, 7), (8, 8)])     # 3*H*W odd: one float per lane; a multiple of four: float4
def test_replayable_k1_k7_with_scalar_arguments_and_with_device_words_agree(N, hw):
    """K1 / K7 come in two forms: the reference-shaped one with host scalars (sea_apgd_linf_step writes a third buffer and the
    caller rotates; sea_apgd_track takes iter, n_iter and check_k as arguments) and the replayable one that the attack loop
    runs (sea_apgd_linf_step_graph updates x_adv / x_old in place; sea_apgd_track_graph reads radius, run length, loop index
    and checkpoint table from device memory, its tables sized for the longest run replayed).  The same seeded buffers go
    through both for five iterations of a 12-step schedule -- a = 1 at iteration 0, the window-2 checkpoint at iteration 1
    with one image that halves its step and restarts and one that does not -- and every buffer (x_adv / x_old by role, not
    by address) and every state field is bit-identical after every iteration."""
    from semseg import attacker as A
    (H, W), B, n_iter, cap, eps, steps = hw, 3, 12, 16, 8.0 / 255, 5
    HW = H * W
    cps = A.apgd_checkpoints(n_iter)
    assert cps[1] == 2 and 0 not in cps
    g = torch.Generator().manual_seed(41 + W)
    x = torch.rand(B, 3, H, W, generator=g)
    x0 = (x + eps * (2 * torch.rand(x.shape, generator=g) - 1)).clamp(0, 1)
    grads = [torch.randn(x.shape, generator=g) for _ in range(steps + 1)]
    preds = [torch.randint(0, 21, (B, H, W), generator=g).to(torch.uint8) for _ in range(steps + 1)]
    # tracking-loss sums per image: image 0 rises (no halving at the checkpoint), image 1 falls (halved, restart), image 2 random
    tracks = [torch.tensor([10.0 + i, 10.0 - i, 20.0 * float(torch.rand(1, generator=g))]) for i in range(steps + 1)]
    corr = [torch.randint(0, HW - 4, (B,), generator=g).to(torch.int32) for _ in range(steps + 1)]
    n_ign = torch.tensor([0, 3, 4], dtype=torch.int32).cuda()

    def drive(device_words):
        rows = cap if device_words else n_iter
        st = A.ApgdState(B, rows, eps, "cuda")
        b = dict(x_adv=x0.cuda(), x_old=x0.cuda(), grad=grads[0].cuda(), x_best=x0.cuda(), x_best_adv=x0.cuda(),
                 grad_best=grads[0].cuda(), pred=preds[0].cuda(), pred_best=preds[0].cuda())
        if device_words:
            b["it_dev"] = torch.zeros(1, dtype=torch.int32, device="cuda")
        stats = lambda i: dict(loss_sum=tracks[i].cuda(), track_sum=tracks[i].cuda(), n_correct=corr[i].cuda())  # noqa: E731
        N.apgd_track(stats(0), n_ign, HW, 0, n_iter, 0, True, True, st)       # step 0 of a run
        tab = torch.zeros(rows, dtype=torch.int32)
        for k, v in cps.items():
            tab[k] = v
        tab, xd = tab.cuda(), x.cuda()
        eps_dev = torch.full((1,), eps, dtype=torch.float32, device="cuda")
        n_dev = torch.full((1,), n_iter, dtype=torch.int32, device="cuda")
        x_next = torch.empty_like(xd)                                       # (a): the third iterate buffer
        snaps = []
        for i in range(steps):
            if device_words:
                N.apgd_linf_step_graph(xd, b["x_adv"], b["x_old"], b["grad"], st.step, eps_dev, b["it_dev"])
            else:
                N.apgd_linf_step(xd, b["x_adv"], b["x_old"], b["grad"], st.step, eps, 0.75 if i > 0 else 1.0, out=x_next)
                b["x_old"], b["x_adv"], x_next = b["x_adv"], x_next, b["x_old"]
            b["grad"].copy_(grads[i + 1])                                   # (what the model's backward would leave)
            b["pred"].copy_(preds[i + 1])
            if device_words:
                N.apgd_track_graph(stats(i + 1), n_ign, HW, b["it_dev"], tab, n_dev, True, st)
            else:
                N.apgd_track(stats(i + 1), n_ign, HW, i, n_iter, cps.get(i, 0), True, False, st)
            N.select_copy(st.flags, b["x_adv"], b["grad"], b["x_best"], b["grad_best"], b["x_best_adv"], b["pred"], b["pred_best"])
            snap = {k: v.clone() for k, v in b.items()}
            snap.update({k: getattr(st, k).clone() for k in ("acc_cnt", "acc", "loss_best", "loss_best_last", "reduced_last",
                                                             "step", "flags", "done")})
            snap["loss_steps"] = st.loss_steps[:n_iter].clone()
            snaps.append(snap)
        return snaps

    scalar, words = drive(False), drive(True)
    for i, (s, d) in enumerate(zip(scalar, words)):
        assert set(d) == set(s) | {"it_dev"}
        for k in s:
            assert torch.equal(s[k], d[k]), (i, k)
    last = words[-1]
    assert int(last["it_dev"]) == steps and not torch.equal(last["x_adv"], x0.cuda())
    assert last["step"][1] < last["step"][0] == words[0]["step"][0]           # image 1 was halved, image 0 never


# ------------------------------------------------------------------------------------------------ K2
MODES = (("mask_ce_avg", 0), ("mask_ce_bal", 1), ("js_avg", 2), ("ce", 3))


@pytest.mark.parametrize("C", [5, 21, 151])
def test_loss_kernel_golden(N, C):
    g = load_golden(f"g1_losses_C{C}")
    logits, y, w = dev(g["logits"]), dev(g["y"]), dev(g["w"])
    B, _, H, W = logits.shape
    HW = H * W
    for key, mode in MODES:
        pred = torch.empty(B, H, W, dtype=torch.int64, device="cuda")
        lpx = torch.empty(B, H, W, device="cuda")
        r = N.loss_fwd_bwd(logits, y, w, mode, 3, 1.0 / HW, want_grad=True, pred=pred, loss_px=lpx)
        torch.cuda.synchronize()
        assert torch.equal(pred.cpu(), g["pred"])                                   # argmax: bit-exact
        torch.testing.assert_close(lpx.cpu(), g[key + "_px"], rtol=2e-5, atol=2e-6)
        torch.testing.assert_close((r["loss_sum"] / HW).cpu(), g[key + "_img"], rtol=2e-5, atol=LOSS_ATOL * 1e-2)
        torch.testing.assert_close((r["track_sum"] / HW).cpu(), g["ce_img"], rtol=2e-5, atol=LOSS_ATOL * 1e-2)
        torch.testing.assert_close(r["dlogits"].cpu(), g[key + "_grad"], rtol=1e-4, atol=2e-8)
        n_ign = (g["y"] == -1).view(B, -1).sum(-1)
        assert torch.equal(r["n_correct"].cpu().long().float() / HW, g["acc_step0"])
        assert torch.equal((r["n_correct"].cpu().long() + n_ign).float() / HW, g["acc_loop"])


def test_argmax_first_maximum(N):
    g = load_golden("g1_argmax_ties")
    z = dev(g["z"]).view(3, 4, 1, 1).contiguous()
    y = torch.zeros(3, 1, 1, dtype=torch.int64, device="cuda")
    pred = torch.empty(3, 1, 1, dtype=torch.int64, device="cuda")
    N.loss_fwd_bwd(z, y, None, 3, 3, 1.0, want_grad=False, pred=pred)
    assert torch.equal(pred.view(3).cpu(), g["arg"])


def _rand_case(B, C, H, W, seed, ignore=0.05):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, H, W, generator=g) * 3
    y = torch.randint(0, C, (B, H, W), generator=g)
    boost = (torch.rand(B, H, W, generator=g) < 0.7).float() * 6
    logits.scatter_add_(1, y.unsqueeze(1), boost.unsqueeze(1))
    # exact ties between two classes on some pixels exercise the tie-break
    tie = torch.rand(B, H, W, generator=g) < 0.02
    logits[:, 1][tie] = logits[:, 0][tie]
    y[torch.rand(B, H, W, generator=g) < ignore] = -1
    w = torch.rand(C, generator=g) + 0.01
    return logits, y, w


def _check_against_oracle(N, logits, y, w, mode, tmode, dl=None, **kw):
    B, C, H, W = logits.shape
    HW = H * W
    ref = O.loss_fwd_bwd(logits.float(), y, w, mode, tmode, with_grad=True)
    ld = dev(logits)
    if kw.pop("channels_last", False):
        ld = ld.contiguous(memory_format=torch.channels_last)
    yd = kw.pop("y_dev", None)
    yd = dev(y) if yd is None else yd
    pred = torch.empty(B, H, W, dtype=kw.pop("pred_dtype", torch.int64), device="cuda")
    r = N.loss_fwd_bwd(ld, yd, dev(w), mode, tmode, 1.0 / HW, want_grad=True, pred=pred, **kw)
    torch.cuda.synchronize()
    assert torch.equal(pred.cpu().long(), ref["pred"])
    assert torch.equal(r["n_correct"].cpu().long(), ref["n_correct"])
    torch.testing.assert_close((r["loss_sum"] / HW).cpu(), ref["loss_img"], rtol=3e-5, atol=LOSS_ATOL * 1e-2)
    torch.testing.assert_close((r["track_sum"] / HW).cpu(), ref["track_img"], rtol=3e-5, atol=LOSS_ATOL * 1e-2)
    got = r["dlogits"]
    assert got.stride() == ld.stride()
    tol = dict(rtol=1e-4, atol=2e-8 + 1e-6 / HW) if logits.dtype == torch.float32 else dict(rtol=2e-2, atol=1e-2 / HW)
    torch.testing.assert_close(got.float().cpu(), ref["dlogits"], **tol)
    return r


@pytest.mark.parametrize("C", [2, 5, 19, 21, 27, 60, 100, 150, 151, 171, 200])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_loss_kernel_class_counts_sweep(N, C, mode):
    """every register-kernel instantiation (exact-C and padded) and the streaming fallback (C=200)"""
    logits, y, w = _rand_case(2, C, 16, 24, seed=C * 7 + mode)
    _check_against_oracle(N, logits, y, w, mode, 3)


@pytest.mark.parametrize("hw", [(16, 16), (33, 31), (17, 18), (1, 5), (64, 48)])
@pytest.mark.parametrize("vec", [0, 1, 2, 4])
def test_loss_kernel_shapes_and_vector_widths(N, hw, vec):
    """odd H*W (473x473-like, no 16-byte alignment of the class planes) and forced pixels-per-lane"""
    logits, y, w = _rand_case(3, 21, hw[0], hw[1], seed=hw[0] * 100 + hw[1])
    _check_against_oracle(N, logits, y, w, 1, 3, force_vec=vec)


@pytest.mark.parametrize("C", [21, 151])
def test_loss_kernel_channels_last_and_label_types(N, C):
    logits, y, w = _rand_case(2, C, 16, 16, seed=C)
    _check_against_oracle(N, logits, y, w, 0, 3, channels_last=True)
    y8 = torch.where(y < 0, torch.full_like(y, 255), y).to(torch.uint8)
    _check_against_oracle(N, logits, y, w, 2, 3, y_dev=dev(y8), pred_dtype=torch.uint8)
    _check_against_oracle(N, logits, y, w, 1, 1, y_dev=dev(y.to(torch.int16)), pred_dtype=torch.int16)
    _check_against_oracle(N, logits, y, w, 3, 3, y_dev=dev(y.to(torch.int32)), pred_dtype=torch.int32)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_loss_kernel_half_precision_logits(N, dtype):
    logits, y, w = _rand_case(2, 21, 16, 16, seed=3)
    logits = logits.to(dtype)
    _check_against_oracle(N, logits, y, w, 0, 3)
    _check_against_oracle(N, logits, y, w, 2, 3)


def test_loss_kernel_no_grad_variant_and_determinism(N):
    logits, y, w = _rand_case(4, 21, 64, 64, seed=11)
    a = N.loss_fwd_bwd(dev(logits), dev(y), dev(w), 1, 3, 1.0 / 4096, want_grad=False)
    b = N.loss_fwd_bwd(dev(logits), dev(y), dev(w), 1, 3, 1.0 / 4096, want_grad=True)
    assert a["dlogits"] is None
    # the no-gradient pass is a different kernel (streaming online soft-max): same integers, float sums to rounding
    assert torch.equal(a["n_correct"], b["n_correct"])
    for k in ("loss_sum", "track_sum"):
        torch.testing.assert_close(a[k], b[k], rtol=2e-6, atol=0)
    a2 = N.loss_fwd_bwd(dev(logits), dev(y), dev(w), 1, 3, 1.0 / 4096, want_grad=False)
    assert all(torch.equal(a[k], a2[k]) for k in ("loss_sum", "track_sum", "n_correct"))   # run-to-run deterministic
    c = N.loss_fwd_bwd(dev(logits), dev(y), dev(w), 1, 3, 1.0 / 4096, want_grad=True)
    assert torch.equal(b["dlogits"], c["dlogits"]) and torch.equal(b["loss_sum"], c["loss_sum"])


def test_loss_kernel_js_is_nan_free_on_underflow(N):
    """softmax underflow makes the reference's JS NaN; the closed form stays finite."""
    z = torch.zeros(1, 5, 2, 2)
    z[:, 0] = 200.0
    y = torch.tensor([[[0, 1], [2, -1]]])
    r = N.loss_fwd_bwd(dev(z), dev(y), None, 2, 2, 0.25, want_grad=True)
    assert torch.isfinite(r["loss_sum"]).all() and torch.isfinite(r["dlogits"]).all()
    assert r["loss_sum"].item() == pytest.approx(2 * 0.6931471805599453, rel=1e-5)


def test_loss_kernel_full_size_voc_batch(N):
    """BASELINE size B=8, C=21, 512x512 against the oracle, plus size-independent properties."""
    B, C, H, W = 8, 21, 512, 512
    logits, y, w = _rand_case(B, C, H, W, seed=2024)
    r = _check_against_oracle(N, logits, y, w, 0, 3)
    # softmax-gradient rows sum to zero per pixel; masked-out pixels have exactly zero gradient
    dl = r["dlogits"]
    assert dl.sum(1).abs().max().item() < 1e-9
    masked = dev((O.argmax_first(logits) != y) | (y == -1))
    assert (dl.abs().sum(1)[masked] == 0).all()
    assert int(r["n_correct"].sum()) == int(((O.argmax_first(logits) == y)).sum())


def test_differentiable_loss_wrappers(N):
    """semseg.attacker's reduction='none' functions + autograd == the reference's (golden G1)."""
    from semseg import attacker as A
    g = load_golden("g1_losses_C21")
    y, w = dev(g["y"]), dev(g["w"])
    mask_bg = (y != -1).float()
    for name, key in (("mask-ce-avg", "mask_ce_avg"), ("mask-ce-bal", "mask_ce_bal"), ("js-avg", "js_avg"), ("ce-avg", "ce")):
        z = dev(g["logits"]).clone().requires_grad_(True)
        lp = A.criterion_dict[name](z, y, w)
        li = A.pixel_to_img_loss(lp, mask_bg)
        (gr,) = torch.autograd.grad(li.sum(), [z])
        torch.testing.assert_close(lp.detach().cpu(), g[key + "_px"], rtol=2e-5, atol=2e-6)
        torch.testing.assert_close(li.detach().cpu(), g[key + "_img"], rtol=2e-5, atol=1e-6)
        torch.testing.assert_close(gr.cpu(), g[key + "_grad"], rtol=1e-4, atol=2e-8)


# ------------------------------------------------------------------------------------------------ K3
@pytest.mark.parametrize("C", [5, 21])
def test_counts_and_confusion_golden(N, C):
    g = load_golden(f"g3_counts_C{C}")
    pred, y = dev(g["pred"]), dev(g["y"])
    hist = N.confusion(pred, y, C)
    assert torch.equal(hist.cpu().float(), g["hist"])
    inter, pc, tc = N.class_counts(pred, y, C, per_image=False, mask_pred=True)
    h = hist.cpu()
    assert torch.equal(inter.cpu(), h.diag()) and torch.equal(tc.cpu(), h.sum(1)) and torch.equal(pc.cpu(), h.sum(0))
    from semseg import attacker as A
    p2 = pred.clone()
    m_acc, a_acc, m_iou = A.compute_iou_acc(p2, y, C)
    assert torch.equal(p2.cpu(), g["pred_after"])
    assert m_acc.item() == pytest.approx(g["m_acc"], rel=1e-6)
    assert a_acc.item() == pytest.approx(g["a_acc"], rel=1e-6)
    assert m_iou.item() == pytest.approx(g["m_iou"], rel=1e-6)
    from semseg.metrics import Metrics
    met = Metrics(C, -1, "cuda")
    met.update(torch.nn.functional.one_hot(g["pred"], C).permute(0, 3, 1, 2).float().cuda(), y)
    assert torch.equal(met.hist.cpu(), g["hist"])
    ious, miou = met.compute_iou()
    acc, macc, aacc = met.compute_pixel_acc()
    f1, mf1 = met.compute_f1()
    assert miou == g["miou"] and macc == g["macc"] and mf1 == g["mf1"]


@pytest.mark.parametrize("C,shape,dt", [(151, (3, 40, 52), torch.int64), (21, (8, 512, 512), torch.uint8),
                                        (300, (2, 16, 16), torch.int16)])
def test_counts_vs_oracle(N, C, shape, dt):
    g = torch.Generator().manual_seed(C)
    pred = torch.randint(0, C, shape, generator=g)
    y = torch.randint(0, C, shape, generator=g)
    m = torch.rand(shape, generator=g) < 0.6
    y[m] = pred[m]
    y[torch.rand(shape, generator=g) < 0.05] = -1
    conv = (lambda t: torch.where(t < 0, torch.full_like(t, 255), t).to(dt)) if dt == torch.uint8 else (lambda t: t.to(dt))
    for per_image in (False, True):
        for mask_pred in (False, True):
            ref = O.class_counts(pred, y, C, per_image=per_image, mask_pred=mask_pred)
            got = N.class_counts(dev(conv(pred)), dev(conv(y)), C, per_image=per_image, mask_pred=mask_pred)
            for a, b in zip(got, ref):
                assert torch.equal(a.cpu(), b)
    assert torch.equal(N.confusion(dev(conv(pred)), dev(conv(y)), C).cpu(), O.confusion_matrix(pred, y, C))
    # size-independent: every valid pixel is counted exactly once; accumulation is additive
    out = N.class_counts(dev(conv(pred)), dev(conv(y)), C)
    assert int(out[2].sum()) == int((y >= 0).sum())
    N.class_counts(dev(conv(pred)), dev(conv(y)), C, out=out)
    assert int(out[2].sum()) == 2 * int((y >= 0).sum())
    assert torch.equal(N.count_ignored(dev(conv(y))).cpu().long(), (y == -1).view(shape[0], -1).sum(-1))


# ------------------------------------------------------------------------------------------------ M1
@pytest.mark.parametrize("shape", [(2, 96, 128, 128), (1, 8, 16, 16), (3, 5, 33, 47), (2, 768, 16, 16), (1, 3, 70, 9)])
def test_dwconv7x7_forward_and_backward_data(N, shape):
    """model-side stencil kernel vs a float64 CPU convolution (fwd incl. bias, and backward-data)"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(shape[1])
    B, C, H, W = shape
    x = torch.randn(shape, generator=g)
    w = torch.randn(C, 1, 7, 7, generator=g) * 0.1
    b = torch.randn(C, generator=g)
    xd = x.double().requires_grad_(True)
    ref = F.conv2d(xd, w.double(), b.double(), padding=3, groups=C)
    gy = torch.randn(ref.shape, generator=g)
    (gx_ref,) = torch.autograd.grad(ref, xd, gy.double())
    y = N.dwconv7x7(dev(x), dev(w), dev(b))
    torch.testing.assert_close(y.cpu().double(), ref.detach(), rtol=1e-5, atol=1e-5)
    gx = N.dwconv7x7(dev(gy), dev(w), None, flip=True)
    torch.testing.assert_close(gx.cpu().double(), gx_ref, rtol=1e-5, atol=1e-5)


def test_convnext_block_uses_stencil_kernel_and_matches_miopen(N):
    from semseg.models import convnext_upernet as M
    torch.manual_seed(0)
    blk = M.Block(96).cuda().eval()
    x = torch.randn(2, 96, 64, 64, device="cuda")
    outs = []
    for flag in (True, False):
        M.USE_HIP_DWCONV = flag
        xi = x.clone().requires_grad_(True)
        y = blk(xi)
        (gx,) = torch.autograd.grad(y, xi, torch.ones_like(y))
        outs.append((y.detach(), gx))
    M.USE_HIP_DWCONV = True
    torch.testing.assert_close(outs[0][0], outs[1][0], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(outs[0][1], outs[1][1], rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------------ K2u
@pytest.mark.parametrize("case", [
    (2, 21, 16, 16, 64, 64),      # x4, UperNet-like
    (2, 5, 8, 8, 128, 128),       # x16, Segmenter-like
    (1, 21, 30, 30, 119, 119),    # non-integer scale (473x473 crops give 119 -> 473)
    (2, 151, 12, 20, 48, 80),     # many classes, non-square
    (1, 3, 7, 5, 7, 5),           # scale 1
    (3, 21, 13, 11, 50, 45),      # ragged tiles + non-integer scales
    (2, 151, 8, 12, 32, 48),      # x4, three class slots of the power-of-two kernel (lanes = classes), non-square
    (1, 65, 6, 7, 24, 28),        # x4, two slots, one class in the second
    (2, 128, 3, 5, 48, 80),       # x16, two full slots, segments of two cells with a ragged last one
    (1, 192, 2, 2, 8, 8),         # x4, the smallest map the power-of-two kernel takes, 192 classes
])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_fused_upsample_loss_kernel(N, case, mode):
    B, C, h, w, H, W = case
    g = torch.Generator().manual_seed(h * 1000 + H + mode)
    low = torch.randn(B, C, h, w, generator=g) * 3
    hi_ref = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    y = hi_ref.max(1)[1]
    flip = torch.rand(B, H, W, generator=g) < 0.3
    y[flip] = torch.randint(0, C, (int(flip.sum()),), generator=g)
    y[torch.rand(B, H, W, generator=g) < 0.05] = -1
    wts = torch.rand(C, generator=g) + 0.01
    ref = O.loss_fwd_bwd_upsampled(low, y, wts, mode, 3, with_grad=True)
    pred = torch.empty(B, H, W, dtype=torch.int64, device="cuda")
    r = N.loss_fwd_bwd_upsampled(dev(low), dev(y), dev(wts), mode, 3, 1.0 / (H * W), want_grad=True, pred=pred)
    torch.cuda.synchronize()
    # argmax / counts: exact wherever the top-2 margin of the interpolated logits exceeds float noise
    top2 = ref["logits_hi"].topk(2, dim=1)[0]
    safe = (top2[:, 0] - top2[:, 1]) > 1e-4
    assert torch.equal(pred.cpu()[safe], ref["pred"][safe])
    n_unsafe = (~safe).view(B, -1).sum(-1)
    assert ((r["n_correct"].cpu().long() - ref["n_correct"]).abs() <= n_unsafe).all()
    if int(n_unsafe.sum()) == 0:
        assert torch.equal(r["n_correct"].cpu().long(), ref["n_correct"])
    torch.testing.assert_close((r["loss_sum"] / (H * W)).cpu(), ref["loss_img"], rtol=1e-4, atol=LOSS_ATOL)
    torch.testing.assert_close((r["track_sum"] / (H * W)).cpu(), ref["track_img"], rtol=1e-4, atol=LOSS_ATOL)
    scale = ref["dlow"].abs().max().item()
    torch.testing.assert_close(r["dlogits"].cpu(), ref["dlow"], rtol=2e-3, atol=2e-4 * scale + 1e-9)
    # determinism (gather formulation, no atomics)
    r2 = N.loss_fwd_bwd_upsampled(dev(low), dev(y), dev(wts), mode, 3, 1.0 / (H * W), want_grad=True)
    assert torch.equal(r["dlogits"], r2["dlogits"]) and torch.equal(r["loss_sum"], r2["loss_sum"])


def test_fused_and_unfused_attack_agree(N):
    """ApgdRun with K2u (low-res logits + fused upsample) vs K2 on the upsampled logits, same model"""
    from semseg import attacker as A

    class LowResNet(torch.nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(3)
            self.c = torch.nn.Conv2d(3, 7, 3, stride=4, padding=1)

        def forward_lowres(self, x):
            return 4.0 * self.c(x), tuple(x.shape[2:])

        def forward(self, x):
            low, size = self.forward_lowres(x)
            return torch.nn.functional.interpolate(low, size=size, mode="bilinear", align_corners=False)

    net = LowResNet().cuda().eval()
    g = torch.Generator().manual_seed(9)
    x = torch.rand(2, 3, 64, 64, generator=g).cuda()
    with torch.no_grad():
        y = net(x).max(1)[1]
    outs = []
    shipped = A.FUSE_UPSAMPLE          # ("auto" since round 6: restored below -- a leaked False changes every later in-process run)
    try:
        for fuse in (True, False):
            A.FUSE_UPSAMPLE = fuse
            outs.append(A.apgd_train(net, x, y, "Linf", 8 / 255, n_iter=8, loss="mask-ce-avg", track_loss="ce-avg",
                                     num_classes=7))
    finally:
        A.FUSE_UPSAMPLE = shipped
    (xb, acc, lb, xba), (xb2, acc2, lb2, xba2) = outs
    assert (acc - acc2).abs().max() <= 3.0 / 4096
    torch.testing.assert_close(lb, lb2, rtol=1e-3, atol=1e-4)
    assert ((xba - xba2).abs() > 1e-6).float().mean() < 0.03


# ------------------------------------------------------------------------------------------------ M2
@pytest.mark.parametrize("case", [(2, 8, 16, 16, 32, 32), (1, 4, 32, 32, 128, 128), (2, 3, 16, 16, 128, 128),
                                  (1, 5, 1, 1, 16, 16), (1, 5, 3, 3, 16, 16), (2, 2, 6, 6, 16, 16),
                                  (1, 7, 30, 30, 119, 119), (1, 2, 13, 11, 50, 45), (1, 1, 9, 7, 9, 7),
                                  # power-of-two factors take the specialised kernels: edges, 1-wide maps, x16
                                  (2, 3, 8, 8, 128, 128), (1, 2, 2, 3, 8, 12), (1, 3, 5, 1, 20, 4), (1, 2, 1, 6, 2, 12),
                                  (1, 2, 3, 2, 48, 32), (1, 3, 7, 5, 56, 40), (1, 2, 4, 8, 8, 32), (1, 2, 5, 3, 10, 6),
                                  # row-streaming backward (output width 128 ... 1024), ragged bands
                                  (1, 2, 5, 64, 20, 256), (1, 1, 3, 32, 48, 512), (1, 1, 7, 512, 14, 1024),
                                  (1, 2, 9, 16, 72, 128), (2, 2, 33, 128, 132, 512), (1, 1, 1, 32, 16, 512)])
def test_upsample_bilinear_forward_backward(N, case):
    import torch.nn.functional as F
    B, C, h, w, H, W = case
    g = torch.Generator().manual_seed(h * 100 + H)
    x = torch.randn(B, C, h, w, generator=g)
    xd = x.double().requires_grad_(True)
    ref = F.interpolate(xd, size=(H, W), mode="bilinear", align_corners=False)
    gy = torch.randn(B, C, H, W, generator=g)
    (gx_ref,) = torch.autograd.grad(ref, xd, gy.double())
    y = N.upsample_bilinear(dev(x), (H, W))
    # float32 source indices (ATen's rule) carry ~1e-6*src error in lambda for non-integer scales: compare
    # tightly with ATen's own float32 result and a little looser with the float64 one
    ref32 = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False)
    torch.testing.assert_close(y.cpu(), ref32, rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(y.cpu().double(), ref.detach(), rtol=1e-5, atol=2e-4)
    gx = N.upsample_bilinear_backward(dev(gy), (h, w))
    pow2 = H == W * h // w and H // h in (2, 4, 8, 16) and H % h == 0 and W % w == 0 and W // w == H // h
    torch.testing.assert_close(gx.cpu().double(), gx_ref, rtol=1e-5, atol=5e-5 if pow2 else 1e-3)
    assert torch.equal(gx, N.upsample_bilinear_backward(dev(gy), (h, w)))  # deterministic gather
    if pow2:  # exact dyadic weights: inf stays inf (no 0 * inf from masked window parts)
        gy2 = gy.clone()
        gy2[0, 0, 0, 0] = float("inf")
        gx2 = N.upsample_bilinear_backward(dev(gy2), (h, w)).cpu()
        assert torch.isinf(gx2[0, 0, 0, 0]) and not torch.isnan(gx2).any()


@pytest.mark.parametrize("case", [(2, 8, 16, 16, 32, 32), (1, 4, 32, 32, 128, 128), (2, 12, 16, 16, 128, 128),
                                  (1, 4, 1, 1, 16, 16), (1, 8, 3, 3, 16, 16), (2, 4, 6, 6, 16, 16),
                                  (1, 8, 30, 30, 119, 119), (1, 4, 13, 11, 50, 45), (1, 4, 9, 7, 9, 7),
                                  (2, 512, 4, 4, 8, 8),
                                  # the pyramid-pooling maps: block-per-coarse-pixel backward, ragged channel groups
                                  (2, 768, 1, 1, 16, 16), (2, 72, 3, 3, 16, 16), (1, 768, 6, 6, 16, 16), (1, 20, 5, 7, 23, 31),
                                  # power-of-two factors with edges everywhere (specialised NHWC kernels)
                                  (1, 4, 2, 3, 8, 12), (1, 8, 3, 2, 24, 16), (1, 4, 5, 1, 10, 2), (1, 4, 1, 5, 4, 20)])
def test_upsample_bilinear_channels_last(N, case):
    """The NHWC kernels must agree with the NCHW ones (same arithmetic) and with ATen."""
    import torch.nn.functional as F
    B, C, h, w, H, W = case
    g = torch.Generator().manual_seed(h * 100 + H + 1)
    x = torch.randn(B, C, h, w, generator=g)
    gy = torch.randn(B, C, H, W, generator=g)
    xd = x.double().requires_grad_(True)
    ref = F.interpolate(xd, size=(H, W), mode="bilinear", align_corners=False)
    (gx_ref,) = torch.autograd.grad(ref, xd, gy.double())
    xc = dev(x).contiguous(memory_format=torch.channels_last)
    gc = dev(gy).contiguous(memory_format=torch.channels_last)
    y = N.upsample_bilinear_cl(xc, (H, W))
    assert y.is_contiguous(memory_format=torch.channels_last) and y.shape == (B, C, H, W)
    ref32 = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False)
    torch.testing.assert_close(y.cpu(), ref32, rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(y, N.upsample_bilinear(dev(x), (H, W)), rtol=1e-6, atol=1e-6)
    gx = N.upsample_bilinear_backward_cl(gc, (h, w))
    assert gx.is_contiguous(memory_format=torch.channels_last) and gx.shape == (B, C, h, w)
    torch.testing.assert_close(gx.cpu().double(), gx_ref, rtol=1e-5, atol=1e-3)
    assert torch.equal(gx, N.upsample_bilinear_backward_cl(gc, (h, w)))
    if w > 1:
        with pytest.raises(N.SeaNativeError):
            N.upsample_bilinear_cl(dev(x), (H, W))  # NCHW tensor refused by the NHWC entry point
    # in-place into / out of a channel slice of a wider NHWC buffer, with the fused residual add
    wide = torch.full((B, C + 8, H, W), -7.0, device="cuda").contiguous(memory_format=torch.channels_last)
    res = dev(torch.randn(B, C, H, W, generator=g)).contiguous(memory_format=torch.channels_last)
    N.upsample_bilinear_cl(xc, (H, W), out=wide[:, 4:4 + C], residual=res)
    torch.testing.assert_close(wide[:, 4:4 + C], y + res, rtol=1e-6, atol=1e-6)
    assert (wide[:, :4] == -7).all() and (wide[:, 4 + C:] == -7).all()
    gwide = torch.zeros(B, C + 8, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
    gwide[:, 4:4 + C] = gc
    assert torch.equal(N.upsample_bilinear_backward_cl(gwide[:, 4:4 + C], (h, w)), gx)


def test_upernet_head_fused_up_cat_and_up_add(N):
    """_up_cat / _up_add (NHWC, in-place slices) against torch.cat / + of ATen up-samplings, values and grads."""
    import torch.nn.functional as F
    from semseg.models import convnext_upernet as M
    g = torch.Generator().manual_seed(3)
    cl = torch.channels_last
    ts = [torch.randn(2, 8, 24, 20, generator=g), torch.randn(2, 12, 12, 10, generator=g),
          torch.randn(2, 4, 1, 1, generator=g), torch.randn(2, 8, 5, 7, generator=g)]
    res0 = torch.randn(2, 12, 24, 20, generator=g)

    def run(fused):
        M.USE_HIP_UPSAMPLE_NHWC = fused
        xs = [dev(t).contiguous(memory_format=cl).requires_grad_(True) for t in ts]
        res = dev(res0).contiguous(memory_format=cl).requires_grad_(True)
        cat = M._up_cat(xs, (24, 20))
        add = M._up_add(xs[1], res)
        loss = (cat * cat).sum() + (add * add * 0.5).sum()
        return cat.detach(), add.detach(), torch.autograd.grad(loss, xs + [res])

    try:
        c1, a1, g1 = run(True)
        c0, a0, g0 = run(False)
    finally:
        M.USE_HIP_UPSAMPLE_NHWC = True
    assert c1.is_contiguous(memory_format=cl)
    ref = torch.cat([ts[0]] + [F.interpolate(t, size=(24, 20), mode="bilinear", align_corners=False) for t in ts[1:]], 1)
    torch.testing.assert_close(c1.cpu(), ref, rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(c1, c0, rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(a1, a0, rtol=1e-5, atol=2e-5)
    for u, v in zip(g1, g0):
        torch.testing.assert_close(u, v, rtol=1e-4, atol=1e-4)


def test_upernet_head_with_and_without_hip_upsample(N):
    from semseg.models import convnext_upernet as M
    torch.manual_seed(0)
    model = M.UperNetForSemanticSegmentation("ConvNeXt-T_CVST", 21, None).cuda().eval()
    x = torch.rand(1, 3, 96, 128, device="cuda")
    outs = []
    for flag, nhwc in ((True, True), (True, False), (False, False)):
        M.USE_HIP_UPSAMPLE, M.USE_HIP_UPSAMPLE_NHWC = flag, nhwc
        xi = x.clone().requires_grad_(True)
        y = model(xi)
        (gx,) = torch.autograd.grad(y, xi, torch.ones_like(y))
        outs.append((y.detach(), gx))
    M.USE_HIP_UPSAMPLE = M.USE_HIP_UPSAMPLE_NHWC = True
    gmax = outs[2][1].abs().max().item()
    for k in (0, 1):
        assert outs[k][0].is_contiguous()  # NCHW logits for K2
        torch.testing.assert_close(outs[k][0], outs[2][0], rtol=1e-4, atol=1e-4)
        # ATen's backward sums with atomics, and last-bit differences flip a few ReLU gates: compare in norm
        assert (outs[k][1] - outs[2][1]).norm() <= 2e-3 * outs[2][1].norm()
        assert ((outs[k][1] - outs[2][1]).abs() > 1e-3 * gmax).float().mean() < 0.01


# ------------------------------------------------------------------------------------------------ M6
@pytest.mark.parametrize("case", [(2, 8, 12, 4, 4, 16, 16), (1, 16, 8, 3, 5, 24, 40), (2, 4, 4, 1, 1, 8, 8),
                                  (1, 8, 8, 5, 4, 17, 13), (1, 32, 64, 8, 8, 64, 64), (1, 8, 8, 2, 6, 8, 24),
                                  (2, 4, 8, 7, 1, 28, 4)])
def test_tap_gather_is_conv3x3_of_the_upsampled_input(N, case):
    """conv3x3(up(f)) == tap_gather(f @ W) (channel mixing commutes with bilinear interpolation), and the
    backward kernel is the exact adjoint."""
    import torch.nn.functional as F
    B, Cin, Cout, h, w, H, W = case
    g = torch.Generator().manual_seed(Cin + H)
    f = torch.randn(B, Cin, h, w, generator=g)
    wt = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
    gz = torch.randn(B, Cout, H, W, generator=g)
    cl = torch.channels_last
    fd = f.double().requires_grad_(True)
    ref = F.conv2d(F.interpolate(fd, size=(H, W), mode="bilinear", align_corners=False), wt.double(), padding=1)
    (gf_ref,) = torch.autograd.grad(ref, fd, gz.double())
    Wl = dev(wt).permute(2, 3, 0, 1).reshape(9 * Cout, Cin).contiguous()
    G = F.linear(dev(f).permute(0, 2, 3, 1).contiguous(), Wl).view(B, h, w, 9, Cout)
    extra = N.tap_gather(G, (H, W))
    assert extra.is_contiguous(memory_format=cl) or min(H, W) == 1
    torch.testing.assert_close(extra.cpu().double(), ref.detach(), rtol=2e-5, atol=2e-5)
    twice = N.tap_gather(G, (H, W), extra.clone())  # accumulate
    torch.testing.assert_close(twice, 2 * extra, rtol=1e-6, atol=1e-6)
    dG = N.tap_gather_backward(dev(gz).contiguous(memory_format=cl), (h, w))
    gf = torch.mm(dG.view(B * h * w, -1), Wl).view(B, h, w, Cin).permute(0, 3, 1, 2)
    torch.testing.assert_close(gf.cpu().double(), gf_ref, rtol=1e-4, atol=1e-4)
    # adjoint identity <tap_gather(G), gz> == <G, tap_gather_backward(gz)>
    lhs = (extra.double() * dev(gz).double()).sum().item()
    rhs = (G.double() * dG.double()).sum().item()
    assert abs(lhs - rhs) <= 1e-5 * max(1.0, abs(lhs))
    gate = torch.randn(B, Cout, H, W, generator=g)
    sc = torch.rand(Cout, generator=g) + 0.5
    out = N.gate_scale(dev(gz).contiguous(memory_format=cl), dev(gate).contiguous(memory_format=cl), dev(sc))
    torch.testing.assert_close(out.cpu(), torch.where(gate > 0, gz * sc[None, :, None, None], torch.zeros(())),
                               rtol=1e-6, atol=1e-6)


def test_fused_fpn_bottleneck_matches_the_reference_composition(N):
    """UperNet head with the coarse FPN inputs folded into coarse GEMMs + gather (M6) against the same head with
    Winograd off and M6 off (MIOpen + ATen composition): logits and input gradients."""
    from semseg.models import convnext_upernet as M
    torch.manual_seed(0)
    model = M.UperNetForSemanticSegmentation("ConvNeXt-T_CVST", 21, None).cuda().eval()
    for mod in model.modules():  # non-trivial BatchNorm statistics
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
    for p in model.parameters():
        p.requires_grad_(False)
    x = torch.rand(2, 3, 256, 192, device="cuda")
    outs, tile = [], M.WINOGRAD_TILE
    try:
        for fused, t in ((True, 4), (True, 2), (False, 4), (False, 0)):
            M.USE_FUSED_FPN_BOTTLENECK, M.WINOGRAD_TILE = fused, t
            xi = x.clone().requires_grad_(True)
            y = model(xi)
            assert (type(y.grad_fn).__name__ != "") and y.is_contiguous()
            (gx,) = torch.autograd.grad((y * y).sum(), xi)
            outs.append((y.detach(), gx))
            cache = getattr(model.decode_head.fpn_bottleneck, "_wino_cache", {})
            assert ("fpn_key" in cache) == fused or not fused  # the fused path really ran
            if not fused:
                cache.pop("fpn_key", None)
    finally:
        M.USE_FUSED_FPN_BOTTLENECK, M.WINOGRAD_TILE = True, tile
    ref_y, ref_g = outs[3]
    for k in range(3):
        assert (outs[k][0] - ref_y).abs().max() <= 2e-4 * ref_y.abs().max()
        assert (outs[k][1] - ref_g).norm() <= 2e-3 * ref_g.norm()


# ------------------------------------------------------------------------------------------------ M5
@pytest.mark.parametrize("shape", [(2, 16, 16, 48), (3, 7, 5, 96), (1, 9, 192), (5, 384), (2, 3, 768), (7, 4),
                                   (3, 1024), (11, 100), (1, 200, 300, 96)])
def test_layernorm_forward_and_input_gradient(N, shape):
    import torch.nn.functional as F
    C = shape[-1]
    g = torch.Generator().manual_seed(C + len(shape))
    x = torch.randn(shape, generator=g) * 2 + 0.5
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    gy = torch.randn(shape, generator=g)
    xd = x.double().requires_grad_(True)
    ref = F.layer_norm(xd, (C,), w.double(), b.double(), 1e-6)
    (gx_ref,) = torch.autograd.grad(ref, xd, gy.double())
    y, mean, rstd = N.layernorm(dev(x), dev(w), dev(b), 1e-6)
    torch.testing.assert_close(y.cpu().double(), ref.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(mean.cpu().double(), x.double().reshape(-1, C).mean(1), rtol=1e-5, atol=1e-6)
    dx = N.layernorm_backward(dev(gy), dev(x), dev(w), mean, rstd)
    torch.testing.assert_close(dx.cpu().double(), gx_ref, rtol=1e-4, atol=1e-5 * max(1.0, gx_ref.abs().max().item()))
    assert torch.equal(y, N.layernorm(dev(x), dev(w), dev(b), 1e-6)[0])
    with pytest.raises(N.SeaNativeError):
        N.layernorm(x, w, b, 1e-6)  # CPU tensors refused


def test_convnext_layernorm_module_uses_hip_and_matches_aten(N):
    from semseg.models import convnext_upernet as M
    ln = M.LayerNorm(96).cuda()
    with torch.no_grad():
        ln.weight.normal_()
        ln.bias.normal_()
    x = torch.randn(2, 20, 24, 96, device="cuda")
    outs = []
    for frozen in (True, False):  # parameters that require grad stay on ATen
        for p in ln.parameters():
            p.requires_grad_(not frozen)
        xi = x.clone().requires_grad_(True)
        y = ln(xi)
        assert (type(y.grad_fn).__name__ == "_LayerNormHipBackward") == frozen
        (gx,) = torch.autograd.grad((y * y).sum(), xi)
        outs.append((y.detach(), gx))
    torch.testing.assert_close(outs[0][0], outs[1][0], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(outs[0][1], outs[1][1], rtol=1e-4, atol=1e-4)


def test_convmodule_pointwise_gemm_matches_miopen(N):
    from semseg.models import convnext_upernet as M
    torch.manual_seed(2)
    mod = M.ConvModule(96, 64, 1).cuda().eval()
    mod.batch_norm.running_mean.normal_()
    mod.batch_norm.running_var.uniform_(0.5, 2.0)
    with torch.no_grad():
        mod.batch_norm.weight.uniform_(0.5, 1.5)
        mod.batch_norm.bias.normal_()
    for p in mod.parameters():
        p.requires_grad_(False)
    x = torch.randn(2, 96, 20, 28, device="cuda").contiguous(memory_format=torch.channels_last)
    outs = []
    try:
        for flag in (True, False):
            M.USE_GEMM_POINTWISE = flag
            assert M._pointwise_ok(mod, x) == flag
            xi = x.clone().requires_grad_(True)
            y = mod(xi)
            (gx,) = torch.autograd.grad((y * y).sum(), xi)
            outs.append((y.detach(), gx))
    finally:
        M.USE_GEMM_POINTWISE = True
    assert outs[0][0].shape == outs[1][0].shape and outs[0][0].is_contiguous(memory_format=torch.channels_last)
    torch.testing.assert_close(outs[0][0], outs[1][0], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(outs[0][1], outs[1][1], rtol=1e-4, atol=1e-4)
    mod.train()
    assert not M._pointwise_ok(mod, x)  # training-mode BatchNorm keeps the reference composition


# ------------------------------------------------------------------------------------------------ M4
@pytest.mark.parametrize("m", [2, 4])
@pytest.mark.parametrize("case", [(2, 8, 12, 16, 16), (1, 64, 32, 33, 31), (2, 4, 4, 5, 7), (1, 16, 8, 1, 1),
                                  (1, 256, 64, 64, 64)])
def test_winograd_conv3x3_forward_and_input_gradient(N, m, case):
    """Winograd transforms + batched GEMM against conv2d in float64: values, bias, ragged tiles, and the
    input-gradient convolution (rotated filters)."""
    import torch.nn.functional as F
    B, Cin, Cout, H, W = case
    g = torch.Generator().manual_seed(Cin * 7 + H)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
    bias = torch.randn(Cout, generator=g)
    gy = torch.randn(B, Cout, H, W, generator=g)
    xd = x.double().requires_grad_(True)
    ref = F.conv2d(xd, w.double(), bias.double(), padding=1)
    (gx_ref,) = torch.autograd.grad(ref, xd, gy.double())
    cl = torch.channels_last
    tol = 2e-5 if m == 2 else 3e-4  # F(4x4,3x3) amplifies fp32 rounding ~20x (documented in DESIGN.md)
    U = N.wino_filter(dev(w), m, False)
    y = N.wino_conv3x3_cl(dev(x).contiguous(memory_format=cl), U, m, dev(bias))
    assert y.shape == (B, Cout, H, W) and y.is_contiguous(memory_format=cl)
    torch.testing.assert_close(y.cpu().double(), ref.detach(), rtol=tol, atol=tol)
    Ub = N.wino_filter(dev(w), m, True)
    gx = N.wino_conv3x3_cl(dev(gy).contiguous(memory_format=cl), Ub, m)
    torch.testing.assert_close(gx.cpu().double(), gx_ref, rtol=tol, atol=tol)
    # fused epilogue act(scale * conv + shift) and its backward as a gated / scaled prologue of the gradient conv
    scale = torch.rand(Cout, generator=g) + 0.5
    ref_nb = F.conv2d(xd, w.double(), None, padding=1)
    y2 = N.wino_conv3x3_cl(dev(x).contiguous(memory_format=cl), U, m, bias=dev(bias), scale=dev(scale), relu=True)
    ref2 = torch.relu(ref_nb * scale.double()[None, :, None, None] + bias.double()[None, :, None, None])
    torch.testing.assert_close(y2.cpu().double(), ref2.detach(), rtol=2 * tol, atol=2 * tol)
    gate = torch.randn(B, Cout, H, W, generator=g)
    (gx_ref2,) = torch.autograd.grad(ref_nb, xd, gy.double() * scale.double()[None, :, None, None] * (gate > 0))
    gx2 = N.wino_conv3x3_cl(dev(gy).contiguous(memory_format=cl), Ub, m, gate=dev(gate).contiguous(memory_format=cl),
                            gate_scale=dev(scale))
    torch.testing.assert_close(gx2.cpu().double(), gx_ref2, rtol=2 * tol, atol=2 * tol)
    # the gradient convolution reads a channel slice of a wider NHWC tensor in place
    wide = torch.zeros(B, Cout + 8, H, W, device="cuda").contiguous(memory_format=cl)
    wide[:, 4:4 + Cout] = dev(gy)
    torch.testing.assert_close(N.wino_conv3x3_cl(wide[:, 4:4 + Cout], Ub, m), gx, rtol=0, atol=0)
    # deterministic
    assert torch.equal(y, N.wino_conv3x3_cl(dev(x).contiguous(memory_format=cl), U, m, dev(bias)))
    with pytest.raises(N.SeaNativeError):
        N.wino_conv3x3_cl(dev(x).contiguous() if W > 1 else dev(x)[:, :, :, :0], U, m)


@pytest.mark.parametrize("terms", [22, 3, 2])
def test_winograd_products_on_the_matrix_cores(N, terms):
    """the Winograd-domain GEMMs through M8 (split operands): same result as the fp32 hipBLASLt batched GEMM to the
    accuracy of the split; in fp16 x 2 mode the input transform itself supplies max|V| (no pass over V)"""
    g = torch.Generator().manual_seed(5)
    B, Cin, Cout, H, W = 2, 64, 96, 64, 60
    x = (torch.randn(B, Cin, H, W, generator=g) * 3).cuda().contiguous(memory_format=torch.channels_last)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)).cuda()
    U = N.wino_filter(w, 4, False)
    ref = torch.nn.functional.conv2d(x.double(), w.double(), padding=1)
    y0 = N.wino_conv3x3_cl(x, U, 4)
    y1 = N.wino_conv3x3_cl(x, U, 4, gemm_terms=terms)
    e0 = (y0.double() - ref).abs().max().item() / ref.abs().max().item()
    e1 = (y1.double() - ref).abs().max().item() / ref.abs().max().item()
    print(f"winograd F(4,3), max err / max|y| vs float64 conv2d: fp32 GEMM {e0:.2e}, split terms {terms} {e1:.2e}")
    # F(4x4,3x3) amplifies the rounding of its products ~20x: the yardstick is the fp32-GEMM Winograd path
    assert e1 <= {22: 2.0, 3: 2.0, 2: 40.0}[terms] * e0 + 1e-6, (e0, e1)
    # a list of inputs (virtual concatenation): every transform launch maxes into the same per-tile words
    y2 = N.wino_conv3x3_cl([x[:, :32], x[:, 32:]], U, 4, gemm_terms=terms)
    assert torch.equal(y1, y2)
    # an image's result does not depend on its batch partner (fp16 x 2: per-tile scales; bf16 terms: no scales at all)
    xb = torch.cat([x[:1], x[1:] * 300.0, x[1:] * 1e-3, x[:1]]).contiguous(memory_format=torch.channels_last)
    yb = N.wino_conv3x3_cl(xb, U, 4, gemm_terms=terms)
    assert torch.equal(yb[0], y1[0]) and torch.equal(yb[3], y1[0])


def test_convmodule_winograd_matches_miopen(N):
    from semseg.models import convnext_upernet as M
    torch.manual_seed(1)
    mod = M.ConvModule(64, 32, 3, padding=1).cuda().eval()
    mod.batch_norm.running_mean.normal_()
    mod.batch_norm.running_var.uniform_(0.5, 2.0)
    for p in mod.parameters():
        p.requires_grad_(False)
    x = torch.randn(2, 64, 40, 36, device="cuda").contiguous(memory_format=torch.channels_last)
    outs, default_tile = [], M.WINOGRAD_TILE
    try:
        for tile in (2, 4, 0):
            M.WINOGRAD_TILE = tile
            xi = x.clone().requires_grad_(True)
            y = mod(xi)
            (gx,) = torch.autograd.grad((y * y).sum(), xi)
            outs.append((y.detach(), gx))
    finally:
        M.WINOGRAD_TILE = default_tile
    for k, tol in ((0, 2e-5), (1, 3e-4)):
        torch.testing.assert_close(outs[k][0], outs[2][0], rtol=tol, atol=tol)
        torch.testing.assert_close(outs[k][1], outs[2][1], rtol=tol * 10, atol=tol * 10)
    # weights that require grad (PIR-AT training) stay on the MIOpen path
    for p in mod.parameters():
        p.requires_grad_(True)
    assert not M._wino_ok(mod.conv, x)
    # in-place weight updates invalidate the cached Winograd-domain filters
    for p in mod.parameters():
        p.requires_grad_(False)
    M.WINOGRAD_TILE = 2
    y0 = mod(x)
    mod.conv.weight.mul_(2.0)
    y1 = mod(x)
    M.WINOGRAD_TILE = 0
    try:
        torch.testing.assert_close(y1, mod(x), rtol=2e-5, atol=2e-5)
    finally:
        M.WINOGRAD_TILE = default_tile
    assert not torch.equal(y0, y1)


# ------------------------------------------------------------------------------------------------ M3
@pytest.mark.parametrize("shape", [(2, 96, 128, 128), (1, 768, 16, 16), (3, 4, 2, 2), (2, 100, 6, 10), (1, 192, 64, 64)])
def test_fused_transposes(N, shape):
    g = torch.Generator().manual_seed(shape[1])
    x = torch.randn(shape, generator=g)
    sc = torch.rand(shape[1], generator=g) + 0.5
    y = N.nchw_to_nhwc(dev(x))
    assert torch.equal(y.cpu(), x.permute(0, 2, 3, 1).contiguous())
    ys = N.nchw_to_nhwc(dev(x), dev(sc))
    assert torch.equal(ys.cpu(), (x * sc.view(1, -1, 1, 1)).permute(0, 2, 3, 1).contiguous())
    t = torch.randn(shape[0], shape[2], shape[3], shape[1], generator=g)
    res = torch.randn(shape, generator=g)
    assert torch.equal(N.nhwc_to_nchw(dev(t)).cpu(), t.permute(0, 3, 1, 2).contiguous())
    out = N.nhwc_to_nchw(dev(t), dev(sc), dev(res))
    ref = res + (sc * t).permute(0, 3, 1, 2)   # same float32 op order: scale, then add
    assert torch.equal(out.cpu(), ref)


def test_convnext_block_fast_layout_path_matches_plain_path(N):
    from semseg.models import convnext_upernet as M
    torch.manual_seed(0)
    blk = M.Block(96).cuda().eval()
    with torch.no_grad():
        blk.gamma.mul_(torch.rand(96, device="cuda") + 0.5)
    x = torch.randn(2, 96, 32, 32, device="cuda")
    outs = []
    for flag in (True, False):
        M.USE_HIP_TRANSPOSE = flag
        for p in blk.parameters():
            p.grad = None
        xi = x.clone().requires_grad_(True)
        y = blk(xi)
        y.square().sum().backward()
        outs.append((y.detach(), xi.grad, blk.gamma.grad.clone(), blk.norm.weight.grad.clone()))
    M.USE_HIP_TRANSPOSE = True
    for a, b in zip(*outs):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("shape", [(2, 96, 64, 64), (1, 768, 16, 16), (2, 192, 33, 21), (1, 4, 7, 70), (2, 384, 32, 32),
                                   (1, 8, 1, 9), (1, 8, 2, 5), (1, 12, 5, 128), (1, 192, 64, 64), (1, 96, 31, 40)])
def test_dwconv7x7_nhwc_forward_and_backward_data(N, shape):
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(shape[1] + 1)
    B, C, H, W = shape
    x = torch.randn(shape, generator=g)
    w = torch.randn(C, 1, 7, 7, generator=g) * 0.1
    b = torch.randn(C, generator=g)
    xd = x.double().requires_grad_(True)
    ref = F.conv2d(xd, w.double(), b.double(), padding=3, groups=C)
    gy = torch.randn(ref.shape, generator=g)
    (gx_ref,) = torch.autograd.grad(ref, xd, gy.double())
    wt = w.view(C, 49).t().contiguous()
    y = N.dwconv7x7_nhwc(dev(x.permute(0, 2, 3, 1).contiguous()), dev(wt), dev(b))
    torch.testing.assert_close(y.cpu().permute(0, 3, 1, 2).double(), ref.detach(), rtol=1e-5, atol=1e-5)
    gx = N.dwconv7x7_nhwc(dev(gy.permute(0, 2, 3, 1).contiguous()), dev(wt), None, flip=True)
    # the two-rows-per-lane kernel (default), the one-row kernel (flip bit 2) and the plain block order (bit 1) agree
    # bit for bit: same accumulation order per output
    xn = dev(x.permute(0, 2, 3, 1).contiguous())
    gyn = dev(gy.permute(0, 2, 3, 1).contiguous())
    skip = dev(torch.randn(gyn.shape, generator=g))
    # fused skip-gradient add: bitwise the separate element-wise add, in both kernel variants
    assert torch.equal(N.dwconv7x7_nhwc(gyn, dev(wt), None, flip=True, addend=skip), gx + skip)
    assert torch.equal(N.dwconv7x7_nhwc(xn, dev(wt), None, flip=False, addend=skip), N.dwconv7x7_nhwc(xn, dev(wt), None) + skip)
    assert torch.equal(N.dwconv7x7_nhwc(gyn, dev(wt), None, flip=2, addend=skip), gx + skip)   # `flip` is a boolean
    with pytest.raises(N.SeaNativeError):
        N.dwconv7x7_nhwc(xn, dev(wt), dev(b), addend=skip)  # bias and addend are mutually exclusive
    # the A/B switches of the launcher (the `ab` mask, per call: 2 = plain block order, 4 = one row per lane, 8 = force two
    # rows, 16 = the plain kernels instead of the software-pipelined ones of the ConvNeXt widths, 32 / 64 = their filter rows
    # never / always through LDS)
    for bits in (2, 4, 6, 8, 10, 16, 20, 24, 36, 40, 68, 72):
        assert torch.equal(y, N.dwconv7x7_nhwc(xn, dev(wt), dev(b), ab=bits))
        assert torch.equal(gx, N.dwconv7x7_nhwc(dev(gy.permute(0, 2, 3, 1).contiguous()), dev(wt), None, flip=True, ab=bits))
        assert torch.equal(N.dwconv7x7_nhwc(gyn, dev(wt), None, flip=True, addend=skip, ab=bits), gx + skip)
    torch.testing.assert_close(gx.cpu().permute(0, 3, 1, 2).double(), gx_ref, rtol=1e-5, atol=1e-5)


def test_convnext_block_channels_last_path(N):
    """the all-NHWC block path (channels_last input) equals the plain PyTorch block, incl. parameter grads"""
    from semseg.models import convnext_upernet as M
    torch.manual_seed(1)
    blk = M.Block(192).cuda().eval()
    with torch.no_grad():
        blk.gamma.mul_(torch.rand(192, device="cuda") + 0.5)
    x = torch.randn(2, 192, 24, 40, device="cuda").contiguous(memory_format=torch.channels_last)
    outs = []
    for flag in (True, False):
        M.USE_HIP_DWCONV = flag
        for p in blk.parameters():
            p.grad = None
        xi = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
        y = blk(xi)
        y.square().sum().backward()
        outs.append((y.detach(), xi.grad, blk.gamma.grad.clone(), blk.dwconv.weight.grad.clone(), blk.dwconv.bias.grad.clone()))
    M.USE_HIP_DWCONV = True
    assert outs[0][0].is_contiguous(memory_format=torch.channels_last)
    for a, b in zip(*outs):
        torch.testing.assert_close(a, b, rtol=2e-4, atol=2e-4 * b.abs().max().item())


def test_convnext_block_frozen_weights_fold_layer_scale(N):
    """attack-time block (frozen parameters): NHWC path with M1 + M5 and the layer scale folded into pwconv2
    against the plain PyTorch block; an in-place change of gamma invalidates the fold."""
    from semseg.models import convnext_upernet as M
    torch.manual_seed(2)
    blk = M.Block(96).cuda().eval()
    with torch.no_grad():
        blk.gamma.mul_(torch.rand(96, device="cuda") + 0.5)
        blk.pwconv2.bias.normal_()
    for p in blk.parameters():
        p.requires_grad_(False)
    x = torch.randn(2, 96, 20, 28, device="cuda").contiguous(memory_format=torch.channels_last)

    def run(flag):
        M.USE_HIP_DWCONV = flag
        try:
            xi = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
            y = blk(xi)
            (g,) = torch.autograd.grad(y.square().sum(), xi)
            return y.detach(), g
        finally:
            M.USE_HIP_DWCONV = True

    fast, ref = run(True), run(False)
    assert "_fold_cache" in blk.__dict__
    for a, b in zip(fast, ref):
        torch.testing.assert_close(a, b, rtol=2e-4, atol=2e-4 * b.abs().max().item())
    blk.gamma.mul_(3.0)
    fast2, ref2 = run(True), run(False)
    torch.testing.assert_close(fast2[0], ref2[0], rtol=2e-4, atol=2e-4 * ref2[0].abs().max().item())
    assert not torch.allclose(fast2[0], fast[0])


@pytest.mark.parametrize("terms", [22, 3])
def test_block_mlp_with_fused_epilogues_matches_the_unfused_pair(N, terms):
    """_FrozenMlp (GELU / GELU' / residual in the GEMM epilogues) against the same two GEMMs with ATen's GELU and add
    between them: same products, so only the element-wise rounding differs; ConvNeXt block and Segmenter feed-forward"""
    from semseg.models import convnext_upernet as M
    from semseg.models import segmenter as S
    torch.manual_seed(4)
    blk = M.Block(128).cuda().eval()
    ff = S.FeedForward(192, 768, 0.0).cuda().eval()
    with torch.no_grad():
        blk.gamma.mul_(torch.rand(128, device="cuda") + 0.5)
    for p in list(blk.parameters()) + list(ff.parameters()):
        p.requires_grad_(False)
    xb = torch.randn(2, 128, 24, 32, device="cuda").contiguous(memory_format=torch.channels_last)
    xf = torch.randn(2, 600, 192, device="cuda")

    def run(mod, x, fuse):
        keep, M.FUSE_MLP = M.FUSE_MLP, fuse
        try:
            with M._gemm_terms(terms):
                xi = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
                y = mod(xi)
                names = set()
                stack = [y.grad_fn]
                while stack:
                    f = stack.pop()
                    if f is not None:
                        names.add(type(f).__name__)
                        stack.extend(n for n, _ in f.next_functions)
                (g,) = torch.autograd.grad((y * torch.cos(y)).sum(), xi)
            return y.detach(), g, names
        finally:
            M.FUSE_MLP = keep

    for mod, x in ((blk, xb), (ff, xf)):
        y0, g0, n0 = run(mod, x, -1)                       # separate autograd nodes, ATen GELU
        assert "_FrozenMlpBackward" not in n0 and "GeluBackward0" in n0
        for mask in (7, 24, 8, 0):                         # epilogue fusions / the default prologues (GELU, GELU') / none
            y1, g1, n1 = run(mod, x, mask)
            assert "_FrozenMlpBackward" in n1 and "GeluBackward0" not in n1
            torch.testing.assert_close(y1, y0, rtol=1e-5, atol=1e-5 * y0.abs().max().item())
            torch.testing.assert_close(g1, g0, rtol=1e-4, atol=2e-5 * g0.abs().max().item())
            assert y1.stride() == y0.stride()
        if mask == 0:
            assert torch.equal(y1, y0)
    # Segmenter's block hands its residual to the feed-forward (it rides in the split-K reduce pass of the second GEMM)
    with M._gemm_terms(terms):
        r0 = torch.randn_like(xf)
        torch.testing.assert_close(ff(xf, res=r0), r0 + ff(xf), rtol=0, atol=1e-6 * (r0 + ff(xf)).abs().max().item())


# ------------------------------------------------------------------------------------------------ full-size ADE workloads
def _ade_case(b, seed, C=151, H=512, W=512, dtype=torch.float32):
    """one image of the SURVEY 8(d) micro-benchmark distribution (generated per image to bound host memory)"""
    g = torch.Generator().manual_seed(seed * 131 + b)
    logits = torch.randn(1, C, H, W, generator=g) * 3
    y = torch.randint(0, C, (1, H, W), generator=g)
    boost = (torch.rand(1, H, W, generator=g) < 0.7).float() * 6
    logits.scatter_add_(1, y.unsqueeze(1), boost.unsqueeze(1))
    y[torch.rand(1, H, W, generator=g) < 0.03] = -1
    return logits.to(dtype), y


@pytest.mark.parametrize("dtype,mode", [(torch.float32, 1), (torch.float32, 2), (torch.bfloat16, 1)])
def test_loss_kernel_full_size_ade_batch(N, dtype, mode):
    """BASELINE configs[2..4] size: 8 x 151 x 512 x 512 (1.27 GB of fp32 logits and as much gradient per launch; the
    238-VGPR one-pixel-per-lane instantiation at its full grid).  Ints exact, losses 1e-4, gradient element-wise;
    the oracle runs image by image on the host."""
    from semseg.utils.utils import ADE_WTS
    B, C, H, W = 8, 151, 512, 512
    HW = H * W
    w = torch.tensor(ADE_WTS)
    imgs = [_ade_case(b, 9, dtype=dtype) for b in range(B)]
    logits = torch.cat([i[0] for i in imgs]).cuda()
    y = torch.cat([i[1] for i in imgs])
    y8 = torch.where(y < 0, torch.full_like(y, 255), y).to(torch.uint8).cuda()
    pred = torch.empty(B, H, W, dtype=torch.uint8, device="cuda")
    r = N.loss_fwd_bwd(logits, y8, w.cuda(), mode, 3, 1.0 / HW, want_grad=True, pred=pred)
    r0 = N.loss_fwd_bwd(logits, y8, w.cuda(), mode, 3, 1.0 / HW, want_grad=False,
                        pred=torch.empty_like(pred))                       # the no-gradient variant, same sums
    torch.cuda.synchronize()
    assert torch.equal(r["n_correct"], r0["n_correct"]) and torch.equal(r0["pred"], pred)
    for k in ("loss_sum", "track_sum"):
        torch.testing.assert_close(r[k], r0[k], rtol=1e-5, atol=0)
    del logits
    for b in range(B):
        lg, yb = imgs[b]
        ref = O.loss_fwd_bwd(lg.float(), yb, w, mode, 3, with_grad=True)
        assert torch.equal(pred[b].cpu().long(), ref["pred"][0])
        assert int(r["n_correct"][b]) == int(ref["n_correct"][0])
        assert (r["loss_sum"][b] / HW).item() == pytest.approx(ref["loss_img"][0].item(), rel=1e-4, abs=1e-6)
        assert (r["track_sum"][b] / HW).item() == pytest.approx(ref["track_img"][0].item(), rel=1e-4, abs=1e-6)
        got = r["dlogits"][b].float().cpu()
        tol = dict(rtol=1e-4, atol=2e-8 + 1e-6 / HW) if dtype == torch.float32 else dict(rtol=2e-2, atol=1e-2 / HW)
        torch.testing.assert_close(got, ref["dlogits"][0], **tol)
        # size-independent: soft-max gradient rows sum to zero (to the rounding of the output type)
        assert got.sum(0).abs().max().item() < (1e-9 if dtype == torch.float32 else 2e-7)


@pytest.mark.parametrize("case", [(151, 32, 512, "Segmenter x16"), (151, 128, 512, "UperNet x4"), (21, 128, 512, "UperNet x4")])
def test_fused_upsample_loss_kernel_full_size(N, case):
    """K2u at the BASELINE sizes: 8 x C x (32|128)^2 low-res logits -> 512^2 labels."""
    C, hl, HH, _ = case
    B = 8
    g = torch.Generator().manual_seed(C + hl)
    low = torch.randn(B, C, hl, hl, generator=g) * 3
    wts = torch.rand(C, generator=g) + 0.01
    ys = []
    for b in range(B):   # labels: the interpolated argmax with 30 % flips and 3 % ignored
        yb = torch.nn.functional.interpolate(low[b:b + 1], size=(HH, HH), mode="bilinear", align_corners=False).max(1)[1]
        flip = torch.rand(1, HH, HH, generator=g) < 0.3
        yb[flip] = torch.randint(0, C, (int(flip.sum()),), generator=g)
        yb[torch.rand(1, HH, HH, generator=g) < 0.03] = -1
        ys.append(yb)
    y = torch.cat(ys)
    pred = torch.empty(B, HH, HH, dtype=torch.int64, device="cuda")
    r = N.loss_fwd_bwd_upsampled(low.cuda(), y.cuda(), wts.cuda(), 1, 3, 1.0 / (HH * HH), want_grad=True, pred=pred)
    torch.cuda.synchronize()
    for b in range(B):
        ref = O.loss_fwd_bwd_upsampled(low[b:b + 1], y[b:b + 1], wts, 1, 3, with_grad=True)
        top2 = ref["logits_hi"].topk(2, dim=1)[0]
        safe = (top2[:, 0] - top2[:, 1]) > 1e-4
        assert torch.equal(pred[b:b + 1].cpu()[safe], ref["pred"][safe])
        assert abs(int(r["n_correct"][b]) - int(ref["n_correct"][0])) <= int((~safe).sum())
        assert (r["loss_sum"][b] / (HH * HH)).item() == pytest.approx(ref["loss_img"][0].item(), rel=1e-4, abs=1e-6)
        assert (r["track_sum"][b] / (HH * HH)).item() == pytest.approx(ref["track_img"][0].item(), rel=1e-4, abs=1e-6)
        scale = ref["dlow"].abs().max().item()
        torch.testing.assert_close(r["dlogits"][b:b + 1].cpu(), ref["dlow"], rtol=2e-3, atol=2e-4 * scale + 1e-9)


def test_counts_full_size_ade(N):
    """K3 at C=151, 8 x 512 x 512: per-image tables and the confusion matrix, exact."""
    C, shape = 151, (8, 512, 512)
    g = torch.Generator().manual_seed(5)
    y = torch.randint(0, C, shape, generator=g)
    pred = torch.where(torch.rand(shape, generator=g) < 0.6, y, torch.randint(0, C, shape, generator=g))
    y[torch.rand(shape, generator=g) < 0.04] = -1
    y[y == 150] = 3                                                         # an absent class
    for mask_pred in (True, False):
        ref = O.class_counts(pred, y, C, per_image=True, mask_pred=mask_pred)
        y8 = torch.where(y < 0, torch.full_like(y, 255), y).to(torch.uint8)
        got = N.class_counts(pred.to(torch.uint8).cuda(), y8.cuda(), C, per_image=True, mask_pred=mask_pred)
        for a, b in zip(got, ref):
            assert torch.equal(a.cpu(), b)
    hist = N.confusion(pred.cuda(), y.cuda(), C)
    assert torch.equal(hist.cpu(), O.confusion_matrix(pred, y, C))


# ------------------------------------------------------------------------------------------------ M7 attention
@pytest.mark.parametrize("case", [(2, 6, 1025, "ViT-S/16 encoder, 512x512"), (1, 6, 1175, "mask transformer, 1024 patches + 151 classes"),
                                  (3, 2, 64, "one tile"), (1, 1, 33, "ragged"), (2, 3, 130, "two blocks, ragged"),
                                  (2, 2, 1, "one row, every other lane clamped"), (2, 2, 65, "second tile with one key"),
                                  (2, 2, 129, "second block with one row, three idle waves")])
@pytest.mark.parametrize("terms", [(22, 22), (3, 22), (3, 2), (3, 3), (0, 0)])
def test_fp32_mfma_attention_forward_and_backward(N, case, terms):
    """softmax(q k^T * scale) v as written in the reference (vit_encoder.py:106-127), explicit fp32 (and an fp64 check).
    terms = (forward, backward) arithmetic of M7b (csrc/attention_bf16.hip): bf16 terms per operand, 22 = fp16 x 2; (0, 0) =
    the fp32 MFMA kernels of M7.  Shipped: (22, 22): forward, log-sum-exp and input gradient with 22-bit operands (fp32-level:
    the strict bounds); (3, 2) is round 3's 16-bit gradient."""
    import os
    B, H, T, _ = case
    os.environ["SEA_ATTN_TERMS"], os.environ["SEA_ATTN_TERMS_BWD"] = str(terms[0]), str(terms[1])
    try:
        _attention_case(N, B, H, T, strict_backward=terms[1] != 2)
    finally:
        os.environ.pop("SEA_ATTN_TERMS", None)
        os.environ.pop("SEA_ATTN_TERMS_BWD", None)


def _attention_case(N, B, H, T, strict_backward):
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(B, T, 3, H, 64, generator=g)
    qkv[:, :, 0] *= 1.5                                      # asymmetric operands: a transposed tile would not cancel
    qkv[:, 3 % T, 1] += 2.0                                  # one key that dominates some rows (large max)
    gout = torch.randn(B, T, H * 64, generator=g)
    scale = 64 ** -0.5

    def ref(t, dt):
        x = t.to(dt).requires_grad_(True)
        q, k, v = x.permute(2, 0, 3, 1, 4)
        att = ((q @ k.transpose(-2, -1)) * scale).softmax(-1)
        y = (att @ v).transpose(1, 2).reshape(B, T, H * 64)
        (gx,) = torch.autograd.grad(y, [x], grad_outputs=gout.to(dt))
        return y.detach(), gx

    y64, g64 = ref(qkv, torch.float64)
    out, lse = N.attention_qkv(dev(qkv), scale)
    dq = N.attention_qkv_backward(dev(qkv), out, lse, dev(gout), scale)
    torch.cuda.synchronize()
    err_y = (out.cpu().double() - y64).abs().max().item()
    err_g = (dq.cpu().double() - g64).abs().max().item()
    y32, g32 = ref(qkv, torch.float32)                        # the fp32 composition's own error vs fp64 as yardstick
    assert err_y <= max(2e-6, 3 * (y32.double() - y64).abs().max().item()), err_y
    if strict_backward:
        assert err_g <= max(1e-5, 3 * (g32.double() - g64).abs().max().item()), err_g
    else:   # two bf16 terms per operand: 2^-17 relative per product; measured 1.5-1.8e-4 of max|g| ~ 5
        assert err_g <= 1e-4 * g64.abs().max().item(), (err_g, g64.abs().max().item())
    ref_lse = torch.logsumexp((qkv[:, :, 0].permute(0, 2, 1, 3).double() @ qkv[:, :, 1].permute(0, 2, 3, 1).double()) * scale, -1)
    torch.testing.assert_close(lse.cpu().double(), ref_lse, rtol=1e-6, atol=1e-5)
    # deterministic
    dq2 = N.attention_qkv_backward(dev(qkv), out, lse, dev(gout), scale)
    assert torch.equal(dq, dq2)


def _attn_ref64(qkv, gout, scale):
    B, T, _, H, _ = qkv.shape
    x = qkv.double().requires_grad_(True)
    q, k, v = x.permute(2, 0, 3, 1, 4)
    att = ((q @ k.transpose(-2, -1)) * scale).softmax(-1)
    y = (att @ v).transpose(1, 2).reshape(B, T, H * 64)
    (gx,) = torch.autograd.grad(y, [x], grad_outputs=gout.double())
    return gx


@pytest.mark.parametrize("case", ["plain", "rows spanning orders of magnitude"])
def test_attention_backward_fp16x2_is_as_accurate_as_three_bf16_terms(N, case):
    """fp16 x 2 (three MFMA products per operand pair) against three bf16 terms (six products) and float64: the error of the
    shipped backward is at the level of the exact-operand mode -- also when the gradient rows (tokens, images) and the
    activations span many orders of magnitude, which is what the power-of-two scales per row / per (image, head) are for."""
    g = torch.Generator().manual_seed(77)
    B, H, T = 3, 6, 1025
    qkv = torch.randn(B, T, 3, H, 64, generator=g)
    gout = torch.randn(B, T, H * 64, generator=g)
    if case != "plain":
        gout = gout * torch.exp2(torch.randint(-20, 1, (B, T, 1), generator=g).float()) * torch.tensor([1.0, 1e-4, 1e-8]).view(B, 1, 1)
        qkv[:, :, 2] *= torch.exp2(torch.randint(-6, 5, (B, 1, H, 1), generator=g).float())          # V per head
        qkv[:, :, 0] *= torch.exp2(torch.randint(-3, 3, (B, T, 1, 1), generator=g).float())          # Q per token
    scale = 64 ** -0.5
    ref = _attn_ref64(qkv, gout, scale)
    out, lse = N.attention_qkv(dev(qkv), scale)
    errs = {}
    for terms in (22, 3, 2):
        d = N.attention_qkv_backward(dev(qkv), out, lse, dev(gout), scale, terms=terms).cpu().double()
        # per image (their gradients differ by orders of magnitude): worst relative-to-max error over the images
        errs[terms] = max(((d[b] - ref[b]).abs().max() / ref[b].abs().max()).item() for b in range(B))
    print(f"\n[attention backward, {case}] max error / max|g| per image: fp16x2 {errs[22]:.2e}   bf16x3 {errs[3]:.2e}   bf16x2 {errs[2]:.2e}")
    assert errs[22] <= max(1.5 * errs[3], 2e-7), errs
    assert errs[22] < 0.1 * errs[2], errs


def test_segmenter_uses_hip_attention_and_matches_sdpa(N):
    from semseg.models import segmenter as S
    torch.manual_seed(0)
    att = S.Attention(384, 6, 0.0).cuda().eval()
    x = torch.randn(2, 1025, 384, device="cuda", requires_grad=True)
    gy = torch.randn(2, 1025, 384, device="cuda")
    outs = []
    for flag in (True, False):
        S.USE_HIP_ATTENTION = flag
        y = att(x)
        (gx,) = torch.autograd.grad(y, [x], grad_outputs=gy)
        outs.append((y.detach(), gx))
    S.USE_HIP_ATTENTION = True
    torch.testing.assert_close(outs[0][0], outs[1][0], rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(outs[0][1], outs[1][1], rtol=1e-4, atol=2e-5)


def test_patch_conv_2x2_matches_conv2d_and_is_deterministic(N):
    """the trunk's 2x2 / stride-2 down-sampling convolutions as patch gather + GEMM (convnext_orig.py:118-124)"""
    from semseg.models import convnext_upernet as M
    torch.manual_seed(0)
    for cin, cout, hw in ((96, 192, 32), (192, 384, 16), (8, 12, 6)):
        conv = torch.nn.Conv2d(cin, cout, 2, stride=2).cuda()
        for p in conv.parameters():
            p.requires_grad_(False)
        x = torch.randn(2, cin, hw, hw, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
        g = torch.randn(2, cout, hw // 2, hw // 2, device="cuda")
        y = M._PatchConv2x2.apply(x, conv.weight, conv.bias, {})
        (gx,) = torch.autograd.grad(y, [x], grad_outputs=g)
        y0 = conv(x)
        (gx0,) = torch.autograd.grad(y0, [x], grad_outputs=g)
        torch.testing.assert_close(y, y0, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(gx, gx0, rtol=1e-4, atol=1e-5)
        y2 = M._PatchConv2x2.apply(x, conv.weight, conv.bias, {})
        assert torch.equal(y, y2)
        # the gather itself: exact
        xn = x.detach().permute(0, 2, 3, 1).contiguous()
        ref = xn.reshape(2, hw // 2, 2, hw // 2, 2, cin).permute(0, 1, 3, 2, 4, 5).reshape(-1, 4 * cin)
        assert torch.equal(N.patch2x2(xn), ref) and torch.equal(N.unpatch2x2(ref.contiguous(), 2, hw, hw), xn)
