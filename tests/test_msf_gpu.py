"""Multi-scale + flip evaluation on the device (`-m gpu`): K10a (input resize + flip), K10b (softmax accumulate, full-res
and low-res modes) against CPU / unfused device computations, and semseg.val.evaluate_msf against the reference's own
evaluate_msf (tests/golden/g15_msf_*.npz, devtools/gen_msf_goldens.py) and against the unfused device path on the real
models."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def N():
    from semseg import _native
    _native.lib()
    return _native


# ---------------------------------------------------------------------------------------------------------------- K10a
@pytest.mark.parametrize("shape,size", [((2, 3, 45, 61), (96, 128)), ((2, 3, 64, 64), (32, 32)), ((1, 3, 45, 61), (32, 32)),
                                        ((3, 3, 7, 5), (64, 96)), ((8, 3, 512, 512), (896, 896))])
def test_resize_flip_matches_interpolate(N, shape, size):
    g = torch.Generator().manual_seed(sum(shape) + size[0])
    x = torch.rand(shape, generator=g)
    want = F.interpolate(x, size=size, mode="bilinear", align_corners=True)
    y, yf = N.msf_resize_input(x.to(DEV), size, flip=True)
    assert (y.cpu() - want).abs().max() <= 2e-7
    assert torch.equal(yf, y.flip(3))
    y2, yf2 = N.msf_resize_input(x.to(DEV), size, flip=True)
    assert torch.equal(y, y2) and torch.equal(yf, yf2)
    y3, none = N.msf_resize_input(x.to(DEV), size, flip=False)
    assert none is None and torch.equal(y3, y)


# ---------------------------------------------------------------------------------------------------------------- K10b
def _ac_axis(n_in, n_out):
    """ATen's align_corners=True index / lambda rule in float32 (what the kernel and the reference compute)"""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    src = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    lam = np.clip(src - i0.astype(np.float32), 0, 1).astype(np.float64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, lam


def _resize_fp64(v, size):
    """(B, C, h, w) float64 -> (B, C, H, W): align_corners=True bilinear with the fp32 index rule, fp64 values"""
    (a0, a1, ly), (b0, b1, lx) = _ac_axis(v.shape[2], size[0]), _ac_axis(v.shape[3], size[1])
    lx, ly = torch.from_numpy(lx), torch.from_numpy(ly)[:, None]
    r0, r1 = v[:, :, a0], v[:, :, a1]
    top = (1 - lx) * r0[..., b0] + lx * r0[..., b1]
    bot = (1 - lx) * r1[..., b0] + lx * r1[..., b1]
    return (1 - ly) * top + ly * bot


@pytest.mark.parametrize("C", [5, 21, 151])
@pytest.mark.parametrize("scaled,out", [((64, 96), (45, 61)), ((32, 32), (45, 61)), ((96, 128), (96, 128))])
def test_accumulate_fullres_vs_fp64(N, C, scaled, out):
    g = torch.Generator().manual_seed(C * 7 + scaled[0] + out[1])
    B = 2
    logits = torch.randn(B, C, *scaled, generator=g) * 3
    score0 = torch.rand(B, C, *out, generator=g) * 4
    score = score0.to(DEV)
    N.msf_accumulate(logits.to(DEV), score, scaled, flip=False)
    N.msf_accumulate(logits.to(DEV), score, scaled, flip=True)
    lg = logits.double()
    want = score0.double() + _resize_fp64(lg, out).softmax(1) + _resize_fp64(lg.flip(3), out).softmax(1)
    err = (score.cpu().double() - want).abs().max().item()
    print(f"C={C} {scaled}->{out}: max |err| {err:.2e}")
    assert err <= 1e-6
    again = score0.to(DEV)
    N.msf_accumulate(logits.to(DEV), again, scaled, flip=False)
    N.msf_accumulate(logits.to(DEV), again, scaled, flip=True)
    assert torch.equal(again, score)          # no atomics: bitwise reproducible


@pytest.mark.parametrize("C", [21, 151])
@pytest.mark.parametrize("r", [4, 16])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("out", [(45, 61), (128, 128)])
def test_accumulate_lowres_vs_unfused(N, C, r, flip, out):
    g = torch.Generator().manual_seed(C + r + out[0] + int(flip))
    B, scaled = 2, (96, 128)
    low = (torch.randn(B, C, scaled[0] // r, scaled[1] // r, generator=g) * 3).to(DEV)
    score0 = (torch.rand(B, C, *out, generator=g) * 4).to(DEV)
    up = N.upsample_bilinear(low, scaled)                       # the model's own final up-sampling (M2, = models._up)
    if flip:
        up = up.flip(3)
    want = score0 + F.interpolate(up, size=out, mode="bilinear", align_corners=True).softmax(1)
    got = N.msf_accumulate(low, score0.clone(), scaled, flip=flip)
    err = (got - want).abs().max().item()
    print(f"C={C} r={r} flip={flip} ->{out}: max |err| {err:.2e}")
    assert err <= 1e-6


# ---------------------------------------------------------------------------------------------------------------- evaluate_msf
class _Recorder:
    """patches semseg.val.Metrics with a subclass that keeps every score tensor handed to update()"""

    def __init__(self, monkeypatch):
        import semseg.val as V
        self.scores = []
        rec = self

        class RecMetrics(V.Metrics):
            def update(self, pred, target):
                rec.scores.append(pred.detach().cpu().clone())
                super().update(pred, target)

        monkeypatch.setattr(V, "Metrics", RecMetrics)


def _near_ties(score, tol=1e-5):
    top2 = score.topk(2, dim=1).values
    return (top2[:, 0] - top2[:, 1]) < tol


def _compare_hist(got_scores, ref_scores, labels, hist_got, hist_ref, what):
    """equal argmax except at pixels whose top-2 reference scores differ by < 1e-5; the histograms differ by those only"""
    ties = _near_ties(ref_scores)
    valid = labels != -1
    pred_got, pred_ref = got_scores.argmax(1), ref_scores.argmax(1)
    diff = (pred_got != pred_ref) & valid
    n_ties = int((ties & valid).sum())
    print(f"{what}: {n_ties} near-tie pixels of {int(valid.sum())}, {int(diff.sum())} argmax differences, "
          f"max |score diff| {(got_scores - ref_scores).abs().max().item():.2e}")
    assert not bool((diff & ~ties).any())
    assert n_ties <= max(4, valid.sum().item() // 200)
    assert (hist_got.long() - hist_ref.long()).abs().sum() <= 2 * int((diff & ties).sum())
    assert hist_got.sum() == hist_ref.sum()


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "g15_msf_*.npz"))), ids=os.path.basename)
def test_evaluate_msf_vs_reference_golden(N, path, monkeypatch):
    from oracle.tiny_models import PointwiseNet, TinyConvNet
    import semseg.val as V
    g = np.load(path)
    C, net_name = int(g["n_classes"]), str(g["net"])
    net = (TinyConvNet if net_name == "conv" else PointwiseNet)(C, seed=int(g["seed"])).to(DEV)
    x, y = torch.from_numpy(g["x"]), torch.from_numpy(g["y"])
    batches = [(x[i], y[i]) for i in range(x.shape[0])]
    rec = _Recorder(monkeypatch)
    scales, flip = [float(s) for s in g["scales"]], bool(int(g["flip"]))
    m = V._evaluate_msf_metrics(net, batches, DEV, scales, flip, n_classes=C, ignore_label=int(g["ignore_label"]))
    got, ref = torch.cat(rec.scores), torch.from_numpy(g["scaled_logits"]).flatten(0, 1)
    _compare_hist(got, ref, y.flatten(0, 1), m.hist.cpu(), torch.from_numpy(g["hist"]), os.path.basename(path))
    assert (got - ref).abs().max() <= 1e-4
    res = V.evaluate_msf(net, batches, DEV, scales, flip, n_classes=C, ignore_label=-1)
    assert len(res) == 6 and len(res[0]) == C and len(res[4]) == C
    assert res[5] == m.compute_iou()[1] and res[1] == m.compute_pixel_acc()[1]


def _unfused_scores(model, images, scales, flip, C, N):
    """the stock formulation on the device: full-resolution logits from model(x), interpolate, flip, softmax, sum"""
    from semseg.val import msf_scaled_size
    B, _, H, W = images.shape
    score = torch.zeros(B, C, H, W, device=DEV)
    for s in scales:
        size = msf_scaled_size(s, H, W)
        x_s, x_f = N.msf_resize_input(images, size, flip=True)
        score += F.interpolate(model(x_s), size=(H, W), mode="bilinear", align_corners=True).softmax(1)
        if flip:
            score += F.interpolate(model(x_f).flip(3), size=(H, W), mode="bilinear", align_corners=True).softmax(1)
    return score


@pytest.mark.parametrize("cfg,C", [("pascalvoc_convnext.yaml", 21), ("ade20k_segmenter.yaml", 151)])
def test_evaluate_msf_real_models_lowres_fused(N, cfg, C, monkeypatch):
    import yaml
    import semseg.val as V
    from semseg import _native
    from tools.infer import build_model
    with open(os.path.join(PKG, "configs", cfg)) as f:
        conf = yaml.load(f, Loader=yaml.SafeLoader)
    torch.manual_seed(0)
    model = build_model(conf, random_init=True, device=DEV)
    for p in model.parameters():
        p.requires_grad_(False)
    gen = torch.Generator().manual_seed(C)
    B, H, W, scales = 2, 256, 256, (0.5, 1.0, 1.5)
    images = torch.rand(B, 3, H, W, generator=gen)
    labels = torch.randint(0, C, (B, H, W), generator=gen)
    labels[torch.rand(B, H, W, generator=gen) < 0.05] = -1
    with torch.no_grad():
        ref = _unfused_scores(model, images.to(DEV), scales, True, C, N)
        # peak of one low-res forward at the largest scale: the model's own activations
        x_big = torch.rand(B, 3, *V.msf_scaled_size(max(scales), H, W), device=DEV)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        model.forward_lowres(x_big)
        torch.cuda.synchronize()
        fwd_peak = torch.cuda.max_memory_allocated() - base
        del x_big
    hist_ref = torch.zeros(C, C, dtype=torch.int64)
    pr, lb = ref.argmax(1).cpu(), labels
    keep = lb != -1
    hist_ref += torch.bincount(lb[keep] * C + pr[keep], minlength=C * C).view(C, C)
    calls = []
    real_acc = _native.msf_accumulate

    def spy(logits, score, scaled_size, flip=False):
        calls.append((tuple(logits.shape[2:]), tuple(scaled_size)))
        return real_acc(logits, score, scaled_size, flip=flip)

    monkeypatch.setattr(_native, "msf_accumulate", spy)
    rec = _Recorder(monkeypatch)
    images_d, labels_d = images.to(DEV), labels.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m = V._evaluate_msf_metrics(model, [(images_d, labels_d)], DEV, scales, True, n_classes=C, ignore_label=-1)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert len(calls) == 2 * len(scales)
    assert all(lo[0] < sc[0] and lo[1] < sc[1] for lo, sc in calls), calls     # the low-res path ran every pass
    _compare_hist(rec.scores[0], ref.cpu(), labels, m.hist.cpu(), hist_ref, f"real {cfg}")
    Hs, Ws = V.msf_scaled_size(max(scales), H, W)
    full = B * C * Hs * Ws * 4          # one full-resolution scaled-logits tensor at the largest scale
    print(f"{cfg}: evaluate_msf peak {peak / 2**20:.1f} MB above the inputs, one low-res forward {fwd_peak / 2**20:.1f} MB, "
          f"full-res scaled logits {full / 2**20:.1f} MB")
    assert peak - fwd_peak < full
    if fwd_peak < full:       # (Segmenter at C = 151: the activations are smaller than the logits)
        assert peak < full
