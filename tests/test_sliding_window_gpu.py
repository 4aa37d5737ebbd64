"""Sliding-window evaluation on the device (`-m gpu`): K11a (merge of window logits, full-res and low-res modes, both
epilogues) and K11b (resize + flip + softmax) against the reference's own ``merge_windows`` (tests/golden/g16_sw_*.npz,
devtools/gen_sw_goldens.py), a float64 restatement and the unfused device path; ``segmenter_eval.inference`` /
``val.evaluate_sliding`` against the goldens and, on the real models, the ``forward_lowres`` path against full-resolution
windows; and tools.eval_sliding end to end.  Window 32 for the kernels: a x16 low-res window is 2 x 2 (every tap
clamps), a x4 one 8 x 8."""
import glob
import json
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
# (H, W) merged size, stride, original size (None = the merged size: K11a alone)
SHAPES = [((32, 32), 32, None), ((32, 45), 32, None), ((48, 61), 16, None), ((50, 70), 24, None),
          ((32, 46), 32, (20, 29)), ((32, 45), 32, (50, 61))]


@pytest.fixture(scope="module")
def N():
    from semseg import _native
    _native.lib()
    return _native


def _anchors(H, W, stride, ws=WS):
    from semseg.utils.segmenter_eval import sw_anchors
    return sw_anchors(H, W, ws, stride)


# ---------------------------------------------------------------------------------------------------------------- references
def _merge_fp64(seg, ha, wa, H, W, ws=WS):
    """(B * n_win, C, ws, ws) float64, image-major -> (B, C, H, W): sum of the covering windows / their number"""
    n_win = len(ha) * len(wa)
    B, C = seg.shape[0] // n_win, seg.shape[1]
    s = seg.view(B, n_win, C, ws, ws)
    logit = torch.zeros(B, C, H, W, dtype=torch.float64)
    count = torch.zeros(1, 1, H, W, dtype=torch.float64)
    for k, (a, b) in enumerate((a, b) for a in ha for b in wa):
        logit[:, :, a:a + ws, b:b + ws] += s[:, k]
        count[:, :, a:a + ws, b:b + ws] += 1
    assert bool((count > 0).all())
    return logit / count


def _u_axis(n_in, n_out):
    """ATen's align_corners=False index / lambda rule in float32 (csrc/bilinear_map.h: axis_map_u), r = in / out"""
    r = np.float32(n_in) / np.float32(n_out)
    src = (r * (np.arange(n_out, dtype=np.float32) + np.float32(0.5))).astype(np.float32) - np.float32(0.5)
    src = np.maximum(src, np.float32(0)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    lam = (src - i0.astype(np.float32)).astype(np.float64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, lam


def _resize_fp64(v, size):
    """(B, C, h, w) float64 -> (B, C, H, W): align_corners=False bilinear with the fp32 index rule, fp64 values"""
    (a0, a1, ly), (b0, b1, lx) = _u_axis(v.shape[2], size[0]), _u_axis(v.shape[3], size[1])
    lx, ly = torch.from_numpy(lx), torch.from_numpy(ly)[:, None]
    r0, r1 = v[:, :, a0], v[:, :, a1]
    top = (1 - lx) * r0[..., b0] + lx * r0[..., b1]
    bot = (1 - lx) * r1[..., b0] + lx * r1[..., b1]
    return (1 - ly) * top + ly * bot


def _probs_fp64(seg, ha, wa, shape, ori, flip):
    avg = _merge_fp64(seg.double(), ha, wa, *shape)
    if ori is not None:
        avg = _resize_fp64(avg, ori)
    if flip:
        avg = avg.flip(3)
    return avg.softmax(1)


def _device_probs(N, seg, ha, wa, shape, ori, flip, out=None, accumulate=False):
    if ori is None:
        return N.sw_merge(seg, WS, ha, wa, shape, softmax=True, flip=flip, out=out, accumulate=accumulate)
    return N.sw_finish(N.sw_merge(seg, WS, ha, wa, shape), ori, flip=flip, out=out, accumulate=accumulate)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_merge_fullres_is_the_reference_bit_for_bit(N, path):
    """sequential fp32 adds in anchor order and one fp32 division, contraction off: the reference's ``logit / count``"""
    g = np.load(path)
    seg, want = torch.from_numpy(g["seg_maps"]), torch.from_numpy(g["logit_avg"])
    got = N.sw_merge(seg.to(DEV), WS, g["h_anchors"].tolist(), g["w_anchors"].tolist(), tuple(g["shape"].tolist())).cpu()
    diff = (got - want).abs().max().item()
    print(f"{os.path.basename(path)}: max |avg - reference| {diff:.2e}, {int((got != want).sum())} elements differ")
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("C", [5, 21, 151])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("shape,stride,ori", SHAPES)
def test_merge_softmax_and_finish_vs_fp64(N, C, flip, shape, stride, ori):
    ha, wa = _anchors(*shape, stride)
    B, n_win = 2, len(ha) * len(wa)
    g = torch.Generator().manual_seed(C * 11 + shape[1] + stride + int(flip))
    seg = torch.randn(B * n_win, C, WS, WS, generator=g) * 3
    want = _probs_fp64(seg, ha, wa, shape, ori, flip)
    seg_d = seg.to(DEV)
    got = _device_probs(N, seg_d, ha, wa, shape, ori, flip)
    err = (got.cpu().double() - want).abs().max().item()
    print(f"C={C} {shape} stride {stride} -> {ori} flip={flip}: max |err| {err:.2e}")
    assert tuple(got.shape) == (B, C, *(ori or shape))
    assert err <= 1e-6
    assert torch.equal(_device_probs(N, seg_d, ha, wa, shape, ori, flip), got)      # no atomics: bitwise reproducible
    buf0 = torch.rand(want.shape, generator=g) * 4
    buf = buf0.to(DEV)
    res = _device_probs(N, seg_d, ha, wa, shape, ori, flip, out=buf, accumulate=True)
    assert res.data_ptr() == buf.data_ptr()
    assert (buf.cpu().double() - (buf0.double() + want)).abs().max().item() <= 1e-6
    over = _device_probs(N, seg_d, ha, wa, shape, ori, flip, out=buf)               # without accumulate: overwritten
    assert torch.equal(over, got)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("C", [5, 151])
@pytest.mark.parametrize("r", [4, 16])
@pytest.mark.parametrize("shape,stride,flip", [((32, 45), 32, False), ((48, 61), 16, True), ((50, 70), 24, False)])
def test_merge_lowres_vs_unfused(N, C, r, shape, stride, flip):
    """low-res window logits merged directly == the model's own up-sampling (M2) per window, then the full-res merge"""
    ha, wa = _anchors(*shape, stride)
    B, n_win = 2, len(ha) * len(wa)
    g = torch.Generator().manual_seed(C + r + shape[1])
    low = (torch.randn(B * n_win, C, WS // r, WS // r, generator=g) * 3).to(DEV)
    up = N.upsample_bilinear(low, (WS, WS))
    avg_low, avg_up = N.sw_merge(low, WS, ha, wa, shape), N.sw_merge(up, WS, ha, wa, shape)
    d = (avg_low - avg_up).abs().max().item()
    print(f"C={C} r={r} {shape}: max |avg fused - unfused| {d:.2e}")
    assert torch.equal(avg_low, avg_up)
    got = N.sw_merge(low, WS, ha, wa, shape, softmax=True, flip=flip)
    want = N.sw_merge(up, WS, ha, wa, shape, softmax=True, flip=flip)
    assert (got - want).abs().max().item() <= 1e-6
    plain = avg_up.flip(3) if flip else avg_up
    assert (got - plain.softmax(1)).abs().max().item() <= 1e-6


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("low", [False, True])
def test_image_major_indexing(N, low):
    shape, stride, C = (48, 61), 16, 21
    ha, wa = _anchors(*shape, stride)
    n_win = len(ha) * len(wa)
    assert n_win == 6
    g = torch.Generator().manual_seed(77)
    side = WS // 4 if low else WS
    seg = (torch.randn(2 * n_win, C, side, side, generator=g) * 3).to(DEV)
    for softmax in (False, True):
        both = N.sw_merge(seg, WS, ha, wa, shape, softmax=softmax)
        for b in (0, 1):
            alone = N.sw_merge(seg[b * n_win:(b + 1) * n_win].contiguous(), WS, ha, wa, shape, softmax=softmax)
            assert torch.equal(both[b:b + 1], alone)
    assert not torch.equal(both[0], both[1])


# ---------------------------------------------------------------------------------------------------------------- 5
def test_argument_errors(N):
    seg = torch.randn(2, 5, WS, WS, device=DEV)
    out = torch.full((1, 5, 32, 45), 7.0, device=DEV)
    E = N.SeaNativeError
    with pytest.raises(E):                                                   # 33 anchors on an axis
        N.sw_merge(torch.randn(33, 5, WS, WS, device=DEV), WS, [0], list(range(33)), (32, 64))
    with pytest.raises(E):                                                   # an anchor beyond W - ws
        N.sw_merge(seg, WS, [0], [0, 20], (32, 45), out=out)
    with pytest.raises(E):                                                   # a gap wider than the window
        N.sw_merge(seg, WS, [0], [0, 40], (32, 72))
    with pytest.raises(E):                                                   # C = 193
        N.sw_merge(torch.randn(2, 193, 2, 2, device=DEV), WS, [0], [0, 13], (32, 45))
    with pytest.raises(E):                                                   # CPU tensors
        N.sw_merge(seg.cpu(), WS, [0], [0, 13], (32, 45))
    with pytest.raises(E):
        N.sw_merge(seg, WS, [0], [0, 13], (32, 45), out=out.cpu())
    with pytest.raises(E):                                                   # out aliasing the logits
        N.sw_merge(seg[:1], WS, [0], [0], (32, 32), out=seg[:1])
    with pytest.raises(E):                                                   # windows per image do not divide the rows
        N.sw_merge(torch.randn(3, 5, WS, WS, device=DEV), WS, [0], [0, 13], (32, 45))
    with pytest.raises(E):                                                   # logits larger than the window
        N.sw_merge(torch.randn(2, 5, 33, 33, device=DEV), WS, [0], [0, 13], (32, 45))
    with pytest.raises(E):                                                   # the mirror belongs to the softmax epilogue
        N.sw_merge(seg, WS, [0], [0, 13], (32, 45), flip=True)
    with pytest.raises(E):
        N.sw_merge(seg, WS, [0], [0, 13], (32, 45), softmax=True, accumulate=True)        # nothing to add to
    avg = torch.randn(1, 5, 32, 46, device=DEV)
    with pytest.raises(E):
        N.sw_finish(avg.cpu(), (20, 29))
    with pytest.raises(E):
        N.sw_finish(torch.randn(1, 193, 4, 4, device=DEV), (20, 29))
    with pytest.raises(E):
        N.sw_finish(avg, (32, 46), out=avg)
    with pytest.raises(E):
        N.sw_finish(avg, (20, 29), out=torch.empty(1, 5, 20, 30, device=DEV))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                          # nothing was launched on the refused call


# ---------------------------------------------------------------------------------------------------------------- 6
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


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_inference_and_evaluate_sliding_vs_reference_golden(N, path, monkeypatch):
    from oracle.tiny_models import PointwiseNet, TinyConvNet
    import semseg.val as V
    from semseg.utils.segmenter_eval import inference, merge_windows
    g = np.load(path)
    C, net_name, flip, stride = int(g["n_classes"]), str(g["net"]), bool(int(g["flip"])), int(g["window_stride"])
    net = (TinyConvNet if net_name == "conv" else PointwiseNet)(C, seed=int(g["seed"])).to(DEV)
    x, y, probs = torch.from_numpy(g["x"]), torch.from_numpy(g["y"]), torch.from_numpy(g["probs"])
    H, W = y.shape[-2:]
    # the reference's dictionary, one image: (C, H, W) as there
    n_win = len(g["anchors"])
    win = {"anchors": [tuple(a) for a in g["anchors"].tolist()], "shape": tuple(g["shape"].tolist()), "flip": flip,
           "seg_maps": torch.from_numpy(g["seg_maps"][:n_win]).to(DEV)}
    one = merge_windows(win, WS, (H, W))
    assert tuple(one.shape) == (C, H, W) and (one.cpu() - probs[0]).abs().max().item() <= 1e-6
    win["seg_maps"] = torch.from_numpy(g["seg_maps"]).to(DEV)
    assert (merge_windows(win, WS, (H, W)).cpu() - probs).abs().max().item() <= 1e-6
    # inference: 3 windows per model call, so the chunks straddle the images
    got = inference(net, x.to(DEV), WS, stride, 3, ori_shape=(H, W), n_cls=C, flip=flip)
    err = (got.cpu() - probs).abs().max().item()
    print(f"{os.path.basename(path)}: inference max |p - reference| {err:.2e}")
    assert tuple(got.shape) == (2, C, H, W) and err <= 1e-5
    assert torch.equal(inference(net, x.to(DEV), WS, stride, 64, n_cls=C, flip=flip), got)       # ori_shape defaults to the input's
    # evaluate_sliding: plain (+ mirrored) pass into one score buffer, argmax + confusion matrix
    score_ref = torch.from_numpy(g["score"]) if flip else probs
    rec = _Recorder(monkeypatch)
    m = V._evaluate_sliding_metrics(net, [(x, y)], DEV, WS, stride, flip=flip, n_classes=C, ignore_label=int(g["ignore_label"]))
    # every pass is within 1e-5 of the reference's probabilities; a flip score is the sum of two passes
    assert (rec.scores[0] - score_ref).abs().max().item() <= (2e-5 if flip else 1e-5)
    _compare_hist(rec.scores[0], score_ref, y, m.hist.cpu(), torch.from_numpy(g["hist"]), os.path.basename(path))
    res = V.evaluate_sliding(net, [(x, y)], DEV, WS, stride, batch_size=4, flip=flip, n_classes=C, ignore_label=-1)
    assert len(res) == 6 and len(res[0]) == C and len(res[4]) == C
    assert res[5] == m.compute_iou()[1] and res[1] == m.compute_pixel_acc()[1]


# ---------------------------------------------------------------------------------------------------------------- 7
class _NoHook(torch.nn.Module):
    """the same model with ``forward_lowres`` hidden: full-resolution window logits"""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x):
        return self.model(x)


@pytest.mark.parametrize("cfg,C,size,stride,low", [("ade20k_segmenter.yaml", 151, (64, 96), 64, 4),
                                                   ("pascalvoc_convnext.yaml", 21, (64, 112), 48, 16)])
def test_inference_real_models_lowres_fused(N, cfg, C, size, stride, low, monkeypatch):
    from semseg import _native
    from semseg.utils.segmenter_eval import inference
    from tools.infer import build_model
    with open(os.path.join(PKG, "configs", cfg)) as f:
        conf = yaml.load(f, Loader=yaml.SafeLoader)
    torch.manual_seed(0)
    model = build_model(conf, random_init=True, device=DEV)
    for p in model.parameters():
        p.requires_grad_(False)
    ws, B = 64, 2
    images = torch.rand(B, 3, *size, generator=torch.Generator().manual_seed(C)).to(DEV)
    calls = []
    real = _native.sw_merge

    def spy(logits, *a, **k):
        calls.append(tuple(logits.shape))
        return real(logits, *a, **k)

    monkeypatch.setattr(_native, "sw_merge", spy)

    def run(m):
        inference(m, images, ws, stride, B, n_cls=C)              # warm-up: weight-derived caches are built once
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        p = inference(m, images, ws, stride, B, n_cls=C)
        torch.cuda.synchronize()
        return p, torch.cuda.max_memory_allocated() - base

    fused, peak_fused = run(model)
    assert calls[-1] == (2 * B, C, low, low), calls               # two windows per image, forward_lowres logits
    plain, peak_plain = run(_NoHook(model))
    assert calls[-1] == (2 * B, C, ws, ws), calls
    err = (fused - plain).abs().max().item()
    print(f"{cfg}: max |p fused - p full-res| {err:.2e}; peak above the inputs {peak_fused / 2**20:.2f} MB with the hook, "
          f"{peak_plain / 2**20:.2f} MB without")
    assert tuple(fused.shape) == (B, C, *size)
    assert (fused.sum(1) - 1).abs().max().item() <= 1e-5
    assert err <= 1e-6
    assert peak_fused < peak_plain


# ---------------------------------------------------------------------------------------------------------------- 8
def test_eval_sliding_tool(N, tmp_path, capsys):
    from tools import eval_sliding
    out = tmp_path / "sliding.json"
    cfg = os.path.join(PKG, "configs", "ade20k_segmenter.yaml")
    with open(cfg) as f:
        assert eval_sliding.default_window(yaml.safe_load(f)) == (512, 512)          # configs/segmenter.yml
    eval_sliding.main(["--cfg", cfg, "--synthetic", "4", "--image_size", "64", "96", "--window_size", "64",
                       "--window_stride", "64", "--batch_size", "2", "--json", str(out)])
    r = json.loads(out.read_text())
    assert r["n_images"] == 4 and r["image_size"] == [64, 96] and r["window_size"] == 64 and r["window_stride"] == 64
    assert len(r["IoU"]) == 151 and 0.0 <= r["mIoU"] <= 100.0 and 0.0 <= r["aAcc"] <= 100.0
    assert "mIoU" in capsys.readouterr().out
