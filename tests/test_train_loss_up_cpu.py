"""T2u, the training criteria fused with the final up-sampling, CPU side (`-m "not gpu"`): ``upsampled()`` with
``native=False`` is the written-out composition, the three entry points are declared, exported and bound, and the model
switch is off by default.  Also the input recipe, the shapes and the float64 yardstick that tests/test_train_loss_up_gpu.py
uses, with the check that the yardstick's OHEM selection is unambiguous for every shape (so the GPU test's precondition is
known to hold before any device runs)."""
import math
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from conftest import PKG, ROOT

B = 2
# (C, h, w, H, W): one way each for the kernels to go wrong (the issue's table)
SHAPES = {
    "x4_C5": (5, 5, 7, 20, 28),            # x4 (UperNet), odd low-resolution sizes
    "x4_C21": (21, 5, 7, 20, 28),          # VOC class count
    "x16_C40": (40, 2, 3, 32, 48),         # x16, map smaller than any tile, C > 32
    "frac_C151": (151, 5, 6, 17, 23),      # non-integer ratio, ADE class count
    "x4_C151": (151, 9, 9, 36, 36),        # several blocks at C = 151 (tile edge 6), eight classes per thread
    "clamped_C21": (21, 1, 1, 4, 4),       # every source index clamped
    "ratio1_C21": (21, 6, 6, 6, 6),        # ratio 1: T2's problem
    "halo_C21": None,                      # one pixel more than the launcher's tile edge: resolved by shape_of()
}
THRESHOLDS = (0.7, 0.05, 1e-9)
# The auxiliary prediction of the tuple cases: the recipe's logits from another seed, with the labels of seed 0.  Seed 1 puts a
# pixel of the 5-class shape 7.8e-5 from the threshold -log 0.7 in float64, inside the 1e-4 the selection check asks for; seed
# 2 is the first that keeps every shape outside it (smallest gaps 4.6e-3 to the threshold, 4.8e-4 between the ranks).
AUX_SEED = 2
SYMBOLS = ("sea_train_ce_up_workspace_bytes", "sea_train_ce_up_fwd", "sea_train_ce_up_bwd")


@pytest.fixture(scope="module")
def native():
    from semseg import _native
    if not os.path.exists(_native.LIB_PATH):
        import sys
        sys.path.insert(0, PKG)
        import build_native
        build_native.build(verbose=False)
    return _native


def shape_of(name):
    """the halo shape reads the tile edge from the launcher: a x4 map one pixel wider and taller than the tile for C = 21
    (two blocks per axis, the second a one-pixel remainder tile)"""
    if SHAPES[name] is not None:
        return SHAPES[name]
    from semseg import _native as N
    for t in range(1, 65):
        if N.train_ce_up_tile(21, t + 1, t + 1, 4 * (t + 1), 4 * (t + 1)) == t:
            return (21, t + 1, t + 1, 4 * (t + 1), 4 * (t + 1))
    raise AssertionError("no x4 shape one pixel larger than its tile")


def recipe(shape, ignore=255, seed=0):
    """the issue's input recipe, in its order; class weights are drawn last"""
    C, h, w, H, W = shape
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(B, C, h, w, generator=g) * 2
    y = torch.randint(0, C, (B, H, W), generator=g)
    y[torch.rand(B, H, W, generator=g) < 0.1] = 255
    weights = torch.rand(C, generator=g) + 0.5
    if ignore != 255:
        y[y == 255] = ignore
    return low, y, weights


def interp(p, y):
    return F.interpolate(p, y.shape[-2:], mode="bilinear", align_corners=False)


def make(kind, ignore, weights=None, native=False, thresh=0.7):
    from semseg.losses import CrossEntropy, OhemCrossEntropy
    if kind == "ohem":
        return OhemCrossEntropy(ignore, weights, thresh=thresh, native=native)
    return CrossEntropy(ignore, weights, native=native)


def f64_pixel_losses(low, y, ignore, weights=None):
    z = interp(low.double(), y)
    return F.cross_entropy(z, y, None if weights is None else weights.double(), ignore_index=ignore, reduction="none")


def ohem_yardstick(low, y, ignore, thresh):
    """(n_min, n_sel, mode, selection gaps) of the float64 criterion; thresh: the module's fp32 threshold -log(p)"""
    px = f64_pixel_losses(low, y, ignore).view(-1)
    valid = (y != ignore).view(-1)
    n_min = int(valid.sum()) // 16
    t = float(-torch.log(torch.tensor(thresh, dtype=torch.float)))
    n_hard = int((px > t).sum())
    mode = 1 if n_hard < n_min else 0
    gap_t = float((px[valid] - t).abs().min()) if bool(valid.any()) else math.inf
    srt = px.sort(descending=True).values
    gap_rank = float(srt[n_min - 1] - srt[n_min]) if 0 < n_min < srt.numel() else math.inf
    return n_min, (n_min if mode else n_hard), mode, gap_t, gap_rank


def assert_selection_unambiguous(low, y, ignore, thresh):
    n_min, n_sel, mode, gap_t, gap_rank = ohem_yardstick(low, y, ignore, thresh)
    assert gap_t > 1e-4, gap_t
    assert gap_rank == 0.0 or gap_rank > 1e-4, gap_rank
    return n_min, n_sel, mode


@pytest.mark.parametrize("name", list(SHAPES))
def test_recipe_gives_an_unambiguous_ohem_selection(native, name):
    low, y, _ = recipe(shape_of(name))
    modes = [assert_selection_unambiguous(low, y, 255, t)[2] for t in THRESHOLDS]
    assert modes[-1] == 1, modes           # 1e-9: nothing is hard, the regime is top-k
    if name not in ("clamped_C21",):       # (32 pixels, n_min = 1: any regime)
        assert modes[0] == 0, modes


@pytest.mark.parametrize("name", list(SHAPES))
def test_auxiliary_prediction_gives_an_unambiguous_ohem_selection(native, name):
    shape = shape_of(name)
    assert_selection_unambiguous(recipe(shape, seed=AUX_SEED)[0], recipe(shape)[1], 255, 0.7)


@pytest.mark.parametrize("kind", ["ce", "ce_w", "ohem"])
def test_upsampled_plain_is_the_composition_on_cpu(kind):
    low, y, weights = recipe(SHAPES["x4_C5"])
    aux = recipe(SHAPES["x4_C5"], seed=AUX_SEED)[0]
    mod = make("ohem" if kind == "ohem" else "ce", 255, weights if kind == "ce_w" else None)
    for preds in ((low,), (low, aux)):
        a = [p.clone().requires_grad_(True) for p in preds]
        b = [p.clone().requires_grad_(True) for p in preds]
        la = mod.upsampled(tuple(a) if len(a) > 1 else a[0], y)
        up = [interp(p, y) for p in b]
        lb = mod(tuple(up) if len(up) > 1 else up[0], y)
        la.backward()
        lb.backward()
        assert torch.isfinite(la) and torch.equal(la, lb)
        for p, q in zip(a, b):
            assert bool((p.grad != 0).any()) and torch.equal(p.grad, q.grad)


def test_upsampled_native_refuses_cpu_tensors_and_dice_has_no_such_method(native):
    from semseg.losses import Dice
    low, y, _ = recipe(SHAPES["x4_C5"])
    for kind in ("ce", "ohem"):
        with pytest.raises(native.SeaNativeError):
            make(kind, 255, native=True).upsampled(low, y)
        with pytest.raises(native.SeaNativeError):
            make(kind, 255, native=True).upsampled((low, low), y)
    assert not hasattr(Dice(), "upsampled")
    with pytest.raises(native.SeaNativeError):
        native.train_ce_up_forward(low, y.shape[-2:], y, None, 255)


def test_entry_points_declared_exported_and_bound(native):
    header = open(os.path.join(ROOT, "include", "sea_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS + ("sea_train_ce_up_tile",):
        decl = re.search(r"^(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)", header, flags=re.M)
        assert decl, name
        assert "torch" not in decl.group(1) and "&" not in decl.group(1)
        assert len(decl.group(1).split(",")) == len(native._SIGS[name][1]), name     # arity of the ctypes prototype
        assert re.search(r" T " + name + r"$", out, flags=re.M), name
    lib = native.lib()
    assert lib.sea_abi_version() == 3
    # T2's select area, then one record per tile: 9 x 9 at tile edge 8 is 2 x 2 tiles per image
    tile = native.train_ce_up_tile(21, 9, 9, 36, 36)
    assert tile >= 1
    tiles = (-(-9 // tile)) ** 2
    assert lib.sea_train_ce_up_workspace_bytes(2, 21, 9, 9, 36, 36) == 4096 + 16 * 1024 + 2 * tiles * 32
    # class-count limits and down-sampling: no plan, and the argument error before any launch
    for C in (1, 193, 200):
        assert lib.sea_train_ce_up_workspace_bytes(2, C, 9, 9, 36, 36) == 0 and native.train_ce_up_tile(C, 9, 9, 36, 36) == 0
    assert lib.sea_train_ce_up_workspace_bytes(2, 21, 9, 9, 8, 36) == 0
    assert lib.sea_train_ce_up_workspace_bytes(0, 21, 9, 9, 36, 36) == 0
    assert lib.sea_train_ce_up_fwd(None, None, None, 255, 0.0, 1, 2, 21, 9, 9, 36, 36, None, None, 0, None, None) == 1
    assert lib.sea_train_ce_up_bwd(None, None, None, 255, 0, 2, 21, 9, 9, 36, 36, None, None, None, None, None, 0, None) == 1
    # the LDS plan: at most 64 KB for the backward whatever C
    for C in (2, 21, 95, 96, 151, 192):
        for (h, H) in ((16, 64), (8, 128), (5, 17)):
            assert 1 <= native.train_ce_up_tile(C, h, h, H, H) <= 8, (C, h, H)


def test_switch_defaults_to_off_and_the_tool_has_the_flag():
    import importlib.util
    assert os.environ.get("SEA_TRAIN_FUSED_LOSS", "0") in ("", "0")
    from semseg.models import convnext_upernet as M
    assert M.TRAIN_FUSED_CRITERION is False
    src = open(os.path.join(PKG, "tools", "train_rob_seg.py")).read()
    assert '"--fused-criterion"' in src and '"fused_criterion"' in src
    spec = importlib.util.spec_from_file_location("train_rob_seg_t2u", os.path.join(PKG, "tools", "train_rob_seg.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with pytest.raises(OSError):           # the flag is parsed and set, then the missing config file ends the run
        tool.main(["--cfg", os.path.join(ROOT, "no_such_config.yaml"), "--fused-criterion"])
    assert M.TRAIN_FUSED_CRITERION is False       # ... and main() restored the switch
