"""T2u-ac, the training criteria fused with PSPNet's align_corners=True up-sampling, CPU side (`-m "not gpu"`):
``upsampled(..., align_corners=True)`` with ``native=False`` is the written-out composition and the default is unchanged, the
four entry points are declared, exported and bound, the plan accepts the shapes it must and refuses the ones it must, the
PSPNet switch is ``torch`` by default and the tool restores it.  Also the shapes and the float64 yardstick that
tests/test_train_loss_up_ac_gpu.py uses (the input recipe is tests/test_train_loss_up_cpu.py's, imported), with the check
that the yardstick's OHEM selection is unambiguous for every shape and both seeds."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import PKG, ROOT
from test_train_loss_up_cpu import AUX_SEED, B, THRESHOLDS, make, recipe

# (C, h, w, H, W): the issue's table
SHAPES = {
    "x8_C21": (21, 5, 8, 33, 57),          # PSPNet's relation H - 1 = 8 (h - 1), VOC classes, non-square
    "x8_C5": (5, 4, 3, 25, 17),            # fewer classes than a chunk
    "x8_C40": (40, 2, 3, 9, 17),           # map smaller than any tile, C > 32
    "x8_C151": (151, 5, 5, 33, 33),        # ADE class count, smaller tile edge
    "frac_C21": (21, 5, 6, 17, 23),        # non-integer ratio: the inverse map's rounding
    "psp65_C21": (21, 9, 9, 65, 65),       # the size of the 65 x 65 golden: several tiles
    "one_C21": (21, 1, 1, 4, 4),           # n_in == 1: scale 0
    "ratio1_C21": (21, 6, 6, 6, 6),        # identity map: T2's problem
    "halo_C21": None,                      # x8 map one pixel wider and taller than the tile edge: resolved by shape_of()
}
PSP_SHAPE = (21, 60, 60, 473, 473)         # PSPNet-ResNet50 on a VOC crop
SYMBOLS = ("sea_train_ce_up_ac_tile", "sea_train_ce_up_ac_workspace_bytes", "sea_train_ce_up_ac_fwd",
           "sea_train_ce_up_ac_bwd")


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
    """the halo shape reads the tile edge from the launcher: a x8 map (H - 1 = 8 (h - 1)) one low-resolution pixel wider and
    taller than the tile for C = 21 (two blocks per axis, the second a one-pixel remainder tile)"""
    if SHAPES[name] is not None:
        return SHAPES[name]
    from semseg import _native as N
    for t in range(1, 65):
        shape = (21, t + 1, t + 1, 8 * t + 1, 8 * t + 1)
        if N.train_ce_up_tile(*shape, align_corners=True) == t:
            return shape
    raise AssertionError("no x8 shape one pixel larger than its tile")


def exact_weights(shape):
    """whether the bilinear weights are exact in fp32 and float64 alike: scale (n_in - 1) / (n_out - 1) a power of two, or 0"""
    _, h, w, H, W = shape

    def exact(n_in, n_out):
        if n_in == 1:
            return True
        q, r = divmod(n_out - 1, n_in - 1)
        return r == 0 and q & (q - 1) == 0
    return exact(h, H) and exact(w, W)


def interp(p, y):
    return F.interpolate(p, y.shape[-2:], mode="bilinear", align_corners=True)


def ohem_yardstick(low, y, ignore, thresh):
    """tests/test_train_loss_up_cpu.py's, on the align_corners=True interpolation"""
    px = F.cross_entropy(interp(low.double(), y), y, ignore_index=ignore, reduction="none").view(-1)
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


@pytest.mark.parametrize("seed", [0, AUX_SEED])
@pytest.mark.parametrize("name", list(SHAPES))
def test_recipe_gives_an_unambiguous_ohem_selection(native, name, seed):
    """the precondition of the GPU file, for the main (seed 0) and the auxiliary (AUX_SEED, labels of seed 0) prediction"""
    shape = shape_of(name)
    low, y = recipe(shape, seed=seed)[0], recipe(shape)[1]
    modes = [assert_selection_unambiguous(low, y, 255, t)[2] for t in THRESHOLDS]
    assert modes[-1] == 1, modes           # 1e-9: nothing is hard, the regime is top-k


def test_halo_shape_is_one_pixel_larger_than_its_tile(native):
    C, h, w, H, W = shape_of("halo_C21")
    tile = native.train_ce_up_tile(C, h, w, H, W, align_corners=True)
    assert h == w == tile + 1 and H - 1 == 8 * (h - 1) and W - 1 == 8 * (w - 1)
    assert exact_weights((C, h, w, H, W)) and not exact_weights(SHAPES["frac_C21"])


@pytest.mark.parametrize("kind", ["ce", "ce_w", "ohem"])
def test_upsampled_plain_is_the_composition_on_cpu(kind):
    low, y, weights = recipe(SHAPES["x8_C5"])
    aux = recipe(SHAPES["x8_C5"], seed=AUX_SEED)[0]
    mod = make("ohem" if kind == "ohem" else "ce", 255, weights if kind == "ce_w" else None)
    for preds in ((low,), (low, aux)):
        a = [p.clone().requires_grad_(True) for p in preds]
        b = [p.clone().requires_grad_(True) for p in preds]
        la = mod.upsampled(tuple(a) if len(a) > 1 else a[0], y, align_corners=True)
        up = [interp(p, y) for p in b]
        lb = mod(tuple(up) if len(up) > 1 else up[0], y)
        la.backward()
        lb.backward()
        assert torch.isfinite(la) and torch.equal(la, lb)
        for p, q in zip(a, b):
            assert bool((p.grad != 0).any()) and torch.equal(p.grad, q.grad)


@pytest.mark.parametrize("kind", ["ce", "ohem"])
def test_default_is_align_corners_false(kind):
    low, y, _ = recipe(SHAPES["x8_C5"])
    mod = make(kind, 255)
    want = mod(F.interpolate(low, y.shape[-2:], mode="bilinear", align_corners=False), y)
    assert torch.equal(mod.upsampled(low, y), want) and torch.equal(mod.upsampled(low, y, align_corners=False), want)
    assert not torch.equal(mod.upsampled(low, y, align_corners=True), want)      # (the two rules do differ on this shape)


def test_upsampled_native_refuses_cpu_tensors(native):
    low, y, _ = recipe(SHAPES["x8_C5"])
    for kind in ("ce", "ohem"):
        with pytest.raises(native.SeaNativeError):
            make(kind, 255, native=True).upsampled(low, y, align_corners=True)
        with pytest.raises(native.SeaNativeError):
            make(kind, 255, native=True).upsampled((low, low), y, align_corners=True)
    with pytest.raises(native.SeaNativeError):
        native.train_ce_up_forward(low, y.shape[-2:], y, None, 255, align_corners=True)


def test_entry_points_declared_exported_and_bound(native):
    header = open(os.path.join(ROOT, "include", "sea_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        decl = re.search(r"^(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)", header, flags=re.M)
        twin = re.search(r"^(?:int|size_t)\s+" + name.replace("_ac_", "_") + r"\s*\(([^)]*)\)", header, flags=re.M)
        assert decl and twin, name
        args = lambda m: [" ".join(a.split()) for a in m.group(1).split(",")]   # noqa: E731
        assert args(decl) == args(twin), name                      # the argument list of the align_corners=False twin
        assert name in native.EXPORTS and native._SIGS[name] == native._SIGS[name.replace("_ac_", "_")]
        assert re.search(r" T " + name + r"$", out, flags=re.M), name
    lib = native.lib()
    assert lib.sea_abi_version() == 3
    assert lib.sea_train_ce_up_ac_fwd(None, None, None, 255, 0.0, 1, 2, 21, 9, 9, 65, 65, None, None, 0, None, None) == 1
    assert lib.sea_train_ce_up_ac_bwd(None, None, None, 255, 0, 2, 21, 9, 9, 65, 65, None, None, None, None, None, 0,
                                      None) == 1


def test_plan(native):
    for name in SHAPES:
        C, h, w, H, W = shape_of(name)
        tile = native.train_ce_up_tile(C, h, w, H, W, align_corners=True)
        assert 1 <= tile <= 8, (name, tile)
        tiles = -(-h // tile) * -(-w // tile)
        # T2's select area, then one record per tile (the layout of the align_corners=False entry point)
        assert native.lib().sea_train_ce_up_ac_workspace_bytes(B, C, h, w, H, W) == 4096 + 16 * 1024 + B * tiles * 32
        assert native.train_ce_up_supported(torch.empty(B, C, h, w), (H, W), align_corners=True)
    assert 1 <= native.train_ce_up_tile(*PSP_SHAPE, align_corners=True) <= 8
    assert native.lib().sea_train_ce_up_ac_workspace_bytes(8, *PSP_SHAPE) > 0
    assert native.train_ce_up_tile(*SHAPES["x8_C151"], align_corners=True) \
        < native.train_ce_up_tile(*SHAPES["x8_C21"], align_corners=True)
    assert -(-9 // native.train_ce_up_tile(*SHAPES["psp65_C21"], align_corners=True)) >= 2      # several tiles
    for C in (1, 193):
        assert native.train_ce_up_tile(C, 9, 9, 65, 65, align_corners=True) == 0
        assert native.lib().sea_train_ce_up_ac_workspace_bytes(2, C, 9, 9, 65, 65) == 0
        assert not native.train_ce_up_supported(torch.empty(2, C, 9, 9), (65, 65), align_corners=True)
    assert native.train_ce_up_tile(21, 9, 9, 8, 65, align_corners=True) == 0          # H < h
    assert native.train_ce_up_tile(21, 9, 9, 65, 8, align_corners=True) == 0
    assert native.lib().sea_train_ce_up_ac_workspace_bytes(0, 21, 9, 9, 65, 65) == 0
    # one source pixel: every output pixel is in the one tile's region, which the plan has to hold
    assert native.train_ce_up_tile(21, 1, 1, 32, 32, align_corners=True) >= 1
    assert native.train_ce_up_tile(21, 1, 1, 73, 73, align_corners=True) == 0
    # the LDS plan: a tile for every class count at PSPNet's x8 and at a fractional ratio
    for C in (2, 21, 95, 96, 151, 192):
        for (h, H) in ((9, 65), (60, 473), (5, 17)):
            assert 1 <= native.train_ce_up_tile(C, h, h, H, H, align_corners=True) <= 8, (C, h, H)
    # the align_corners=False plan is what it was
    assert native.train_ce_up_tile(21, 9, 9, 36, 36) == native.train_ce_up_tile(21, 9, 9, 36, 36, align_corners=False) == 8


def test_switch_defaults_to_torch_and_the_tool_restores_it():
    import importlib.util
    assert os.environ.get("SEA_PSP_TRAIN_CRITERION", "") in ("", "torch")
    from semseg.models import pspnet
    assert pspnet.TRAIN_CRITERION == "torch" and pspnet.TRAIN_CRITERIA == ("torch", "native", "fused")
    spec = importlib.util.spec_from_file_location("train_rob_seg_t2u_ac", os.path.join(PKG, "tools", "train_rob_seg.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for flags in (["--fused-criterion"], ["--native-criterion"], ["--native-criterion", "--fused-criterion"],
                  ["--fused-criterion", "--fused-kernel", "pow2"]):
        with pytest.raises(OSError):       # the flags are parsed and set, then the missing config file ends the run
            tool.main(["--cfg", os.path.join(ROOT, "no_such_config.yaml")] + flags)
        assert pspnet.TRAIN_CRITERION == "torch"      # ... and main() restored the switch


def test_switch_refuses_an_unknown_value():
    env = dict(os.environ, SEA_PSP_TRAIN_CRITERION="fast", PYTHONPATH=PKG)
    run = subprocess.run([sys.executable, "-c", "import semseg.models.pspnet"], env=env, capture_output=True, text=True)
    assert run.returncode != 0 and "SEA_PSP_TRAIN_CRITERION" in run.stderr
    env["SEA_PSP_TRAIN_CRITERION"] = "fused"
    run = subprocess.run([sys.executable, "-c", "import semseg.models.pspnet as p; print(p.TRAIN_CRITERION)"], env=env,
                         capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "fused", run.stderr


def test_pspnet_still_has_no_forward_lowres():
    from semseg.models import PSPNet
    assert not hasattr(PSPNet(50, 21), "forward_lowres")
