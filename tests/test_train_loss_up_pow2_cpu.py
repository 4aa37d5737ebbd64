"""T2u's single-pass kernel for x4 / x16 (csrc/train_loss_up_pow2.hip), CPU side (`-m "not gpu"`): the entry points are
declared, exported and bound, the predicate's truth table, ``upsampled()`` with ``native=False, up_kernel="pow2"`` is the
written-out composition, the kernel switch defaults to "gather" and the tool has ``--fused-kernel``.  Also the shapes that
tests/test_train_loss_up_pow2_gpu.py runs."""
import os
import re
import subprocess

import pytest
import torch

from conftest import PKG, ROOT
from test_train_loss_up_cpu import AUX_SEED, SHAPES, interp, make, recipe

# (C, h, w, H, W): one way each for the kernel to go wrong
POW2_SHAPES = {
    "x4_C5": SHAPES["x4_C5"],                # odd low-resolution sizes
    "x4_C21": SHAPES["x4_C21"],              # VOC class count
    "x4_C151": SHAPES["x4_C151"],            # three slots, x4
    "x16_C40": SHAPES["x16_C40"],            # x16 on a tiny map
    "x16_C151": (151, 2, 2, 32, 32),         # three slots, x16
    "x4_C2": (2, 3, 5, 12, 20),              # minimum class count
    "x4_C64": (64, 3, 3, 12, 12),            # slot boundary 1 -> 2
    "x4_C65": (65, 3, 3, 12, 12),
    "x4_C128": (128, 2, 2, 8, 8),            # slot boundary 2 -> 3
    "x4_C129": (129, 2, 2, 8, 8),
    "x4_C192": (192, 2, 2, 8, 8),            # maximum class count
    "one_row_C21": (21, 1, 3, 4, 12),        # one low-resolution row (clamped borders)
    "one_col_C21": (21, 3, 1, 12, 4),        # one low-resolution column
    "clamped_C21": SHAPES["clamped_C21"],    # every source index clamped
    # a wave walks a segment of 8 cells (x4) or 2 cells (x16) of the w + 1 cells of a cell row: 19 and 21 segments here, so
    # leading partial vectors exist and most columns are flushed by two different waves
    "long_x4_C5": (5, 2, 150, 8, 600),
    "long_x16_C5": (5, 2, 40, 32, 640),
}
SYMBOLS = ("sea_train_ce_up_pow2_supported", "sea_train_ce_up_pow2_workspace_bytes", "sea_train_ce_up_pow2_fwd",
           "sea_train_ce_up_pow2_scale")
TRUTH = {(21, 5, 7, 20, 28): 1, (40, 2, 3, 32, 48): 1, (151, 9, 9, 36, 36): 1, (2, 3, 5, 12, 20): 1, (192, 2, 2, 8, 8): 1,
         (151, 5, 6, 17, 23): 0, (21, 6, 6, 6, 6): 0, (21, 5, 7, 40, 56): 0, (21, 5, 7, 20, 112): 0, (193, 2, 2, 8, 8): 0,
         (1, 2, 2, 8, 8): 0}


@pytest.fixture(scope="module")
def native():
    from semseg import _native
    if not os.path.exists(_native.LIB_PATH):
        import sys
        sys.path.insert(0, PKG)
        import build_native
        build_native.build(verbose=False)
    return _native


def test_entry_points_declared_exported_and_bound(native):
    header = open(os.path.join(ROOT, "include", "sea_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        decl = re.search(r"^(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)", header, flags=re.M)
        assert decl, name
        assert "torch" not in decl.group(1) and "&" not in decl.group(1)
        assert len(decl.group(1).split(",")) == len(native._SIGS[name][1]), name     # arity of the ctypes prototype
        assert re.search(r" T " + name + r"$", out, flags=re.M), name
        assert name in native.EXPORTS
    for fn in ("train_ce_up_pow2_supported", "train_ce_up_pow2_forward", "train_ce_up_pow2_backward"):
        assert callable(getattr(native, fn))
    # the header cites the reference lines each entry replaces
    for cite in ("uperforseg.py:416-434", "segmenter.py:228", "train_rob_seg.py:346-347"):
        assert cite in header, cite


def test_predicate_truth_table(native):
    lib = native.lib()
    for shape, want in TRUTH.items():
        assert lib.sea_train_ce_up_pow2_supported(*shape) == want, shape
        assert (lib.sea_train_ce_up_pow2_workspace_bytes(2, *shape) != 0) == bool(want), shape
        C, h, w, H, W = shape
        assert native.train_ce_up_pow2_supported(torch.empty(2, C, h, w), (H, W)) is bool(want), shape
    assert lib.sea_train_ce_up_pow2_workspace_bytes(0, 21, 5, 7, 20, 28) == 0
    assert not native.train_ce_up_pow2_supported(torch.empty(21, 5, 7), (20, 28))
    # every shape of the GPU tests, so that a change of the predicate shows here first
    for name, shape in POW2_SHAPES.items():
        assert lib.sea_train_ce_up_pow2_supported(*shape) in (0, 1), name


def test_a_refused_call_returns_the_argument_error(native):
    lib = native.lib()
    assert lib.sea_train_ce_up_pow2_fwd(None, None, None, 255, 2, 21, 5, 7, 20, 28, None, None, 0, None, None) == 1
    assert lib.sea_train_ce_up_pow2_scale(None, None, None, None, 10, None) == 1
    low, y, _ = recipe(SHAPES["x4_C5"])
    with pytest.raises(native.SeaNativeError):         # CPU tensors: no fallback
        native.train_ce_up_pow2_forward(low, y.shape[-2:], y, None, 255)


@pytest.mark.parametrize("kind", ["ce", "ce_w", "ohem"])
def test_upsampled_plain_with_pow2_is_the_composition_on_cpu(kind):
    from semseg.losses import CrossEntropy, OhemCrossEntropy, get_loss
    low, y, weights = recipe(SHAPES["x4_C5"])
    aux = recipe(SHAPES["x4_C5"], seed=AUX_SEED)[0]
    cls = OhemCrossEntropy if kind == "ohem" else CrossEntropy
    mod = cls(255, weights if kind == "ce_w" else None, native=False, up_kernel="pow2")
    ref = make("ohem" if kind == "ohem" else "ce", 255, weights if kind == "ce_w" else None)
    assert mod.up_kernel == "pow2" and ref.up_kernel == "gather"
    for preds in ((low,), (low, aux)):
        a = [p.clone().requires_grad_(True) for p in preds]
        b = [p.clone().requires_grad_(True) for p in preds]
        la = mod.upsampled(tuple(a) if len(a) > 1 else a[0], y)
        up = [interp(p, y) for p in b]
        lb = ref(tuple(up) if len(up) > 1 else up[0], y)
        la.backward()
        lb.backward()
        assert torch.isfinite(la) and torch.equal(la, lb)
        for p, q in zip(a, b):
            assert bool((p.grad != 0).any()) and torch.equal(p.grad, q.grad)
    assert get_loss("CrossEntropy", -1, None, native=False, up_kernel="pow2").up_kernel == "pow2"
    assert get_loss("OhemCrossEntropy", -1, None, up_kernel="pow2").up_kernel == "pow2"
    assert get_loss("CrossEntropy").up_kernel == "gather"
    with pytest.raises(ValueError):
        CrossEntropy(up_kernel="scatter")


def test_native_pow2_refuses_cpu_tensors(native):
    from semseg.losses import CrossEntropy
    low, y, _ = recipe(SHAPES["x4_C5"])
    with pytest.raises(native.SeaNativeError):
        CrossEntropy(255, native=True, up_kernel="pow2").upsampled(low, y)


def test_kernel_switch_defaults_to_gather_and_the_tool_has_the_flag():
    import importlib.util
    assert os.environ.get("SEA_TRAIN_FUSED_KERNEL", "gather") == "gather"
    from semseg.models import convnext_upernet as M
    assert M.TRAIN_FUSED_KERNEL == "gather" and M._fused_criterion().up_kernel == "gather"
    src = open(os.path.join(PKG, "tools", "train_rob_seg.py")).read()
    assert '"--fused-kernel"' in src and '"fused_kernel"' in src
    spec = importlib.util.spec_from_file_location("train_rob_seg_pow2", os.path.join(PKG, "tools", "train_rob_seg.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert callable(tool.segmenter_loss) and tool.build_fused_criterion("pow2").up_kernel == "pow2"
    with pytest.raises(OSError):           # the flags are parsed and set, then the missing config file ends the run
        tool.main(["--cfg", os.path.join(ROOT, "no_such_config.yaml"), "--fused-criterion", "--fused-kernel", "pow2"])
    assert M.TRAIN_FUSED_CRITERION is False and M.TRAIN_FUSED_KERNEL == "gather"      # ... and main() restored both
    with pytest.raises(SystemExit):
        tool.main(["--fused-kernel", "scatter"])


def test_segmenter_forward_has_the_lowres_argument():
    import inspect
    from semseg.models.segmenter import SegMenter
    sig = inspect.signature(SegMenter.forward)
    assert list(sig.parameters) == ["self", "im", "lowres"] and sig.parameters["lowres"].default is False
