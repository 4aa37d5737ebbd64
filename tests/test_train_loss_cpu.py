"""T2, the training criteria on the device, CPU side (`-m "not gpu"`): the entry points are exported and declared, the
``native`` keyword exists and refuses CPU tensors, and the g17 fixtures of the reference are reproduced by the plain
PyTorch modules (``native=False``) on CPU, which pins the fixtures to this torch."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG, ROOT

FILES = sorted(glob.glob(os.path.join(GOLDEN, "g17_train_loss_*.npz")))
SYMBOLS = ("sea_train_ce_workspace_bytes", "sea_train_ce_fwd", "sea_train_ohem_select", "sea_train_ce_bwd")


def load_case(path):
    """(kind, ignore_label, weights or None, aux weights, labels int64, [pred fp32], [grad], loss, fixture)"""
    g = np.load(path)
    preds, grads = [], []
    k = 0
    while f"pred{k}_bf16bits" in g.files:
        bits = g[f"pred{k}_bf16bits"].astype(np.uint32) << 16
        preds.append(torch.from_numpy(bits.view(np.float32).copy()))
        grads.append(torch.from_numpy(g[f"grad{k}"]))
        k += 1
    w = torch.from_numpy(g["weights"]) if g["weights"].size else None
    return dict(ohem=bool(g["ohem"]), ignore=int(g["ignore_label"]), weights=w, aux=[float(a) for a in g["aux_weights"]],
                labels=torch.from_numpy(g["labels"].astype(np.int64)), preds=preds, grads=grads,
                loss=torch.from_numpy(g["loss"]), regime=int(g["regime"]), n_sel=[int(v) for v in g["n_sel"]],
                n_min=[int(v) for v in g["n_min"]])


def make_module(case, native, device=None):
    from semseg.losses import CrossEntropy, OhemCrossEntropy
    w = case["weights"]
    if w is not None and device is not None:
        w = w.to(device)
    return (OhemCrossEntropy if case["ohem"] else CrossEntropy)(case["ignore"], w, native=native)


def run_module(mod, preds, labels):
    leaves = [p.clone().requires_grad_(True) for p in preds]
    loss = mod(tuple(leaves) if len(leaves) > 1 else leaves[0], labels)
    loss.backward()
    return loss.detach(), [p.grad for p in leaves]


@pytest.fixture(scope="module")
def native():
    from semseg import _native
    if not os.path.exists(_native.LIB_PATH):
        import sys
        sys.path.insert(0, PKG)
        import build_native
        build_native.build(verbose=False)
    return _native


def test_g17_fixtures_cover_the_cases():
    assert len(FILES) == 84, len(FILES)
    seen = set()
    for f in FILES:
        c = load_case(f)
        C = c["preds"][0].shape[1]
        hw = (12, 10) if (C == 151 and len(c["preds"]) == 2) else (24, 20)   # the C = 151 2-tuples are smaller (file size)
        assert c["preds"][0].shape == (2, C) + hw and c["labels"].shape == (2,) + hw
        assert os.path.getsize(f) < 900 * 1024
        seen.add((C, c["ignore"], c["weights"] is not None, len(c["preds"]), c["ohem"], c["regime"]))
    assert {s[0] for s in seen} == {5, 21, 151} and {s[1] for s in seen} == {255, -1}
    assert {s[5] for s in seen if s[4]} == {0, 1, 2} and {s[3] for s in seen} == {1, 2}
    assert {s[2] for s in seen} == {False, True}
    for C in (5, 21, 151):   # every class count: both ignore labels x with / without weights x single / 2-tuple
        assert {s[1:4] for s in seen if s[0] == C} == {(i, w, n) for i in (255, -1) for w in (False, True) for n in (1, 2)}


def test_train_symbols_exported_and_declared(native):
    header = open(os.path.join(ROOT, "include", "sea_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        decl = re.search(r"^(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)", header, flags=re.M)
        assert decl, name
        assert "torch" not in decl.group(1) and "&" not in decl.group(1)
        assert name in native.EXPORTS
        assert re.search(r" T " + name + r"$", out, flags=re.M), name
    assert "semseg/losses.py:6-63" in header
    lib = native.lib()
    # records of the smallest tile (256 pixels) behind the fixed select area
    assert lib.sea_train_ce_workspace_bytes(8, 512 * 512) == 4096 + 16 * 1024 + 8 * 1024 * 32
    assert lib.sea_train_ce_workspace_bytes(0, 4) == 0
    # argument checks fire on the host before any launch
    assert lib.sea_train_ce_fwd(None, 0, None, None, 255, 0.0, 1, 1, 5, 16, None, None, 0, None, None) == 1
    assert lib.sea_train_ohem_select(None, 16, None, 0, None, None) == 1
    assert lib.sea_train_ce_bwd(None, 0, None, None, 255, 0, 1, 5, 16, None, None, None, None, None) == 1


def test_native_keyword_refuses_cpu_tensors(native):
    from semseg.losses import CrossEntropy, Dice, OhemCrossEntropy, get_loss
    z, y = torch.randn(1, 5, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    for name, cls in (("CrossEntropy", CrossEntropy), ("OhemCrossEntropy", OhemCrossEntropy)):
        mod = get_loss(name, 255, None, native=True)
        assert isinstance(mod, cls) and mod.native and mod.criterion.ignore_index == 255
        with pytest.raises(native.SeaNativeError):
            mod(z, y)
        with pytest.raises(native.SeaNativeError):
            mod((z, z), y)
        assert not get_loss(name, 255, None).native
        assert torch.isfinite(get_loss(name, 255, None)(z, y))          # the default stays plain torch on CPU
    assert isinstance(get_loss("Dice", native=True), Dice)
    with pytest.raises(native.SeaNativeError):
        native.train_ce_forward(z, y, None, 255)


def test_train_tool_builds_the_criterion_from_the_config():
    """--native-criterion: the Segmenter branch's criterion is get_loss(cfg LOSS.NAME, -1, None, native=True)"""
    import importlib.util
    from semseg.losses import CrossEntropy, OhemCrossEntropy
    spec = importlib.util.spec_from_file_location("train_rob_seg_t2", os.path.join(PKG, "tools", "train_rob_seg.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for name, cls in (("CrossEntropy", CrossEntropy), ("OhemCrossEntropy", OhemCrossEntropy)):
        mod = tool.build_criterion({"LOSS": {"NAME": name, "CLS_WEIGHTS": False}}, native=True)
        assert isinstance(mod, cls) and mod.native and mod.criterion.ignore_index == -1 and mod.criterion.weight is None
    assert isinstance(tool.build_criterion({}, native=True), CrossEntropy)
    assert tool.build_criterion({"LOSS": {"NAME": "OhemCrossEntropy"}}, native=False) is None


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[15:-4] for f in FILES])
def test_plain_modules_reproduce_the_reference(path):
    c = load_case(path)
    mod = make_module(c, native=False)
    assert mod.aux_weights[:len(c["aux"])] == c["aux"]
    loss, grads = run_module(mod, c["preds"], c["labels"])
    torch.testing.assert_close(loss, c["loss"], rtol=1e-6, atol=0, equal_nan=True)
    for got, want in zip(grads, c["grads"]):
        torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-12, equal_nan=True)
    if c["regime"] == 2:   # every label ignored: NaN loss, and torch's gradient is all zeros (no NaN)
        assert torch.isnan(loss) and all(bool((gr == 0).all()) for gr in c["grads"])
