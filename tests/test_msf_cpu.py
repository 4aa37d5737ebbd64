"""Multi-scale + flip evaluation, CPU side (`-m "not gpu"`): the reference goldens load, the scaled-size rule matches
the reference's on the fixture sizes, and the K10 entry points are exported with plain-C signatures."""
import ctypes as C
import glob
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT

FILES = sorted(glob.glob(os.path.join(GOLDEN, "g15_msf_*.npz")))


@pytest.fixture(scope="module")
def native():
    from semseg import _native
    if not os.path.exists(_native.LIB_PATH):
        import sys
        sys.path.insert(0, PKG)
        import build_native
        build_native.build(verbose=False)
    return _native


def test_g15_fixtures_load():
    assert len(FILES) == 8, FILES
    sizes, flips, classes = set(), set(), set()
    for f in FILES:
        g = np.load(f)
        x, y, sl, hist = g["x"], g["y"], g["scaled_logits"], g["hist"]
        nb, B, _, H, W = x.shape
        C = int(g["n_classes"])
        assert y.shape == (nb, B, H, W) and sl.shape == (nb, B, C, H, W) and hist.shape == (C, C)
        assert sl.dtype == np.float32 and np.isfinite(sl).all()
        n_pass = len(g["scales"]) * (2 if int(g["flip"]) else 1)
        # every pass adds a softmax: the class sum of the accumulated scores is the number of passes
        np.testing.assert_allclose(sl.sum(2), n_pass, rtol=0, atol=1e-4 * n_pass)
        assert hist.sum() == (y != int(g["ignore_label"])).sum()
        assert "values to unpack" in str(g["ref_error"])          # the reference's compute_pixel_acc unpack
        sizes.add((H, W))
        flips.add(int(g["flip"]))
        classes.add(C)
    assert flips == {0, 1} and classes == {5, 21}
    assert any(h == w for h, w in sizes) and any(h % 2 and w % 2 for h, w in sizes)


def _ref_rule(scale, H, W):
    new_H, new_W = int(scale * H), int(scale * W)
    return int(math.ceil(new_H / 32)) * 32, int(math.ceil(new_W / 32)) * 32


def test_scaled_size_matches_reference_rule():
    from semseg.val import msf_scaled_size
    cases = set()
    for f in FILES:
        g = np.load(f)
        H, W = g["x"].shape[-2:]
        for s in g["scales"]:
            cases.add((float(s), int(H), int(W)))
    for s in (0.5, 0.75, 1.0, 1.25, 1.5, 1.75):
        cases |= {(s, 512, 512), (s, 500, 375), (s, 256, 256)}
    for s, H, W in sorted(cases):
        got = msf_scaled_size(s, H, W)
        assert got == _ref_rule(s, H, W), (s, H, W, got)
        assert got[0] % 32 == 0 and got[1] % 32 == 0
    assert msf_scaled_size(1.75, 512, 512) == (896, 896) and msf_scaled_size(1.75, 45, 61) == (96, 128)


def test_msf_symbols_exported_with_c_signatures(native):
    header = open(os.path.join(ROOT, "include", "sea_hip.h")).read()
    for name in ("sea_msf_resize_input", "sea_msf_accumulate"):
        decl = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)", header, flags=re.M)
        assert decl, name
        assert "torch" not in decl.group(1) and "&" not in decl.group(1)
        assert name in native.EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T sea_msf_resize_input$", out, flags=re.M) and re.search(r" T sea_msf_accumulate$", out, flags=re.M)
    lib = native.lib()
    assert lib.sea_abi_version() == 3
    # argument checks fire on the host before any launch: invalid arguments return 1 (no device needed)
    assert lib.sea_msf_resize_input(None, None, None, 1, 4, 4, 8, 8, None) == 1
    assert lib.sea_msf_accumulate(None, None, 1, 5, 4, 4, 8, 8, 8, 8, 0, None) == 1
    dummy = C.c_void_p(16)
    assert lib.sea_msf_accumulate(dummy, dummy, 1, 193, 4, 4, 8, 8, 8, 8, 0, None) == 1     # > SEA_MSF_MAX_CLASSES
    assert lib.sea_msf_accumulate(dummy, dummy, 1, 5, 16, 4, 8, 8, 8, 8, 0, None) == 1      # logits larger than the scale
    assert native.MSF_MAX_CLASSES == 192


def test_msf_wrappers_refuse_cpu_tensors(native):
    import torch
    with pytest.raises(native.SeaNativeError):
        native.msf_resize_input(torch.zeros(1, 3, 4, 4), (8, 8), flip=True)
    with pytest.raises(native.SeaNativeError):
        native.msf_accumulate(torch.zeros(1, 5, 4, 4), torch.zeros(1, 5, 8, 8), (8, 8))
