"""Sliding-window evaluation, CPU side (`-m "not gpu"`): the anchor rule against the reference's goldens
(tests/golden/g16_sw_*.npz, devtools/gen_sw_goldens.py) and hand cases, the resize-target rule, the padding round trip,
and the host-side argument checks of the K11 entry points (no device needed)."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG

FILES = sorted(glob.glob(os.path.join(GOLDEN, "g16_sw_*.npz")))


@pytest.fixture(scope="module")
def native():
    from semseg import _native
    if not os.path.exists(_native.LIB_PATH):
        import sys
        sys.path.insert(0, PKG)
        import build_native
        build_native.build(verbose=False)
    return _native


def test_g16_sw_fixtures_load():
    assert len(FILES) == 8, FILES
    classes, flips, shapes = set(), set(), set()
    for f in FILES:
        g = np.load(f)
        x, y, C_ = g["x"], g["y"], int(g["n_classes"])
        B, _, H, W = x.shape
        Hm, Wm = (int(v) for v in g["shape"])
        n_win, ws = len(g["anchors"]), int(g["window_size"])
        assert B == 2 and max(H, W, Hm, Wm) < 128 and y.shape == (B, H, W)
        assert g["seg_maps"].shape == (B * n_win, C_, ws, ws) and g["logit_avg"].shape == (B, C_, Hm, Wm)
        assert g["probs"].shape == (B, C_, H, W) and g["hist"].shape == (C_, C_)
        np.testing.assert_allclose(g["probs"].sum(1), 1.0, rtol=0, atol=1e-5)
        assert g["hist"].sum() == (y != int(g["ignore_label"])).sum()
        assert int(g["near_ties"]) <= max(4, int((y != -1).sum()) // 200)
        assert ("score" in g.files) == bool(int(g["flip"]))
        assert os.path.getsize(f) < 2 ** 20
        classes.add(C_)
        flips.add(int(g["flip"]))
        shapes.add((H, W, int(g["window_stride"])))
    assert classes == {5, 21} and flips == {0, 1}
    assert shapes == {(32, 32, 32), (32, 45, 32), (48, 61, 16), (50, 70, 24), (20, 29, 32)}


def test_sw_anchors_match_the_reference_goldens():
    from semseg.utils.segmenter_eval import sliding_window, sw_anchors
    for f in FILES:
        g = np.load(f)
        Hm, Wm = (int(v) for v in g["shape"])
        ws, st = int(g["window_size"]), int(g["window_stride"])
        ha, wa = sw_anchors(Hm, Wm, ws, st)
        assert ha == g["h_anchors"].tolist() and wa == g["w_anchors"].tolist(), f
        win = sliding_window(torch.zeros(1, 3, Hm, Wm), False, ws, st)
        assert win["anchors"] == [tuple(a) for a in g["anchors"].tolist()]
        assert win["shape"] == (Hm, Wm) and win["flip"] is False
        assert all(c.shape == (1, 3, ws, ws) for c in win["crop"])


@pytest.mark.parametrize("H,W,ws,stride,ha,wa", [(32, 32, 32, 32, [0], [0]), (32, 45, 32, 32, [0], [0, 13]),
                                                 (48, 61, 32, 16, [0, 16], [0, 16, 29]),
                                                 (50, 70, 32, 24, [0, 18], [0, 24, 38]), (32, 46, 32, 32, [0], [0, 14]),
                                                 (512, 683, 512, 512, [0], [0, 171]), (64, 112, 64, 48, [0], [0, 48])])
def test_sw_anchors_hand_cases(H, W, ws, stride, ha, wa):
    from semseg.utils.segmenter_eval import sw_anchors
    assert sw_anchors(H, W, ws, stride) == (ha, wa)


def test_sw_anchors_refuses_uncovered_pixels():
    from semseg.utils.segmenter_eval import sw_anchors
    with pytest.raises(ValueError):
        sw_anchors(64, 96, 32, 33)               # the reference would divide 0 by 0 at the uncovered columns
    with pytest.raises(ValueError):
        sw_anchors(20, 29, 32, 32)               # smaller than the window: resize comes first
    assert sw_anchors(64, 96, 32, 32) == ([0, 32], [0, 32, 64])


def test_resize_target_rule():
    from semseg.utils.segmenter_eval import resize
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, 20, 29, generator=g)
    r = resize(x, 32)
    assert tuple(r.shape) == (2, 3, 32, 46)      # int(29 / 20 * 32) = 46
    assert torch.equal(r, torch.nn.functional.interpolate(x, (32, 46), mode="bilinear"))
    big = torch.rand(2, 3, 32, 45, generator=g)
    assert resize(big, 32) is big                # the short side is large enough: untouched
    tall = resize(torch.rand(1, 3, 29, 20, generator=g), 32)
    assert tuple(tall.shape) == (1, 3, 46, 32)


def test_padding_unpadding_round_trip():
    from semseg.utils.segmenter_eval import padding, unpadding
    g = torch.Generator().manual_seed(4)
    x = torch.rand(2, 3, 45, 61, generator=g)
    p = padding(x, 16, fill_value=7.0)
    assert tuple(p.shape) == (2, 3, 48, 64)
    assert torch.equal(p[:, :, :45, :61], x) and bool((p[:, :, 45:] == 7.0).all()) and bool((p[:, :, :, 61:] == 7.0).all())
    assert torch.equal(unpadding(p, (45, 61)), x)
    same = torch.rand(1, 3, 32, 64, generator=g)
    assert padding(same, 16) is same and unpadding(same, (32, 64)) is same


def test_merge_windows_refuses_unordered_anchors():
    from semseg.utils.segmenter_eval import merge_windows
    win = {"anchors": [(0, 13), (0, 0)], "shape": (32, 45), "flip": False, "seg_maps": torch.zeros(2, 5, 32, 32)}
    with pytest.raises(ValueError):
        merge_windows(win, 32, (32, 45))


def test_sw_entry_points_check_arguments_on_the_host(native):
    lib = native.lib()
    assert lib.sea_abi_version() == 3 and native.SW_MAX_ANCHORS == 32
    assert "sea_sw_merge" in native.EXPORTS and "sea_sw_finish" in native.EXPORTS
    d = C.c_void_p(16)
    e = C.c_void_p(4096)

    def merge(ha, wa, H, W, Cc=5, hl=32, wl=32, ws=32, B=1, flip=0, softmax=0, acc=0, a=d, b=e):
        return lib.sea_sw_merge(a, b, B, Cc, hl, wl, ws, (C.c_int * len(ha))(*ha), len(ha), (C.c_int * len(wa))(*wa), len(wa),
                                H, W, flip, softmax, acc, None)

    assert merge([0], [0, 14], 32, 45) == 1                  # the last anchor is not W - ws
    assert merge([0], [0, 20], 32, 45) == 1                  # an anchor beyond W - ws
    assert merge([0], [0, 40], 32, 72) == 1                  # a gap wider than the window
    assert merge([0], [13, 0], 32, 45) == 1                  # not ascending
    assert merge([0], [1, 13], 32, 45) == 1                  # the first anchor is not 0
    assert merge([0], list(range(33)), 32, 64) == 1          # 33 anchors on an axis
    assert merge([0], [0, 13], 32, 45, Cc=193) == 1          # > SEA_MSF_MAX_CLASSES
    assert merge([0], [0, 13], 32, 45, hl=33) == 1           # logits larger than the window
    assert merge([0], [0, 13], 32, 45, flip=1) == 1          # the mirror belongs to the softmax epilogue
    assert merge([0], [0, 13], 32, 45, a=d, b=d) == 1        # out aliases the logits
    assert merge([0], [0, 13], 32, 45, a=None) == 1
    assert merge([0], list(range(0, 32)), 32, 63, B=2048) == 1        # B * n_win > 65535
    assert lib.sea_sw_finish(None, e, 1, 5, 32, 46, 20, 29, 0, 0, None) == 1
    assert lib.sea_sw_finish(d, e, 1, 193, 32, 46, 20, 29, 0, 0, None) == 1
    assert lib.sea_sw_finish(d, d, 1, 5, 32, 46, 20, 29, 0, 0, None) == 1
    assert lib.sea_sw_finish(d, e, 1, 5, 32, 46, 0, 29, 0, 0, None) == 1


def test_sw_wrappers_refuse_cpu_tensors(native):
    with pytest.raises(native.SeaNativeError):
        native.sw_merge(torch.zeros(2, 5, 32, 32), 32, [0], [0, 13], (32, 45))
    with pytest.raises(native.SeaNativeError):
        native.sw_finish(torch.zeros(1, 5, 32, 46), (20, 29))
