"""SEA through sliding windows, CPU side (`-m "not gpu"`): the three new entry points are declared in the header and bound
in ``_native._SIGS``, check their arguments on the host, and ``SlidingWindowModel`` refuses bad arguments before any device
call."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import PKG

NEW = ("sea_sw_cut", "sea_sw_cut_bwd", "sea_sw_merge_bwd")


@pytest.fixture(scope="module")
def native():
    from semseg import _native
    if not os.path.exists(_native.LIB_PATH):
        import sys
        sys.path.insert(0, PKG)
        import build_native
        build_native.build(verbose=False)
    return _native


def test_new_symbols_are_declared_and_bound(native):
    header = open(os.path.join(os.path.dirname(PKG), "include", "sea_hip.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in native._SIGS and name in native.EXPORTS
        assert hasattr(native.lib(), name)
    assert "segmenter_eval.py:51-67" in header and "segmenter_eval.py:70-83" in header
    for fn in ("sw_cut", "sw_cut_backward", "sw_merge_backward"):
        assert callable(getattr(native, fn))


def test_new_entry_points_check_arguments_on_the_host(native):
    lib = native.lib()
    d, e = C.c_void_p(16), C.c_void_p(4096)

    def arr(a):
        return (C.c_int * len(a))(*a), len(a)

    def cut(fn, ha, wa, H, W, ws=32, B=1, Cx=3, a=d, b=e):
        return fn(a, b, B, Cx, ws, *arr(ha), *arr(wa), H, W, None)

    def merge_bwd(ha, wa, H, W, Cc=5, hl=32, wl=32, ws=32, B=1, a=d, b=e):
        return lib.sea_sw_merge_bwd(a, b, B, Cc, hl, wl, ws, *arr(ha), *arr(wa), H, W, None)

    for fn in (lib.sea_sw_cut, lib.sea_sw_cut_bwd):
        assert cut(fn, [0], [0, 14], 32, 45) == 1                # the last anchor is not W - ws
        assert cut(fn, [0], [0, 40], 32, 72) == 1                # a gap wider than the window
        assert cut(fn, [0], [13, 0], 32, 45) == 1                # not ascending
        assert cut(fn, [0], list(range(33)), 32, 64) == 1        # 33 anchors on an axis
        assert cut(fn, [0], [0, 13], 32, 45, ws=33) == 1         # window larger than the image
        assert cut(fn, [0], [0, 13], 32, 45, a=None) == 1
        assert cut(fn, [0], [0, 13], 32, 45, a=d, b=d) == 1      # aliasing
        assert cut(fn, [0], [0, 13], 32, 45, Cx=0) == 1
        assert cut(fn, [0], list(range(0, 32)), 32, 63, B=2048) == 1      # B * n_win > 65535
    assert merge_bwd([0], [0, 14], 32, 45) == 1
    assert merge_bwd([0], [0, 40], 32, 72) == 1
    assert merge_bwd([0], [1, 13], 32, 45) == 1                  # the first anchor is not 0
    assert merge_bwd([0], [0, 13], 32, 45, Cc=193) == 1          # > SEA_MSF_MAX_CLASSES
    assert merge_bwd([0], [0, 13], 32, 45, hl=33) == 1           # logits larger than the window
    assert merge_bwd([0], [0, 13], 32, 45, wl=0) == 1
    assert merge_bwd([0], [0, 13], 32, 45, b=None) == 1
    assert merge_bwd([0], [0, 13], 32, 45, a=d, b=d) == 1
    assert merge_bwd([0], list(range(0, 32)), 32, 63, B=2048) == 1


def test_new_wrappers_refuse_cpu_tensors(native):
    E = native.SeaNativeError
    with pytest.raises(E):
        native.sw_cut(torch.zeros(1, 3, 32, 45), 32, [0], [0, 13])
    with pytest.raises(E):
        native.sw_cut_backward(torch.zeros(2, 3, 32, 32), 32, [0], [0, 13], (32, 45))
    with pytest.raises(E):
        native.sw_merge_backward(torch.zeros(1, 5, 32, 45), 32, [0], [0, 13], (32, 32))


class _Boom(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        raise AssertionError("the model was called")


def test_sliding_window_model_validates_before_any_device_call(monkeypatch):
    from semseg import _native
    from semseg.utils.segmenter_eval import SlidingWindowModel

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    for fn in ("lib", "sw_cut", "sw_merge"):
        monkeypatch.setattr(_native, fn, no_device)
    inner = _Boom().eval()
    for ws, st, bs in [(32, 33, None), (0, 1, None), (32, 0, None), (32, 16, 0)]:
        with pytest.raises(ValueError):
            SlidingWindowModel(inner, ws, st, bs)
    with pytest.raises(TypeError):
        SlidingWindowModel(lambda x: x, 32, 16)
    wrap = SlidingWindowModel(inner, 32, 16, batch_size=4)
    with pytest.raises(ValueError):
        wrap(torch.zeros(1, 3, 20, 64))              # shorter than the window
    with pytest.raises(ValueError):
        wrap(torch.zeros(1, 3, 64, 31))              # narrower than the window
    with pytest.raises(ValueError):
        wrap(torch.zeros(3, 64, 64))
    assert not hasattr(wrap, "forward_lowres")
    assert [n for n, _ in wrap.named_parameters()] == ["model.p"]
    assert wrap.training is False
    inner.train()
    assert wrap.training is True
    wrap.eval()
    assert inner.training is False and wrap.training is False
    assert wrap.train() is wrap and inner.training is True
