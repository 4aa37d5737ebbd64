"""SEA through multi-scale + flip, CPU side (`-m "not gpu"`): the two new entry points are declared in the header and bound
in ``_native._SIGS`` with the declared arity, check their arguments on the host, and ``MsfModel`` refuses bad arguments before
any device call."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import PKG

NEW = ("sea_msf_resize_bwd", "sea_msf_accumulate_bwd")


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
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert m, name
        assert name in native._SIGS and name in native.EXPORTS
        assert hasattr(native.lib(), name)
        assert len(native._SIGS[name][1]) == len(m.group(1).split(",")), name           # arity of the declaration
    assert "adjoint of sea_msf_resize_input" in header and "adjoint of sea_msf_accumulate" in header
    for fn in ("msf_resize_input_backward", "msf_accumulate_backward"):
        assert callable(getattr(native, fn))
    assert native.EXPORTS[-2:] == NEW                       # appended: the earlier rows keep their places


def test_abi_version_stays_3(native):
    assert native.lib().sea_abi_version() == 3


def test_new_entry_points_check_arguments_on_the_host(native):
    lib = native.lib()
    a, b, c, d = (C.c_void_p(4096 * k) for k in (1, 2, 3, 4))

    def rb(g=a, gf=b, dsrc=c, planes=6, h=32, w=64, H=64, W=96, src_flip=0):
        return lib.sea_msf_resize_bwd(g, gf, dsrc, planes, h, w, H, W, src_flip, None)

    assert rb(g=None, gf=None) == 1                         # no gradient at all
    assert rb(dsrc=None) == 1
    assert rb(dsrc=a) == 1 and rb(dsrc=b) == 1              # aliasing
    assert rb(planes=0) == 1
    assert rb(h=0) == 1 and rb(w=0) == 1 and rb(H=0) == 1 and rb(W=0) == 1
    assert rb(h=1 << 16, w=1 << 15) == 1                    # h * w = 2^31
    assert rb(H=1 << 16, W=1 << 15) == 1

    def ab(lg=a, ds=b, G=c, out=d, B=2, Cc=5, hl=32, wl=64, Hs=32, Ws=64, H=64, W=96, flip=0):
        return lib.sea_msf_accumulate_bwd(lg, ds, G, out, B, Cc, hl, wl, Hs, Ws, H, W, flip, None)

    assert ab(Cc=193) == 1                                  # > SEA_MSF_MAX_CLASSES
    assert ab(Cc=0) == 1 and ab(B=0) == 1 and ab(B=65536) == 1
    for k in ("lg", "ds", "G", "out"):
        assert ab(**{k: None}) == 1
    assert ab(G=a) == 1 and ab(G=b) == 1 and ab(out=a) == 1 and ab(out=b) == 1 and ab(out=c) == 1      # aliasing
    assert ab(hl=33) == 1 and ab(wl=65) == 1                # logits larger than the scaled size
    assert ab(hl=0) == 1 and ab(H=0) == 1 and ab(W=0) == 1
    assert ab(H=1 << 16, W=1 << 15) == 1
    assert ab(hl=8, wl=8, Hs=1 << 16, Ws=1 << 15) == 1


def test_new_wrappers_refuse_cpu_tensors_and_bad_shapes(native):
    E = native.SeaNativeError
    with pytest.raises(E):
        native.msf_resize_input_backward(torch.zeros(1, 3, 64, 96), None, (32, 64))
    with pytest.raises(E):
        native.msf_resize_input_backward(None, None, (32, 64))
    with pytest.raises(E):
        native.msf_accumulate_backward(torch.zeros(1, 5, 32, 64), torch.zeros(1, 5, 64, 96), (32, 64))


class _Boom(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        raise AssertionError("the model was called")


class _Wide(torch.nn.Module):
    """193 classes"""

    def forward(self, x):
        return torch.zeros(x.shape[0], 193, *x.shape[2:])


def test_msf_model_validates_before_any_device_call(monkeypatch):
    from semseg import _native
    from semseg.utils.msf_model import MsfModel

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    for fn in ("lib", "msf_resize_input", "msf_accumulate"):
        monkeypatch.setattr(_native, fn, no_device)
    inner = _Boom().eval()
    for scales in ([], [0.5, 0.0], [-1.0], [float("nan")]):
        with pytest.raises(ValueError):
            MsfModel(inner, scales, True)
    with pytest.raises(ValueError):
        MsfModel(inner, [1.0], False, n_classes=193)
    with pytest.raises(TypeError):
        MsfModel(lambda x: x, [1.0], False)
    wrap = MsfModel(inner, (0.5, 1.0), True, n_classes=192)
    with pytest.raises(ValueError):
        wrap(torch.zeros(3, 64, 64))
    with pytest.raises(ValueError):
        wrap.score(torch.zeros(3, 64, 64))
    with pytest.raises(ValueError):
        MsfModel(inner, [0.01], False)(torch.zeros(1, 3, 64, 64))          # int(0.01 * 64) = 0: an empty scaled image
    assert not hasattr(wrap, "forward_lowres")
    assert [n for n, _ in wrap.named_parameters()] == ["model.p"] and list(wrap.buffers()) == []
    assert wrap.training is False
    inner.train()
    assert wrap.training is True
    wrap.eval()
    assert inner.training is False and wrap.training is False
    assert wrap.train() is wrap and inner.training is True


def test_msf_model_refuses_193_classes_before_the_first_accumulate(monkeypatch):
    """the class count is the model's to tell: a wrapper built without ``n_classes`` refuses when the first pass's logits show
    it, before any K10b launch and before it allocates the score buffer"""
    from semseg import _native
    from semseg.utils.msf_model import MsfModel

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    def fake_resize(x, size, flip=False, **k):
        y = torch.zeros(x.shape[0], x.shape[1], *size)
        return y, (y if flip else None)

    monkeypatch.setattr(_native, "msf_accumulate", no_device)
    monkeypatch.setattr(_native, "msf_resize_input", fake_resize)
    wrap = MsfModel(_Wide().eval(), [1.0], True)
    with pytest.raises(ValueError, match="192"):
        wrap.score(torch.zeros(1, 3, 64, 64))
    assert wrap.__dict__["_held"] == {}
