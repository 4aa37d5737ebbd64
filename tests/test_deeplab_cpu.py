"""DeepLabV3-ResNet50 without a GPU: the model's key list against the reference's (recorded in the golden fixtures
tests/golden/g19_deeplab_*.npz), the fixtures themselves, the plain (reference-semantics) forward against the reference's
logits, the training-mode return value, the constructor's refusals, tools.infer's model factory on the new config, and the
two P5 entry points (declared in the header, exported by the library, bound with the right arity, argument errors before
any launch)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG, ROOT

CASES = ((65, 65), (57, 97), (153, 153))
SYMBOLS = ("sea_aspp_tap_sum", "sea_aspp_tap_sum_backward")


def _golden(H, W):
    from devtools import deeplab_goldens
    return deeplab_goldens.load(GOLDEN, H, W)


def _seeded_model(seed):
    from devtools.psp_weights import seeded_state_dict
    from semseg.models import DeepLabV3
    m = DeepLabV3(50, classes=21)
    m.load_state_dict(seeded_state_dict(m.state_dict(), seed), strict=True)
    return m.eval()


@pytest.fixture(scope="module")
def native():
    from semseg import _native
    if not os.path.exists(_native.LIB_PATH):
        import sys
        sys.path.insert(0, PKG)
        import build_native
        build_native.build(verbose=False)
    return _native


def test_state_dict_keys_match_the_reference():
    from semseg.models import DeepLabV3, PSPNet
    keys = list(DeepLabV3(50, classes=21, pretrained=False).state_dict())
    for H, W in CASES:
        assert keys == [str(k) for k in _golden(H, W)["keys"]]
    assert len(keys) == 376 and any(k.startswith("aux.") for k in keys) and "aspp.convs.4.1.weight" in keys
    # the backbone is PSPNet(clean=True)'s, key for key
    layer_keys = [k for k in keys if k.startswith("layer")]
    assert len(layer_keys) == 330 and layer_keys == [k for k in PSPNet(50, 21).state_dict() if k.startswith("layer")]


@pytest.mark.parametrize("H,W", CASES)
def test_fixtures_load(H, W):
    from devtools import deeplab_goldens
    g = _golden(H, W)
    for f in deeplab_goldens.files(GOLDEN, H, W):
        assert os.path.getsize(f) <= 1 << 20, f
    assert int(g["seed"]) == 19
    assert g["x"].shape == (1, 3, H, W) and g["x"].dtype == np.float32
    assert g["logits"].shape == (1, 21, H, W) and g["logits"].dtype == np.float32
    assert g["y"].shape == (1, H, W) and g["pred"].shape == (1, H, W)
    assert 0.02 < float((g["y"] == -1).mean()) < 0.08
    assert np.array_equal(g["pred"], g["logits"].argmax(1))
    for k in ("grad_mask_ce_avg", "grad_mask_ce_bal"):
        assert g[k].shape == g["x"].shape and np.isfinite(g[k]).all() and np.abs(g[k]).max() > 0


@pytest.mark.parametrize("H,W", CASES)
def test_plain_forward_reproduces_the_reference_logits_on_cpu(H, W):
    g = _golden(H, W)
    model = _seeded_model(int(g["seed"]))
    with torch.no_grad():
        out = model(torch.from_numpy(g["x"]))
    ref = torch.from_numpy(g["logits"])
    assert (out - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


def test_every_aspp_branch_carries_signal():
    """what makes the fixtures a test of the ASPP: no branch of the seeded model is dead on the 20 x 20 map"""
    g = _golden(153, 153)
    model = _seeded_model(int(g["seed"]))
    seen = {}
    hook = model.aspp.register_forward_hook(lambda m, i, o: seen.update(out=o))
    with torch.no_grad():
        model(torch.from_numpy(g["x"]))
    hook.remove()
    per_branch = seen["out"].view(1, 5, 256, 20, 20).abs().amax((0, 2, 3, 4))
    assert per_branch.min().item() > 0.5, per_branch


def test_training_mode_returns_the_references_four_elements():
    from semseg.models import DeepLabV3
    torch.manual_seed(0)
    m = DeepLabV3(50, classes=5).train()
    x = torch.rand(2, 3, 33, 33)
    y = torch.randint(0, 5, (2, 33, 33))
    y[:, :2] = 255
    out = m(x, y)
    assert isinstance(out, tuple) and len(out) == 4
    pred, main_loss, aux_loss, logits = out
    assert logits.shape == (2, 5, 33, 33) and torch.equal(pred, logits.max(1)[1])
    assert main_loss.dim() == 0 and aux_loss.dim() == 0 and torch.isfinite(main_loss) and torch.isfinite(aux_loss)
    (main_loss + 0.4 * aux_loss).backward()
    assert m.aspp.convs[2][0].weight.grad is not None and m.aux[0].weight.grad is not None
    # eval with indicate=1 keeps the four elements; plain eval returns the logits alone
    m.eval()
    with torch.no_grad():
        assert len(m(x, y, indicate=1)) == 4
        assert m(x).shape == (2, 5, 33, 33)


def test_constructor_contract():
    import inspect
    from semseg.models import DeepLabV3
    with pytest.raises(ValueError):
        DeepLabV3(101, classes=21)
    with pytest.raises(ValueError):
        DeepLabV3(50, classes=21, use_aspp=False)
    sig = inspect.signature(DeepLabV3.__init__)
    assert list(sig.parameters)[1:] == ["layers", "atrous_rates", "dropout", "classes", "zoom_factor", "use_aspp",
                                        "criterion", "BatchNorm", "pretrained"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["layers"], d["atrous_rates"], d["dropout"], d["classes"], d["zoom_factor"], d["use_aspp"]) == \
        (50, (6, 12, 18), 0.1, 2, 8, True)
    assert d["criterion"].ignore_index == 255 and d["BatchNorm"] is torch.nn.BatchNorm2d and d["pretrained"] is True
    m = DeepLabV3(50, classes=21)
    assert [c[0].dilation for c in m.aspp.convs[1:4]] == [(6, 6), (12, 12), (18, 18)]
    with pytest.raises(AssertionError):
        m.eval()(torch.zeros(1, 3, 64, 64))        # (H - 1) % 8 == 0, as the reference asserts


def test_build_model_accepts_the_deeplabv3_config():
    import yaml
    from semseg.models import DeepLabV3
    from semseg.utils.utils import getModelName
    from tools.infer import build_model
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "pascalvoc_deeplabv3.yaml")))
    psp = yaml.safe_load(open(os.path.join(PKG, "configs", "pascalvoc_pspnet.yaml")))
    assert cfg["MODEL"]["NAME"] == "DeepLabV3" and int(cfg["EVAL"]["IMAGE_SIZE"][0]) == 473
    psp["MODEL"]["NAME"] = "DeepLabV3"
    assert cfg == psp                                  # the PSPNet config with another MODEL.NAME
    model = build_model(cfg, random_init=True, device=torch.device("cpu"))
    assert isinstance(model, DeepLabV3) and not model.training
    assert model.cls[4].out_channels == cfg["EVAL"]["N_CLS"]
    assert [c[0].dilation[0] for c in model.aspp.convs[1:4]] == [6, 12, 18]     # N_CLS did not land in atrous_rates
    assert getModelName("DeepLabV3", "RN50") == "DeepLabV3_RN50" and getModelName("PSPNet", "RN50") == "PSPNet_RN50"


def test_entry_points_declared_exported_and_bound(native):
    header = open(os.path.join(ROOT, "include", "sea_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        decl = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)", header, flags=re.M)
        assert decl, name
        assert "torch" not in decl.group(1) and "&" not in decl.group(1)
        assert len(decl.group(1).split(",")) == len(native._SIGS[name][1]), name     # arity of the ctypes prototype
        assert re.search(r" T " + name + r"$", out, flags=re.M), name
        assert name in native.EXPORTS
    assert "ddcat_psp.py:44-58" in header and "ddcat_psp.py:69-81" in header          # the reference lines they replace
    assert callable(native.aspp_tap_sum) and callable(native.aspp_tap_sum_backward)
    src = open(os.path.join(PKG, "build_native.py")).read()
    assert re.search(r'\("aspp_kernels\.hip",\s*\["-ffp-contract=off"\]\)', src)
    lib = native.lib()
    import ctypes
    rates = (ctypes.c_int * 3)(6, 12, 18)
    # null pointers: the argument error, before any launch (no device is touched)
    assert lib.sea_aspp_tap_sum(None, 6912, 0, None, None, 1280, 256, 1, 9, 9, 3, 256, rates, None) == 1
    assert lib.sea_aspp_tap_sum_backward(None, 1280, 256, None, 1280, 256, None, 6912, 0, 1, 9, 9, 3, 256, rates, None) == 1
    with pytest.raises(native.SeaNativeError):       # CPU tensors: no fallback
        native.aspp_tap_sum(torch.zeros(1, 9, 9, 27 * 12), (6, 12, 18), torch.zeros(36))
