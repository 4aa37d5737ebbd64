"""PSPNet-ResNet50 without a GPU: the model's key list against the reference's (recorded in the golden fixtures), the
seeded weight rule, the fixtures themselves, the plain (reference-semantics) forward against the reference's logits, and
tools.infer's model factory on the new config."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG

CASES = ("65x65", "57x97")


def _golden(tag):
    return np.load(os.path.join(GOLDEN, f"g16_psp_{tag}.npz"))


def _seeded_model(seed):
    from devtools.psp_weights import seeded_state_dict
    from semseg.models import PSPNet
    m = PSPNet(50, 21)
    m.load_state_dict(seeded_state_dict(m.state_dict(), seed), strict=True)
    return m.eval()


def test_state_dict_keys_match_the_reference():
    from semseg.models import PSPNet
    keys = list(PSPNet(50, 21, pretrained=False).state_dict())
    for tag in CASES:
        assert keys == [str(k) for k in _golden(tag)["keys"]]
    assert len(keys) == 370 and any(k.startswith("aux.") for k in keys) and any(k.endswith("num_batches_tracked") for k in keys)


def test_weight_rule_is_reproducible_and_order_free():
    from devtools.psp_weights import seeded_state_dict
    from semseg.models import PSPNet
    sd = PSPNet(50, 21).state_dict()
    a = seeded_state_dict(sd, 16)
    b = seeded_state_dict(dict(reversed(list(sd.items()))), 16)
    c = seeded_state_dict(sd, 17)
    assert list(a) == list(sd)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["layer4.2.conv2.weight"], c["layer4.2.conv2.weight"])
    assert float(a["layer1.0.bn1.running_var"].min()) >= 0.5 and float(a["layer1.0.bn1.weight"].max()) <= 1.5
    # the bottleneck conv3 scale-down
    w3, w1 = a["layer3.0.conv3.weight"], a["layer3.0.conv1.weight"]
    assert float(w3.std() * (w3.shape[1] ** 0.5)) < 0.5 * float(w1.std() * (w1.shape[1] ** 0.5))


@pytest.mark.parametrize("tag", CASES)
def test_fixtures_load(tag):
    g = _golden(tag)
    H, W = (int(v) for v in tag.split("x"))
    assert os.path.getsize(os.path.join(GOLDEN, f"g16_psp_{tag}.npz")) < 1_000_000
    assert g["x"].shape == (1, 3, H, W) and g["x"].dtype == np.float32
    assert g["logits"].shape == (1, 21, H, W) and g["logits"].dtype == np.float32
    assert g["y"].shape == (1, H, W) and g["pred"].shape == (1, H, W)
    assert 0.02 < float((g["y"] == -1).mean()) < 0.08
    assert np.array_equal(g["pred"], g["logits"].argmax(1))
    for k in ("grad_mask_ce_avg", "grad_mask_ce_bal"):
        assert g[k].shape == g["x"].shape and np.isfinite(g[k]).all() and np.abs(g[k]).max() > 0


def test_plain_forward_reproduces_the_reference_logits_on_cpu():
    g = _golden("65x65")
    model = _seeded_model(int(g["seed"]))
    with torch.no_grad():
        out = model(torch.from_numpy(g["x"]))
    ref = torch.from_numpy(g["logits"])
    assert (out - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()


def test_constructor_contract():
    from semseg.models import PSPNet
    with pytest.raises(ValueError):
        PSPNet(101, 21)
    m = PSPNet(50, 21)
    assert not hasattr(m, "forward_lowres")        # K2u / K10b assume align_corners=False: no fused up-sampling hook
    with pytest.raises(AssertionError):
        m.eval()(torch.zeros(1, 3, 64, 64))        # (H - 1) % 8 == 0, as the reference asserts


def test_build_model_accepts_the_pspnet_config():
    import yaml
    from semseg.models import PSPNet
    from tools.infer import build_model
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "pascalvoc_pspnet.yaml")))
    assert cfg["MODEL"]["NAME"] == "PSPNet" and int(cfg["EVAL"]["IMAGE_SIZE"][0]) == 473
    model = build_model(cfg, random_init=True, device=torch.device("cpu"))
    assert isinstance(model, PSPNet) and not model.training
    assert model.cls[4].out_channels == cfg["EVAL"]["N_CLS"]
