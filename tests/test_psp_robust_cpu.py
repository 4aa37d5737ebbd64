"""PSPNet(clean=False), the robust torchvision-style stem, without a GPU: the key list and shapes against the reference's
(recorded in the g18 fixtures of devtools/gen_psp_robust_goldens.py), the plain forward against the reference's logits, the
unchanged clean=True model, and the optional MODEL.CLEAN key of both tools."""
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN, PKG

CASES = ("65x65", "57x97")


def _golden(tag):
    return np.load(os.path.join(GOLDEN, f"g18_psp_robust_{tag}.npz"))


@pytest.fixture(scope="module")
def seeded():
    from devtools.psp_weights import seeded_state_dict
    from semseg.models import PSPNet
    m = PSPNet(50, 21, pretrained=False, clean=False)
    m.load_state_dict(seeded_state_dict(m.state_dict(), int(_golden("65x65")["seed"])), strict=True)
    return m.eval()


def test_state_dict_keys_and_shapes_match_the_reference():
    from semseg.models import PSPNet
    sd = PSPNet(50, 21, pretrained=False, clean=False).state_dict()
    keys = list(sd)
    for tag in CASES:
        assert keys == [str(k) for k in _golden(tag)["keys"]]
    assert len(keys) == 358 and any(k.startswith("aux.") for k in keys)
    # the reference's shapes (backbones/resnet_ddcat.py:115-131, 146-166 with inplanes = 64)
    assert tuple(sd["layer0.0.weight"].shape) == (64, 3, 7, 7)
    assert tuple(sd["layer0.1.running_mean"].shape) == (64,)
    assert tuple(sd["layer1.0.conv1.weight"].shape) == (64, 64, 1, 1)
    assert tuple(sd["layer1.0.downsample.0.weight"].shape) == (256, 64, 1, 1)
    assert tuple(sd["layer1.1.conv1.weight"].shape) == (64, 256, 1, 1)
    assert not any(k.startswith(("layer0.3.", "layer0.4.", "layer0.6.", "layer0.7.")) for k in keys)
    # everything after layer1.0 has the shapes of the clean=True model
    clean = PSPNet(50, 21).state_dict()
    for k in keys:
        if not k.startswith(("layer0.", "layer1.0.conv1.", "layer1.0.downsample.0.")):
            assert sd[k].shape == clean[k].shape, k


def test_clean_model_is_unchanged():
    from semseg.models import PSPNet
    m = PSPNet(50, 21)
    assert len(m.state_dict()) == 370 and len(m.layer0) == 10
    assert tuple(m.layer0[0].weight.shape) == (64, 3, 3, 3) and m.layer1[0].conv1.in_channels == 128


@pytest.mark.parametrize("tag", CASES)
def test_fixtures_load(tag):
    g = _golden(tag)
    H, W = (int(v) for v in tag.split("x"))
    assert os.path.getsize(os.path.join(GOLDEN, f"g18_psp_robust_{tag}.npz")) < 1_000_000
    assert g["x"].shape == (1, 3, H, W) and g["x"].dtype == np.float32
    assert g["logits"].shape == (1, 21, H, W) and g["logits"].dtype == np.float32
    assert g["y"].shape == (1, H, W) and g["pred"].shape == (1, H, W) and int(g["seed"]) == 18
    assert 0.02 < float((g["y"] == -1).mean()) < 0.08
    assert np.array_equal(g["pred"], g["logits"].argmax(1))
    for k in ("grad_mask_ce_avg", "grad_mask_ce_bal"):
        assert g[k].shape == g["x"].shape and np.isfinite(g[k]).all() and np.abs(g[k]).max() > 0


@pytest.mark.parametrize("tag", CASES)
def test_plain_forward_reproduces_the_reference_logits_on_cpu(seeded, tag):
    """the tolerance of tests/test_psp_cpu.py for g16: 1e-4 of the logit scale; the argmax may differ only at near-ties"""
    g = _golden(tag)
    with torch.no_grad():
        out = seeded(torch.from_numpy(g["x"]))
    ref = torch.from_numpy(g["logits"])
    assert (out - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()
    top2 = ref.topk(2, 1).values
    decided = (top2[:, 0] - top2[:, 1]) > 2e-4 * ref.abs().max()
    assert torch.equal(out.argmax(1)[decided], torch.from_numpy(g["pred"].astype(np.int64))[decided])
    assert decided.float().mean().item() > 0.99


def test_tools_read_model_clean():
    from semseg.models import PSPNet
    from tools.infer import build_model
    from tools.train_rob_seg import psp_clean
    old = yaml.safe_load(open(os.path.join(PKG, "configs", "pascalvoc_pspnet.yaml")))
    new = yaml.safe_load(open(os.path.join(PKG, "configs", "pascalvoc_pspnet_pirat.yaml")))
    assert "CLEAN" not in old["MODEL"] and new["MODEL"]["CLEAN"] is False
    # the same recipe otherwise
    assert {k: v for k, v in new["MODEL"].items() if k != "CLEAN"} == old["MODEL"]
    assert all(new[k] == old[k] for k in old if k != "MODEL")
    assert psp_clean(old["MODEL"]) is True and psp_clean(new["MODEL"]) is False
    assert psp_clean({"NAME": "PSPNet", "CLEAN": True}) is True
    with pytest.raises(ValueError):
        psp_clean({"NAME": "PSPNet", "CLEAN": "no"})
    cpu = torch.device("cpu")
    m_old, m_new = build_model(old, random_init=True, device=cpu), build_model(new, random_init=True, device=cpu)
    assert isinstance(m_old, PSPNet) and len(m_old.layer0) == 10 and len(m_old.state_dict()) == 370
    assert isinstance(m_new, PSPNet) and not m_new.training and len(m_new.state_dict()) == 358
    assert tuple(m_new.layer0[0].weight.shape) == (64, 3, 7, 7) and m_new.cls[4].out_channels == new["EVAL"]["N_CLS"]
    with pytest.raises(ValueError):
        build_model({"MODEL": {"NAME": "PSPNet", "CLEAN": 0}, "EVAL": {"N_CLS": 21}}, random_init=True, device=cpu)
