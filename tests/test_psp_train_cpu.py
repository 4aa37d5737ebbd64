"""PIR-AT on PSPNet, the parts that need no GPU: the reference's eight SGD parameter groups (tools/train_rob_seg.py:185-204
of the reference) and its poly LR rule with the x10 factor of the new modules (lines 356-361)."""
import pytest
import torch

from tools import train_rob_seg as T
from semseg.models import PSPNet


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return PSPNet(50, 21)


def test_param_groups_partition_the_parameters_in_the_reference_order(model):
    groups = T.psp_param_groups(model, 0.01)
    assert len(groups) == 8
    mods = [model.layer0, model.layer1, model.layer2, model.layer3, model.layer4, model.ppm, model.cls, model.aux]
    for g, m in zip(groups, mods):
        assert g["lr"] == 0.01
        assert [id(p) for p in g["params"]] == [id(p) for p in m.parameters()]
    flat = [id(p) for g in groups for p in g["params"]]
    assert len(flat) == len(set(flat))                                          # disjoint
    assert sorted(flat) == sorted(id(p) for p in model.parameters())            # and complete
    opt = torch.optim.SGD(groups, 0.01, momentum=0.9, weight_decay=1e-4)
    assert all(g["weight_decay"] == 1e-4 and g["momentum"] == 0.9 for g in opt.param_groups)


def test_poly_lr_sequence():
    base, total = 4e-4, 7
    opt = torch.optim.SGD([dict(params=[torch.nn.Parameter(torch.zeros(1))], lr=base) for _ in range(8)], base,
                          momentum=0.9)
    seen = []
    for it in range(total):
        seen.append([g["lr"] for g in opt.param_groups])                       # the rate step `it` runs at
        T.set_psp_lr(opt, base, it, total)
    assert seen[0] == [base] * 8                                               # step 0: every group at base (the reference)
    for it in range(1, total):
        want = base * (1 - (it - 1) / total) ** 0.9
        assert seen[it][:5] == pytest.approx([want] * 5, rel=1e-12)
        assert seen[it][5:] == pytest.approx([10 * want] * 3, rel=1e-12)
    assert T.poly_lr(base, 0, total) == base
    assert T.poly_lr(base, total, total) == 0.0
