"""The float64 reference of the no-gradient K2 tests (oracle.sea_oracle.loss_eval_f64), pinned without a GPU: against the
goldens generated from the reference repository, and on the six non-finite rows that define torch.max's index."""
import pytest
import torch

from conftest import load_golden
from oracle import sea_oracle as O

MODES = (("mask_ce_avg", 0), ("mask_ce_bal", 1), ("js_avg", 2), ("ce", 3))

NAN, INF = float("nan"), float("inf")
NONFINITE_ROWS = ([1, NAN, 5, NAN], [INF, 2, INF, 0], [-INF] * 4, [NAN, INF, 1, 2], [1, INF, NAN, INF], [-INF, 3, 3, -INF])
NONFINITE_ARG = [1, 0, 0, 0, 2, 1]


@pytest.mark.parametrize("C", [5, 21, 151])
def test_f64_reference_matches_goldens(C):
    g = load_golden(f"g1_losses_C{C}")
    logits, y, w = g["logits"], g["y"], g["w"]
    B, _, H, W = logits.shape
    HW = H * W
    for key, mode in MODES:
        ref = O.loss_eval_f64(logits, y, w, mode, 3)
        assert torch.equal(ref["pred"], g["pred"])
        assert torch.equal(ref["n_correct"].float() / HW, g["acc_step0"])
        torch.testing.assert_close(ref["loss_px"].float(), g[key + "_px"], rtol=2e-5, atol=2e-6)
        torch.testing.assert_close((ref["loss_sum"] / HW).float(), g[key + "_img"], rtol=3e-5, atol=1e-6)
        torch.testing.assert_close(ref["track_px"].float(), g["ce_px"], rtol=2e-5, atol=2e-6)
        torch.testing.assert_close((ref["track_sum"] / HW).float(), g["ce_img"], rtol=3e-5, atol=1e-6)


def test_f64_reference_first_maximum():
    g = load_golden("g1_argmax_ties")
    z = g["z"].view(3, 4, 1, 1)
    ref = O.loss_eval_f64(z, torch.zeros(3, 1, 1, dtype=torch.int64), None, 3, 3)
    assert torch.equal(ref["pred"].view(3), g["arg"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_f64_reference_non_finite_rows(dtype):
    """the first NaN wins, else the first maximum; the label of row r is its expected index, so all six count as correct"""
    z = torch.tensor(NONFINITE_ROWS, dtype=dtype).view(6, 4, 1, 1)
    y = torch.tensor(NONFINITE_ARG).view(6, 1, 1)
    ref = O.loss_eval_f64(z, y, None, 0, 3)
    assert ref["pred"].view(6).tolist() == NONFINITE_ARG
    assert ref["n_correct"].tolist() == [1] * 6
    assert torch.isfinite(ref["loss_px"][5]).all()              # two -inf classes, two tied finite ones: a finite loss
    assert ref["loss_px"][5].item() == pytest.approx(0.6931471805599453, rel=1e-12)


def test_f64_reference_ignores_out_of_range_labels():
    z = torch.randn(1, 5, 2, 3, generator=torch.Generator().manual_seed(0))
    y = torch.tensor([[[0, 5, 8], [-1, 2, 255]]])
    ref = O.loss_eval_f64(z, y, None, 3, 3)
    assert (ref["loss_px"][0] != 0).tolist() == [[True, False, False], [False, True, False]]
    y8 = torch.where(y < 0, torch.full_like(y, 255), y).to(torch.uint8)
    ref8 = O.loss_eval_f64(z, y8, None, 3, 3)
    assert torch.equal(ref8["loss_px"], ref["loss_px"]) and torch.equal(ref8["n_correct"], ref["n_correct"])
