"""Training-time losses (counterpart of semseg/losses.py:6-109) of the PIR-AT OUTER step.

``CrossEntropy`` and ``OhemCrossEntropy`` take ``native=True`` to run on the device through T2 (csrc/train_loss.hip:
fused forward, hard-pixel selection and backward, no host read, no log-softmax kept for the backward).  The default
``native=False`` is the plain PyTorch arithmetic every existing caller gets.  With ``native=True`` a tensor that is not
on the HIP device raises ``SeaNativeError`` (no CPU fallback), and so do logits that are neither dense NCHW nor
channels_last; channels_last logits, for which T2 has no kernel, go through the PyTorch criterion (with its host
synchronisations for OHEM).  The native loss is an fp32 scalar whatever the logits' dtype.  ``Dice`` stays PyTorch: it takes probabilities, and no configuration of the reference
uses it.

Both criteria also have ``upsampled(preds_low, labels)``: the value and gradient of ``self(F.interpolate(p, labels.shape[-2:],
mode="bilinear", align_corners=False), labels)`` for the low-resolution output ``p`` of a model head (a tensor, or a tuple with
``aux_weights``).  With ``native=False`` it is exactly that composition; with ``native=True`` it runs T2u
(csrc/train_loss_up.hip), which interpolates inside the criterion's kernels: the full-resolution logits and their gradient are
never created.  A class count T2u has no kernel for (outside 2..192) takes the composition with T2.

``upsampled(preds_low, labels, align_corners=True)`` is the same for PSPNet's rule, ``F.interpolate(..., align_corners=True)``:
``native=True`` runs T2u-ac (the kernels of csrc/train_loss_up.hip instantiated for that rule), or P2 (``upsample_ac``) + T2
where T2u-ac has no plan; ``up_kernel="pow2"`` takes the gather there (the single-pass kernel is an align_corners=False kernel).

``up_kernel`` chooses T2u's kernel for ``upsampled``: ``"gather"`` (the default: csrc/train_loss_up.hip, any ratio, two
launches) or ``"pow2"`` (csrc/train_loss_up_pow2.hip: forward and gradient in one pass for ``CrossEntropy`` on a prediction
that is exactly 1/4 or 1/16 of the labels on both axes; any other prediction goes where ``"gather"`` sends it).
``OhemCrossEntropy`` accepts the argument and keeps the gather kernels: its selection needs every loss before any gradient."""
from __future__ import annotations

import torch
from torch import Tensor, nn
from torch.nn import functional as F

__all__ = ["CrossEntropy", "OhemCrossEntropy", "Dice"]


class _NativeCriterion(torch.autograd.Function):
    """T2: forward (+ OHEM select) and backward of one prediction; the gradient is for ``preds`` only."""

    @staticmethod
    def forward(ctx, preds, labels, weight, ignore_label, thresh, ohem):
        from . import _native as N
        loss, loss_px, words = N.train_ce_forward(preds, labels, weight, ignore_label, thresh, ohem)
        ctx.save_for_backward(preds, labels, loss_px, words)
        ctx.weight, ctx.ignore_label, ctx.ohem = weight, ignore_label, ohem
        ctx.mark_non_differentiable(words)
        return loss, words   # fp32 whatever the logits' dtype (what autocast makes of F.cross_entropy)

    @staticmethod
    def backward(ctx, g, _g_words):
        from . import _native as N
        preds, labels, loss_px, words = ctx.saved_tensors
        return (N.train_ce_backward(preds, labels, ctx.weight, ctx.ignore_label, ctx.ohem, loss_px, words, g),
                None, None, None, None, None)


def _native_forward(module, preds, labels, thresh, ohem):
    from . import _native as N
    if not (preds.is_cuda and labels.is_cuda):
        raise N.SeaNativeError("native=True criteria work on HIP device tensors only (no CPU fallback)")
    if not preds.is_contiguous():
        if preds.dim() == 4 and preds.is_contiguous(memory_format=torch.channels_last):
            return None            # channels_last: no T2 kernel for that layout, the torch criterion runs (module docstring)
        raise N.SeaNativeError("native=True criteria take dense NCHW (or channels_last) logits; got strides "
                               f"{tuple(preds.stride())} for shape {tuple(preds.shape)}: call .contiguous() first")
    w = module.criterion.weight
    loss, module.last_words = _NativeCriterion.apply(preds, labels, None if w is None else w.detach().float(),
                                                     module.criterion.ignore_index, thresh, ohem)
    return loss


class _NativeCriterionUp(torch.autograd.Function):
    """T2u: as ``_NativeCriterion`` on low-resolution logits; the labels' size is the up-sampling target."""

    @staticmethod
    def forward(ctx, low, labels, weight, ignore_label, thresh, ohem, align_corners=False):
        from . import _native as N
        loss, loss_px, words = N.train_ce_up_forward(low, labels.shape[-2:], labels, weight, ignore_label, thresh, ohem,
                                                     align_corners=align_corners)
        ctx.save_for_backward(low, labels, loss_px, words)
        ctx.weight, ctx.ignore_label, ctx.ohem, ctx.align_corners = weight, ignore_label, ohem, align_corners
        ctx.mark_non_differentiable(words)
        return loss, words

    @staticmethod
    def backward(ctx, g, _g_words):
        from . import _native as N
        low, labels, loss_px, words = ctx.saved_tensors
        return (N.train_ce_up_backward(low, labels.shape[-2:], labels, ctx.weight, ctx.ignore_label, ctx.ohem, loss_px,
                                       words, g, align_corners=ctx.align_corners), None, None, None, None, None, None)


class _NativeCriterionUpPow2(torch.autograd.Function):
    """T2u for x4 / x16, mean-reduced cross-entropy: the forward leaves the un-normalised gradient, the backward scales it."""

    @staticmethod
    def forward(ctx, low, labels, weight, ignore_label):
        from . import _native as N
        loss, raw, words = N.train_ce_up_pow2_forward(low, labels.shape[-2:], labels, weight, ignore_label)
        ctx.save_for_backward(raw, words)
        ctx.mark_non_differentiable(words)
        return loss, words

    @staticmethod
    def backward(ctx, g, _g_words):
        from . import _native as N
        raw, words = ctx.saved_tensors
        return N.train_ce_up_pow2_backward(raw, words, g), None, None, None


UP_KERNELS = ("gather", "pow2")


def _check_up_kernel(up_kernel):
    if up_kernel not in UP_KERNELS:
        raise ValueError(f"up_kernel must be one of {UP_KERNELS}, got {up_kernel!r}")
    return up_kernel


def _upsample(p, labels, align_corners=False):
    return F.interpolate(p, size=labels.shape[-2:], mode="bilinear", align_corners=align_corners)


class _AuxWeighted(nn.Module):
    aux_weights: list

    def _forward(self, preds, labels):
        raise NotImplementedError

    def forward(self, preds, labels: Tensor) -> Tensor:
        if isinstance(preds, tuple):
            return sum(w * self._forward(p, labels) for p, w in zip(preds, self.aux_weights))
        return self._forward(preds, labels)


class _Upsampled(_AuxWeighted):
    """``upsampled`` of the two cross-entropy criteria (module docstring)."""
    _ohem = False

    def _thresh(self) -> float:
        return 0.0

    def upsampled(self, preds_low, labels: Tensor, align_corners: bool = False) -> Tensor:
        align_corners = bool(align_corners)
        if isinstance(preds_low, tuple):
            return sum(w * self._upsampled(p, labels, align_corners) for p, w in zip(preds_low, self.aux_weights))
        return self._upsampled(preds_low, labels, align_corners)

    def _upsampled(self, low, labels, align_corners=False):
        if self.native:
            from . import _native as N
            if not (low.is_cuda and labels.is_cuda):
                raise N.SeaNativeError("native=True criteria work on HIP device tensors only (no CPU fallback)")
            w = self.criterion.weight
            if align_corners:
                if low.dim() == 4 and N.train_ce_up_supported(low, labels.shape[-2:], align_corners=True):
                    loss, self.last_words = _NativeCriterionUp.apply(
                        low.float().contiguous(), labels, None if w is None else w.detach().float(),
                        self.criterion.ignore_index, self._thresh(), self._ohem, True)
                    return loss
                from .models.pspnet import _up_ac_train   # no T2u-ac kernel for this shape: P2 up-sampling + T2
                return self._forward(_up_ac_train(low.float(), labels.shape[-2:]), labels)
            if (self.up_kernel == "pow2" and not self._ohem
                    and N.train_ce_up_pow2_supported(low, labels.shape[-2:])):
                loss, self.last_words = _NativeCriterionUpPow2.apply(
                    low.float().contiguous(), labels, None if w is None else w.detach().float(),
                    self.criterion.ignore_index)
                return loss
            if low.dim() == 4 and N.train_ce_up_supported(low, labels.shape[-2:]):
                loss, self.last_words = _NativeCriterionUp.apply(
                    low.float().contiguous(), labels, None if w is None else w.detach().float(),
                    self.criterion.ignore_index, self._thresh(), self._ohem)
                return loss
            from .models.convnext_upernet import _up   # no T2u kernel for this shape: M2 up-sampling + T2
            return self._forward(_up(low, labels.shape[-2:]), labels)
        return self._forward(_upsample(low, labels, align_corners), labels)


class CrossEntropy(_Upsampled):
    def __init__(self, ignore_label: int = 255, weight: Tensor = None, aux_weights=(1, 0.4, 0.4),
                 native: bool = False, up_kernel: str = "gather") -> None:
        super().__init__()
        self.aux_weights = list(aux_weights)
        self.native = native
        self.up_kernel = _check_up_kernel(up_kernel)
        self.last_words = None      # native: the device words of the last prediction (debugging / tests)
        self.criterion = nn.CrossEntropyLoss(weight=weight, ignore_index=ignore_label)

    def _forward(self, preds, labels):
        if self.native:
            loss = _native_forward(self, preds, labels, 0.0, False)
            if loss is not None:
                return loss
        return self.criterion(preds, labels)


class OhemCrossEntropy(_Upsampled):
    _ohem = True

    def _thresh(self) -> float:
        return float(self.thresh)

    def __init__(self, ignore_label: int = 255, weight: Tensor = None, thresh: float = 0.7, aux_weights=(1, 1),
                 native: bool = False, up_kernel: str = "gather") -> None:
        super().__init__()
        self.ignore_label = ignore_label
        self.aux_weights = list(aux_weights)
        self.native = native
        self.up_kernel = _check_up_kernel(up_kernel)   # accepted, not used: OHEM keeps the gather kernels
        self.last_words = None
        self.thresh = -torch.log(torch.tensor(thresh, dtype=torch.float))
        self.criterion = nn.CrossEntropyLoss(weight=weight, ignore_index=ignore_label, reduction="none")

    def _forward(self, preds, labels):
        if self.native:
            loss = _native_forward(self, preds, labels, float(self.thresh), True)
            if loss is not None:
                return loss
        n_min = labels[labels != self.ignore_label].numel() // 16
        loss = self.criterion(preds, labels).view(-1)
        hard = loss[loss > self.thresh]
        if hard.numel() < n_min:
            hard, _ = loss.topk(n_min)
        return torch.mean(hard)


class Dice(_AuxWeighted):
    def __init__(self, delta: float = 0.5, aux_weights=(1, 0.4, 0.4)):
        super().__init__()
        self.delta = delta
        self.aux_weights = list(aux_weights)

    def _forward(self, preds, labels):
        k = preds.shape[1]
        onehot = F.one_hot(labels, k).permute(0, 3, 1, 2)
        tp = torch.sum(onehot * preds, dim=(2, 3))
        fn = torch.sum(onehot * (1 - preds), dim=(2, 3))
        fp = torch.sum((1 - onehot) * preds, dim=(2, 3))
        score = (tp + 1e-6) / (tp + self.delta * fn + (1 - self.delta) * fp + 1e-6)
        return (torch.sum(1 - score, dim=-1) / k).mean()


def get_loss(loss_fn_name: str = "CrossEntropy", ignore_label: int = 255, cls_weights: Tensor = None,
             native: bool = False, up_kernel: str = "gather"):
    assert loss_fn_name in __all__, f"Unavailable loss function name >> {loss_fn_name}.\nAvailable loss functions: {__all__}"
    if loss_fn_name == "Dice":
        return Dice()
    return {"CrossEntropy": CrossEntropy, "OhemCrossEntropy": OhemCrossEntropy}[loss_fn_name](ignore_label, cls_weights,
                                                                                        native=native,
                                                                                        up_kernel=up_kernel)
