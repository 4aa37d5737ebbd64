"""Multi-scale + flip evaluation as a differentiable model: attack what ``semseg.val.evaluate_msf`` scores.

``evaluate_msf`` predicts with an ensemble: for every scale, plain and mirrored, the input is resized (K10a), the model
runs, and the softmax of its logits, resized back, is added to one score buffer (K10b).  ``MsfModel`` is that protocol
as an ``nn.Module`` whose output the attacks (``apgd_train``, ``apgd_largereps``, ``tools/infer.py``) take like any
model's logits, with the adjoints K10a', K10g and K10r' of ``csrc/msf_grad.hip`` as its backward.
"""
from __future__ import annotations

import torch

from .. import _native as N
from ..val import _msf_logits, msf_scaled_size

__all__ = ["MsfModel"]

FLT_MIN = float(torch.finfo(torch.float32).tiny)
SHAPES_KEPT = 4          # batch shapes whose score buffer and workspace a wrapper keeps


class _Resize(torch.autograd.Function):
    """K10a forward (both images in one pass), K10a' backward (both gradients in one launch)"""

    @staticmethod
    def forward(ctx, x, size, flip):
        ctx.in_size = tuple(x.shape[2:])
        x_s, x_f = N.msf_resize_input(x, size, flip=flip)
        if not flip:
            return x_s
        return x_s, x_f

    @staticmethod
    def backward(ctx, *gs):
        g = gs[0]
        g_f = gs[1] if len(gs) > 1 else None
        g = None if g is None else g.contiguous()
        g_f = None if g_f is None else g_f.contiguous()
        return N.msf_resize_input_backward(g, g_f, ctx.in_size), None, None


class _Accumulate(torch.autograd.Function):
    """K10b forward, in place in the score buffer; backward: the score's gradient passes through unchanged, the logits'
    is K10g + K10r' (+ M2's backward for ``forward_lowres`` logits)"""

    @staticmethod
    def forward(ctx, score, logits, size, flip, workspace):
        ctx.args = (size, flip, workspace)
        ctx.save_for_backward(logits)
        N.msf_accumulate(logits, score, size, flip=flip)
        ctx.mark_dirty(score)
        return score

    @staticmethod
    def backward(ctx, dscore):
        size, flip, workspace = ctx.args
        (logits,) = ctx.saved_tensors
        dscore = dscore.contiguous()
        dlogits = N.msf_accumulate_backward(logits, dscore, size, flip=flip, workspace=workspace)
        return (dscore if ctx.needs_input_grad[0] else None), dlogits, None, None, None


class _LogScore(torch.autograd.Function):
    """z = log(max(score, FLT_MIN)); dscore = dz / score, 0 where the clamp was active"""

    @staticmethod
    def forward(ctx, score):
        ctx.save_for_backward(score)
        return torch.log(score.clamp_min(FLT_MIN))

    @staticmethod
    def backward(ctx, dz):
        (score,) = ctx.saved_tensors
        return (dz / score).masked_fill_(score < FLT_MIN, 0.0)


class MsfModel(torch.nn.Module):
    """``model`` evaluated at several scales (+ horizontal flip), as a model: (B, 3, H, W) -> z = log(max(score, FLT_MIN)),
    (B, C, H, W), where ``score`` is the buffer ``evaluate_msf`` holds for that batch: the same K10a / K10b calls in the
    same order (scales; plain before mirrored), ``forward_lowres`` logits when the inner model offers them (the rule of
    ``val._msf_logits``).  ``softmax(z)`` is the ensemble's mean probability and ``argmax z`` its prediction, so the
    attack losses, all soft-max based, see the scored ensemble.  ``score(x)`` returns the raw buffer without a gradient.

    The backward: dscore = dz / score (0 where the clamp was active); then per pass K10g (softmax backward at label
    resolution), K10r' (adjoint of the resize back, onto the scaled grid), M2's backward for ``forward_lowres`` logits,
    the model's own backward, and K10a' (adjoint of the input resize, plain and mirrored gradient in one launch).  All
    are gathers in a fixed order: the gradient is bitwise reproducible.

    Nothing is read by the host, so ``ApgdRun`` captures forward and backward in its HIP-graph pair; the score buffer and
    the K10g workspace belong to the wrapper and keep their addresses between calls of one shape.  A call overwrites the
    score buffer: the graph of an earlier call of that shape can no longer be differentiated.

    Applies to models that accept ``msf_scaled_size`` inputs (multiples of 32).  PSPNet, which needs
    ``(n - 1) % 8 == 0``, does not, exactly as in ``evaluate_msf``.  The wrapper deliberately has no ``forward_lowres``: its
    output is full resolution.  ``training`` is the inner model's flag.

    ``ValueError``: no scales, a non-positive scale, an input that is not 4-D (all before any launch), and more than 192
    classes (K10b's limit): at construction when ``n_classes`` is given, else when the first pass's logits show it,
    before any K10b launch."""

    def __init__(self, model, scales, flip=False, n_classes=None):
        super().__init__()
        scales = [float(s) for s in scales]
        if n_classes is not None and int(n_classes) > N.MSF_MAX_CLASSES:
            raise ValueError(f"MsfModel supports up to {N.MSF_MAX_CLASSES} classes, got {int(n_classes)}")
        if not scales:
            raise ValueError("MsfModel: no scales")
        if any(not s > 0 for s in scales):
            raise ValueError(f"MsfModel: scales must be positive, got {scales}")
        if not isinstance(model, torch.nn.Module):
            raise TypeError("MsfModel wraps an nn.Module")
        self.model = model
        self.scales, self.flip = tuple(scales), bool(flip)
        self.__dict__["_held"] = {}          # (B, C, H, W, device) -> (score, workspace); plain attributes, not nn buffers

    # ``training`` is the inner model's flag (see SlidingWindowModel)
    @property
    def training(self):
        inner = self.__dict__.get("_modules", {}).get("model")
        return True if inner is None else inner.training

    @training.setter
    def training(self, mode):
        pass

    def _buffers_for(self, shape, device):
        key = (*shape, str(device))
        held = self.__dict__["_held"]
        pair = held.pop(key, None)
        if pair is None:
            # the most recently used shapes stay (an evaluation has a full and a ragged last batch, and a captured attack
            # step of either addresses its pair): more than ApgdRun's cache keeps graphs for
            while len(held) >= SHAPES_KEPT:
                held.pop(next(iter(held)))
            pair = (torch.empty(shape, dtype=torch.float32, device=device),
                    torch.empty(shape, dtype=torch.float32, device=device))
        held[key] = pair                     # (re-inserted: the dict keeps the most recently used shape last)
        return pair

    def _accumulate(self, x):
        if x.dim() != 4:
            raise ValueError(f"MsfModel: expected (B, 3, H, W) images, got {tuple(x.shape)}")
        x = x.float().contiguous()
        B, _, H, W = x.shape
        sizes = [msf_scaled_size(scale, H, W) for scale in self.scales]
        if min(min(size) for size in sizes) < 1:
            raise ValueError(f"MsfModel: scales {self.scales} of a {H}x{W} image give the sizes {sizes}")
        score = ws = None
        for size in sizes:
            xs = _Resize.apply(x, size, self.flip)
            for flipped, x_in in enumerate(xs if self.flip else (xs,)):
                logits = _msf_logits(self.model, x_in)
                if score is None:
                    C = logits.shape[1]
                    if logits.dim() != 4 or logits.shape[0] != B:
                        raise ValueError(f"MsfModel: the model returned {tuple(logits.shape)} for {tuple(x_in.shape)}")
                    if C > N.MSF_MAX_CLASSES:
                        raise ValueError(f"MsfModel supports up to {N.MSF_MAX_CLASSES} classes, got {C}")
                    buf, ws = self._buffers_for((B, C, H, W), x.device)
                    score = buf.detach().zero_()
                score = _Accumulate.apply(score, logits, size, bool(flipped), ws)
        return score

    def forward(self, x):
        return _LogScore.apply(self._accumulate(x))

    @torch.no_grad()
    def score(self, x):
        """the raw score buffer of ``evaluate_msf`` for this batch (owned by the wrapper: the next call overwrites it)"""
        return self._accumulate(x)
