"""Sliding-window evaluation of a segmentation model (counterpart of semseg/utils/segmenter_eval.py): how a Segmenter
is evaluated on images that are not ``window_size`` squares.  The (resized) image is covered with ``window_size``
windows at ``window_stride``, the window logits are averaged where they overlap, resized to the original size and turned
into probabilities.  ``padding``, ``unpadding``, ``resize`` and ``sliding_window`` follow the reference's rules; the
merge runs in libsea_hip's K11 kernels (``_native.sw_merge`` / ``sw_finish``) as a gather: no sum, count, quotient or
resized copy of the logits is written, and with a ``forward_lowres`` model not even the full-resolution window logits.
``SlidingWindowModel`` is the same protocol as a differentiable module (window cut K11c, merge K11a, their adjoints K11c'
and K11a'), so that the attacks of ``semseg.attacker`` run on whole images.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import _native as N
from ..attacker import _FrozenParameters

__all__ = ["padding", "unpadding", "resize", "sliding_window", "sw_anchors", "merge_windows", "inference",
           "SlidingWindowModel"]


def padding(im, patch_size, fill_value=0):
    """pad H and W on the bottom / right up to multiples of ``patch_size`` (segmenter_eval.py:9-20)"""
    H, W = im.size(2), im.size(3)
    pad_h = patch_size - (H % patch_size) if H % patch_size > 0 else 0
    pad_w = patch_size - (W % patch_size) if W % patch_size > 0 else 0
    if pad_h > 0 or pad_w > 0:
        return F.pad(im, (0, pad_w, 0, pad_h), value=fill_value)
    return im


def unpadding(y, target_size):
    """crop what ``padding`` added (segmenter_eval.py:23-33)"""
    H, W = target_size
    extra_h, extra_w = y.size(2) - H, y.size(3) - W
    if extra_h > 0:
        y = y[:, :, :-extra_h]
    if extra_w > 0:
        y = y[:, :, :, :-extra_w]
    return y


def _resize_target(h, w, smaller_size):
    """segmenter_eval.py:36-45: the short side becomes ``smaller_size``, the long one ``int(ratio * smaller_size)`` with the
    ratio a Python float; None when the short side is already large enough"""
    if h < w:
        h_res, w_res = smaller_size, (w / h) * smaller_size
    else:
        h_res, w_res = (h / w) * smaller_size, smaller_size
    return (int(h_res), int(w_res)) if min(h, w) < smaller_size else None


def resize(im, smaller_size):
    """up-scale (bilinear, align_corners=False) so that the short side is ``smaller_size``; larger images are returned
    untouched (segmenter_eval.py:36-48).  Device tensors go through libsea_hip's up-sampling kernel (M2)."""
    size = _resize_target(int(im.shape[2]), int(im.shape[3]), smaller_size)
    if size is None:
        return im
    if im.is_cuda:
        return N.upsample_bilinear(im.float().contiguous(), size)
    return F.interpolate(im, size, mode="bilinear")


def sw_anchors(H, W, window_size, window_stride):
    """the window origins of an (H, W) image per axis (segmenter_eval.py:56-59): every multiple of the stride below
    ``n - window_size``, then ``n - window_size`` itself.  Pure host code.  A stride above the window would leave pixels
    uncovered (the reference then divides 0 by 0): ValueError."""
    H, W, ws, st = int(H), int(W), int(window_size), int(window_stride)
    if st < 1 or ws < 1:
        raise ValueError(f"window_size {ws} and window_stride {st} must be positive")
    if st > ws:
        raise ValueError(f"window_stride {st} > window_size {ws} leaves pixels uncovered")
    if H < ws or W < ws:
        raise ValueError(f"image {H}x{W} is smaller than the window {ws} (resize it first)")
    return ([a for a in range(0, H, st) if a < H - ws] + [H - ws], [a for a in range(0, W, st) if a < W - ws] + [W - ws])


def sliding_window(im, flip, window_size, window_stride):
    """the reference's window dictionary (segmenter_eval.py:51-67): ``crop`` = one (B, C, ws, ws) view per window, h anchor
    outer, w anchor inner, ``anchors`` = their (ha, wa), plus ``flip`` and ``shape``"""
    B, C, H, W = im.shape
    ws = window_size
    h_anchors, w_anchors = sw_anchors(H, W, ws, window_stride)
    windows = {"crop": [], "anchors": []}
    for ha in h_anchors:
        for wa in w_anchors:
            windows["crop"].append(im[:, :, ha:ha + ws, wa:wa + ws])
            windows["anchors"].append((ha, wa))
    windows["flip"] = flip
    windows["shape"] = (H, W)
    return windows


def _merge(seg_maps, window_size, h_anchors, w_anchors, shape, ori_shape, flip, out=None, accumulate=False):
    """(B * n_win, C, hl, wl) window logits -> (B, C, *ori_shape) probabilities: K11a alone when the original size is the
    merged one, else K11a (averaged logits) + K11b (resize, flip, softmax)"""
    shape, ori_shape = (int(shape[0]), int(shape[1])), (int(ori_shape[0]), int(ori_shape[1]))
    if ori_shape == shape:
        return N.sw_merge(seg_maps, window_size, h_anchors, w_anchors, shape, softmax=True, flip=flip, out=out,
                          accumulate=accumulate)
    avg = N.sw_merge(seg_maps, window_size, h_anchors, w_anchors, shape)
    return N.sw_finish(avg, ori_shape, flip=flip, out=out, accumulate=accumulate)


def merge_windows(windows, window_size, ori_shape):
    """softmax_C of the overlap-averaged window logits at ``ori_shape`` (segmenter_eval.py:70-92).  ``windows`` is the
    reference's dictionary: ``anchors`` (h outer, w inner, as ``sliding_window`` lists them), ``shape``, ``flip`` and
    ``seg_maps``, the (n_win, C, ws, ws) logits of one image -> (C, *ori_shape) as in the reference, or of B images with
    the leading dimension B * n_win, image-major -> (B, C, *ori_shape).  ``seg_maps`` may also hold the models'
    ``forward_lowres`` logits (smaller than the window): their up-sampling is then done inside the merge."""
    anchors = [(int(a), int(b)) for a, b in windows["anchors"]]
    h_anchors, w_anchors = sorted({a for a, _ in anchors}), sorted({b for _, b in anchors})
    if anchors != [(a, b) for a in h_anchors for b in w_anchors]:
        raise ValueError("merge_windows: anchors must be the product of ascending h and w anchors, h outer")
    seg_maps = windows["seg_maps"]
    if not torch.is_tensor(seg_maps):
        seg_maps = torch.stack(list(seg_maps))
    seg_maps = seg_maps.float().contiguous()
    res = _merge(seg_maps, window_size, h_anchors, w_anchors, windows["shape"], ori_shape, bool(windows["flip"]))
    return res[0] if seg_maps.shape[0] == len(anchors) else res


def _window_logits(model, x):
    """logits of a chunk of windows: ``forward_lowres`` (before the model's final bilinear up-sampling) when the model
    offers it and it returns a tensor for this size, else ``model(x)``"""
    if hasattr(model, "forward_lowres"):
        r = model.forward_lowres(x)
        if isinstance(r, (tuple, list)):
            r = r[0]
        if torch.is_tensor(r):
            return r.float().contiguous()
    return model(x).float().contiguous()


@torch.no_grad()
def inference(model, ims, window_size, window_stride, batch_size, ori_shape=None, n_cls=None, flip=False, out=None,
              accumulate=False):
    """Sliding-window class probabilities (B, C, *ori_shape) of a device batch ``ims`` (B, 3, h, w):

    1. ``resize`` when the short side is below ``window_size``; 2. mirror along W when ``flip``; 3. cut the windows of
    all B images, image-major; 4. run them through ``model.forward_lowres`` (when the model has it and returns a tensor
    for the window size) or ``model``, ``batch_size`` windows at a time, without gradients and with frozen parameters;
    5. gather the chunks in one (B * n_win, C, hl, wl) buffer; 6. merge (K11) -- overlap average, resize to ``ori_shape``
    (default: the input's own size), un-mirror, softmax; 7. return the probabilities, written to ``out`` when given and
    added to it with ``accumulate``.  ``n_cls`` checks the model's class count.

    Differences from the reference's ``inference`` (segmenter_eval.py:95-123), which cannot serve as a specification: it
    hard-codes C = 151, ``ori_shape = (512, 512)`` and ``"cuda"``; keeps only image 0 of the batch
    (``torch.stack(crops)[:, 0]``), broadcasts that one map over ``batch_size`` rows and divides it by ``len(ims)``; and
    prints.  Here row ``i`` of the result is what the reference's ``sliding_window`` and ``merge_windows`` give for
    ``ims[i:i+1]``."""
    if ims.dim() != 4:
        raise ValueError(f"inference: expected (B, 3, h, w) images, got {tuple(ims.shape)}")
    ws = int(window_size)
    if ori_shape is None:
        ori_shape = tuple(ims.shape[2:])
    ims = resize(ims.float().contiguous(), ws)
    if flip:
        ims = ims.flip(3)
    B, _, H, W = ims.shape
    h_anchors, w_anchors = sw_anchors(H, W, ws, window_stride)
    n_win = len(h_anchors) * len(w_anchors)
    if n_win == 1:
        crops = ims
    else:
        crops = torch.stack([ims[:, :, ha:ha + ws, wa:wa + ws] for ha in h_anchors for wa in w_anchors], 1).flatten(0, 1)
    n_rows, step = B * n_win, max(1, int(batch_size))
    seg_maps = None
    with _FrozenParameters(model):
        for i in range(0, n_rows, step):
            logits = _window_logits(model, crops[i:i + step].contiguous())
            if n_cls is not None and logits.shape[1] != int(n_cls):
                raise ValueError(f"model returned {logits.shape[1]} classes, expected {int(n_cls)}")
            if step >= n_rows:
                seg_maps = logits
            else:
                if seg_maps is None:
                    seg_maps = torch.empty((n_rows, *logits.shape[1:]), dtype=torch.float32, device=logits.device)
                seg_maps[i:i + step] = logits
    return _merge(seg_maps, ws, h_anchors, w_anchors, (H, W), ori_shape, bool(flip), out=out, accumulate=accumulate)


class _SwCut(torch.autograd.Function):
    """K11c forward, K11c' backward"""

    @staticmethod
    def forward(ctx, x, ws, h_anchors, w_anchors):
        ctx.args = (ws, h_anchors, w_anchors, tuple(x.shape[2:]))
        return N.sw_cut(x, ws, h_anchors, w_anchors)

    @staticmethod
    def backward(ctx, dcrops):
        ws, h_anchors, w_anchors, size = ctx.args
        return N.sw_cut_backward(dcrops.contiguous(), ws, h_anchors, w_anchors, size), None, None, None


class _SwMerge(torch.autograd.Function):
    """K11a (averaged logits) forward, K11a' backward"""

    @staticmethod
    def forward(ctx, logits, ws, h_anchors, w_anchors, size):
        ctx.args = (ws, h_anchors, w_anchors, tuple(logits.shape[2:]))
        return N.sw_merge(logits, ws, h_anchors, w_anchors, size)

    @staticmethod
    def backward(ctx, g):
        ws, h_anchors, w_anchors, logits_size = ctx.args
        return N.sw_merge_backward(g.contiguous(), ws, h_anchors, w_anchors, logits_size), None, None, None, None


class SlidingWindowModel(torch.nn.Module):
    """``model`` evaluated through sliding windows, as a model: (B, 3, H, W) -> the overlap-averaged LOGITS (B, C, H, W) of
    ``merge_windows`` (whose probabilities are their softmax), differentiable with respect to the input.  The attacks
    (``apgd_train``, ``apgd_largereps``) take it like any other model and then attack the protocol that
    ``inference`` / ``evaluate_sliding`` score.

    1. cut the windows of all B images (K11c); 2. window logits ``batch_size`` windows at a time (default: all at once),
    from ``model.forward_lowres`` when the model offers it; 3. merge (K11a), the model's final up-sampling inside for
    low-resolution logits.  The backward runs the adjoints K11a' and K11c'.  An image that is exactly one window is the
    model itself: ``model(x)`` is returned.  There is no resizing (the attack's labels have the image's size): an image
    smaller than the window is a ValueError.  Nothing is read by the host, so the forward can be captured in a HIP graph.
    The wrapper deliberately has no ``forward_lowres``: its logits are full resolution.  ``training`` is the inner
    model's flag."""

    def __init__(self, model, window_size, window_stride, batch_size=None):
        super().__init__()
        ws, st = int(window_size), int(window_stride)
        if ws < 1 or st < 1:
            raise ValueError(f"window_size {ws} and window_stride {st} must be positive")
        if st > ws:
            raise ValueError(f"window_stride {st} > window_size {ws} leaves pixels uncovered")
        if batch_size is not None and int(batch_size) < 1:
            raise ValueError(f"batch_size {batch_size} must be positive")
        if not isinstance(model, torch.nn.Module):
            raise TypeError("SlidingWindowModel wraps an nn.Module")
        self.model = model
        self.window_size, self.window_stride = ws, st
        self.batch_size = None if batch_size is None else int(batch_size)

    # ``training`` is not a flag of the wrapper's own: it reads the inner model's, and assigning to it (nn.Module.__init__,
    # train(), or a caller setting ``wrapper.training`` alone) changes nothing.  train() / eval() still reach the inner model,
    # because nn.Module.train() recurses into the children.
    @property
    def training(self):
        inner = self.__dict__.get("_modules", {}).get("model")
        return True if inner is None else inner.training

    @training.setter
    def training(self, mode):
        pass

    def forward(self, x):
        if x.dim() != 4:
            raise ValueError(f"SlidingWindowModel: expected (B, 3, H, W) images, got {tuple(x.shape)}")
        B, _, H, W = x.shape
        ws = self.window_size
        h_anchors, w_anchors = sw_anchors(H, W, ws, self.window_stride)      # ValueError for an image below the window
        n_win = len(h_anchors) * len(w_anchors)
        if n_win == 1:
            return self.model(x)
        crops = _SwCut.apply(x.float().contiguous(), ws, h_anchors, w_anchors)
        n_rows = B * n_win
        step = n_rows if self.batch_size is None else self.batch_size
        if step >= n_rows:
            logits = _window_logits(self.model, crops)
        else:
            logits = torch.cat([_window_logits(self.model, crops[i:i + step]) for i in range(0, n_rows, step)])
        return _SwMerge.apply(logits, ws, h_anchors, w_anchors, (H, W))
