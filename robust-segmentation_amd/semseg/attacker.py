"""SEA attack engine: APGD (L-inf) with the SEA losses, device-resident on MI355X.

Call-compatible with the reference module of the same name (semseg/attacker.py): same function
names, positional order, defaults and return tuples, so ``tools/infer.py`` style callers such as

    attack_fn = partial(attacker.apgd_largereps, norm="Linf", eps=eps/255, n_iter=300, use_rs=True,
                        loss="mask-ce-bal", track_loss="ce-avg", early_stop=True, num_classes=C)
    x_adv, _, acc = attack_fn(model, x.clone(), y, weights)

work unchanged.  What differs is HOW an iteration runs:

* the ~14 element-wise launches of the step (reference lines 389-410) are one kernel (K1);
* loss forward, its logit gradient, the tracking loss, per-image accuracy and the argmax are one
  kernel over the (B,C,H,W) logits (K2, closed-form gradients, JS in closed form);
* every per-image decision (best-adv, best-loss, oscillation check, step halving, early stop) is
  taken by a one-block kernel on the device (K4/K7) and applied by one conditional-copy kernel:
  the loop never calls ``.nonzero()``, ``.cpu()`` or ``.sum() > 0`` and never launches the
  2*n_cls-iteration ``compute_iou_acc`` unless ``verbose``.

Only device tensors are accepted: there is no CPU fallback (see semseg/_native.py).
"""
from __future__ import annotations

from functools import partial

import os
import weakref

import torch

from . import _native as N

__all__ = [
    "apgd_train", "apgd_largereps", "apgd_restarts", "criterion_dict", "masked_cross_entropy",
    "masked_cross_entropy_balanced", "js_loss", "js_div_fn", "pixel_to_img_loss", "compute_iou_acc",
    "check_oscillation", "Logger",
]


class Logger:
    """print + append to file (the autoattack.other_utils.Logger the reference imports, attacker.py:6)."""

    def __init__(self, log_path=None):
        self.log_path = log_path

    def log(self, str_to_log):
        print(str_to_log)
        if self.log_path is not None:
            with open(self.log_path, "a") as f:
                f.write(str_to_log + "\n")
                f.flush()


# ---------------------------------------------------------------------------------------------------
# differentiable per-pixel losses (API surface of reference lines 143-257)
# ---------------------------------------------------------------------------------------------------
class _PixelLoss(torch.autograd.Function):
    """loss map (B,H,W) of one SEA loss; backward = closed-form d loss/d logits times the upstream
    per-pixel gradient (the mask of the masked losses is detached in the reference, line 148)."""

    @staticmethod
    def forward(ctx, logits, target, weights, mode):
        B, Cc, H, W = logits.shape
        lg = logits.detach()
        loss_px = torch.empty(B, H, W, dtype=torch.float32, device=logits.device)
        need_grad = logits.requires_grad
        r = N.loss_fwd_bwd(lg, target.contiguous(), weights, mode, mode, 1.0, want_grad=need_grad, loss_px=loss_px)
        if need_grad:
            ctx.save_for_backward(r["dlogits"])
        ctx.has_grad = need_grad
        return loss_px

    @staticmethod
    def backward(ctx, g):
        if not ctx.has_grad:
            return None, None, None, None
        (dl,) = ctx.saved_tensors
        return dl * g.unsqueeze(1).to(dl.dtype), None, None, None


def _loss_map(pred, target, weights, mode):
    if weights is not None:
        weights = weights.to(device=pred.device, dtype=torch.float32)
    return _PixelLoss.apply(pred, target, weights, mode)


def masked_cross_entropy(pred, target, weights=None, reduction="none", ignore_index=-1):
    """Cross-entropy of only correctly classified pixels (reference lines 143-152)."""
    loss = _loss_map(pred, target, None, 0)
    if reduction == "mean":
        return loss.view(pred.shape[0], -1).mean(-1)
    return loss


def masked_cross_entropy_balanced(pred, target, weights=None, reduction="none", ignore_index=-1):
    """Class-balanced cross-entropy of only correctly classified pixels (reference lines 155-173)."""
    loss = _loss_map(pred, target, weights, 1)
    if reduction == "mean":
        return loss.view(pred.shape[0], -1).mean(-1)
    return loss


def _is_class_dim(red_dim) -> bool:
    return red_dim in (1, (1,), [1])


def js_div_fn(p, q, weights=None, softmax_output=False, reduction="none", red_dim=None, ignore_index=-1):
    """JS divergence between softmax(p) and one-hot(q) (reference lines 187-226).

    The configuration the attack uses (logits in, ``reduction="none"``, summed over the class dim: what
    ``js_loss`` passes) runs in the fused kernel K2 in closed form (NaN-free).  Every other
    argument combination is cold API surface and is composed from device tensor ops with the reference's
    semantics, including its quirks: ``reduction != "none"`` raises unless every pixel is ignored (line 209),
    ignored pixels contribute 0, and a soft-max that underflows to exactly 0 yields NaN like the reference."""
    if not softmax_output and reduction == "none" and _is_class_dim(red_dim):
        return _loss_map(p, q, None, 2)
    prob = p if softmax_output else torch.softmax(p, 1)
    keep = q != ignore_index
    if reduction != "none" and bool(keep.any()):
        raise ValueError("Incompatible setup.")
    onehot = torch.zeros_like(prob).scatter_(1, torch.where(keep, q, torch.zeros_like(q)).unsqueeze(1), 1.0)
    log_m = ((prob + onehot) / 2).log()
    kl = torch.nn.functional.kl_div
    loss = (kl(log_m, prob, reduction=reduction) + kl(log_m, onehot, reduction=reduction)) / 2
    loss = keep.unsqueeze(1).to(loss.dtype) * loss
    if red_dim is not None:
        assert reduction == "none", "Incompatible setup."
        loss = loss.sum(dim=red_dim)
    return loss


def js_loss(p, q, num_classes=21, reduction="mean"):
    loss = js_div_fn(p, q, red_dim=(1))
    if reduction == "mean":
        return loss.view(p.shape[0], -1).mean(-1)
    elif reduction == "none":
        return loss


def _ce(x, y, *unused):
    # the reference's 2-argument lambdas (lines 252-253) make `loss="ce"` a TypeError inside apgd_train
    # (SURVEY fact 3 / D3); accepting the ignored third argument keeps those call sites alive.
    return _loss_map(x, y, None, 3)


def pixel_to_img_loss(loss, mask_background=None):
    if mask_background is not None:
        loss = mask_background * loss
    return loss.view(loss.shape[0], -1).mean(-1)


criterion_dict = {
    "ce": _ce,
    "ce-avg": _ce,
    "mask-ce-avg": masked_cross_entropy,
    "mask-ce-bal": masked_cross_entropy_balanced,
    "js-avg": partial(js_loss, reduction="none"),
}


# ---------------------------------------------------------------------------------------------------
# statistics helpers
# ---------------------------------------------------------------------------------------------------
def compute_iou_acc(pred, target, n_cls, verbose=False, ignore_index=-1, device=None):
    """(m_acc, a_acc, m_iou) as 0-dim CPU float32 tensors (reference lines 9-52): one histogram kernel
    instead of 2*n_cls Python iterations.  Like the reference it overwrites ``pred`` with the ignore
    label at ignored pixels in place (line 20)."""
    pred[target == ignore_index] = ignore_index
    inter, pc, tc = N.class_counts(pred.contiguous(), target.contiguous(), n_cls, per_image=False, mask_pred=False)
    inter, pc, tc = inter.float(), pc.float(), tc.float()
    union = tc + pc - inter
    ind = tc > 0
    m_acc = (inter[ind] / tc[ind]).mean().cpu()
    a_acc = (inter.sum() / tc.sum()).cpu()
    ind = union > 0
    m_iou = (inter[ind] / union[ind]).mean().cpu()
    if verbose:
        print(f"mAcc={m_acc:.2%} aAcc={a_acc:.2%}", f" mIoU={m_iou:.2%}")
    return m_acc, a_acc, m_iou


def check_oscillation(x, j, k, y5, k3=0.75):
    """Reference lines 243-248 (kept for API parity; the attack itself does this inside K7)."""
    t = torch.zeros(x.shape[1], device=x.device)
    for counter5 in range(k):
        t += (x[j - counter5] > x[j - counter5 - 1]).float()
    return (t <= k * k3 * torch.ones_like(t)).float()


def apgd_checkpoints(n_iter: int):
    """{iteration: window k} of the step-size checks; data independent (reference lines 323-329, 528-551)."""
    k = max(int(0.22 * n_iter), 1)
    k_min = max(int(0.06 * n_iter), 1)
    dec = max(int(0.03 * n_iter), 1)
    out, c3 = {}, 0
    for i in range(n_iter):
        c3 += 1
        if c3 == k:
            out[i] = k
            c3 = 0
            k = max(k - dec, k_min)
    return out


# ---------------------------------------------------------------------------------------------------
# device-resident state
# ---------------------------------------------------------------------------------------------------
class ApgdState:
    """All per-image bookkeeping of one apgd_train call, resident in HBM."""

    def __init__(self, B: int, n_iter: int, eps: float, device):
        f32 = dict(dtype=torch.float32, device=device)
        self.B = B
        self.acc_cnt = torch.zeros(B, dtype=torch.int32, device=device)
        self.acc = torch.zeros(B, **f32)
        self.loss_best = torch.zeros(B, **f32)
        self.loss_best_last = torch.zeros(B, **f32)
        self.reduced_last = torch.ones(B, **f32)
        self.step = torch.full((B,), 2.0 * eps, **f32)  # alpha * eps, alpha = 2 (reference lines 329, 339)
        self.loss_steps = torch.zeros(max(n_iter, 1), B, **f32)
        self.flags = torch.zeros(3, B, dtype=torch.uint8, device=device)
        self.done = torch.zeros(1, dtype=torch.int32, device=device)


def compact_labels(y: torch.Tensor, n_cls: int) -> torch.Tensor:
    """int64 labels -> uint8 (255 = ignore) or int16: the labels are read every iteration but never change,
    so the 8-byte reads of the reference become 1-2 bytes per pixel."""
    if y.dtype in (torch.uint8, torch.int16):
        return y.contiguous()
    if n_cls <= 255:
        return torch.where(y < 0, torch.full_like(y, 255), y).to(torch.uint8).contiguous()
    return y.to(torch.int16).contiguous()


class _FrozenParameters:
    """The attack differentiates w.r.t. the input only (reference line 367: ``torch.autograd.grad(loss, [x])``),
    so the forward runs with the parameters frozen: autograd keeps no weight-gradient edges and the model's
    frozen-weight kernels (Winograd-domain filter cache) apply.  ``requires_grad`` flags are restored on exit."""

    def __init__(self, model):
        plain = isinstance(model, torch.nn.Module) and not isinstance(model, torch.nn.parallel.DistributedDataParallel)
        self.params = [p for p in model.parameters() if p.requires_grad] if plain else []  # DDP tracks its own flags

    def __enter__(self):
        for p in self.params:
            p.requires_grad_(False)

    def __exit__(self, *exc):
        for p in self.params:
            p.requires_grad_(True)
        return False


def _forward_logits(model, x_buf, want_grad: bool, lowres: bool = False):
    """Model forward on a leaf alias of the iterate buffer.  With ``lowres`` the model's
    ``forward_lowres`` hook is used: it returns the logits BEFORE the final bilinear upsample, which the
    fused kernel K2u then interpolates on the fly."""
    x_in = x_buf.detach()
    fn = model.forward_lowres if lowres else model
    if want_grad:
        x_in.requires_grad_(True)
        with torch.enable_grad(), _FrozenParameters(model):
            logits = fn(x_in)
    else:
        with torch.no_grad(), _FrozenParameters(model):
            logits = fn(x_in)
    if lowres:
        logits = logits[0]
    return x_in, logits


def _input_grad(logits, x_in, dlogits):
    (g,) = torch.autograd.grad(logits, [x_in], grad_outputs=dlogits)
    return g if g.is_contiguous() else g.contiguous()


# K2u (loss fused with the model's final bilinear upsample; needs `model.forward_lowres`).  It never materialises the
# full-resolution logits and their gradient (2.5 GB at B=8, C=151, 512^2).  Since round 6 the x4 / x16 ratios of the BASELINE
# models run a kernel with lanes = classes (csrc/loss_upsampled.hip, "power-of-two ratios") that is FASTER than up-sample + K2 +
# up-sample-backward from two class slots on (C = 151: 629 vs 982 us at x4, 663 vs 906 us at x16, profiles/r6_k2u_bench.log),
# and slower below (C = 21: 305 vs 140 us -- a third of the lanes idle).  Default "auto": fuse where that kernel applies and
# C >= FUSE_UPSAMPLE_MIN_CLASSES, or when the materialised tensors would exceed FUSE_UPSAMPLE_AUTO_BYTES (the general gather
# kernel as a memory-saving mode); SEA_FUSE_UPSAMPLE=1 / 0 (or fuse_upsample=True / False) force / forbid it.
_fu = os.environ.get("SEA_FUSE_UPSAMPLE", "auto")
FUSE_UPSAMPLE = "auto" if _fu == "auto" else (_fu == "1")
FUSE_UPSAMPLE_AUTO_BYTES = 24 * 2 ** 30
FUSE_UPSAMPLE_MIN_CLASSES = 96
# A/B switch (env SEA_K2U_POW2=0): K2u's general gather kernel at the factors 4 and 16 too (the one place it is read)
K2U_POW2 = os.environ.get("SEA_K2U_POW2", "1")[:1] != "0"

# HIP-graph replay of the middle iterations of an APGD run (see ApgdRun._capture).  SEA_HIP_GRAPH=0 executes every one.
USE_HIP_GRAPH = os.environ.get("SEA_HIP_GRAPH", "1") != "0"
GRAPH_MIN_ITER = 12


_CAPTURE_STREAMS = {}


def _capture_stream(device):
    """ONE side stream per device for every run's graph captures.  PyTorch keeps a BLAS workspace per (handle, stream) for
    the life of the process (tens to hundreds of MB each); a fresh torch.cuda.Stream() per run -- three per attack and batch --
    left one such set behind per pooled stream handle (measured: 150-200 MB per run still allocated after an evaluation).
    Runs are sequential, and each orders itself against the caller's stream with wait_stream both ways."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    st = _CAPTURE_STREAMS.get(key)
    if st is None:
        st = _CAPTURE_STREAMS[key] = torch.cuda.Stream(device=device)
    return st



# ---- one owner for a run's device buffers and its captured graph pair -------------------------------------------------------
# SEA runs nine apgd_train calls per batch (three losses x three stages, reference attacker.py:691-728 and
# tools/infer.py:338-370).  Nothing distinguishes them for the captured graphs except the radius, the run length (with its
# checkpoint table) and the contents of the buffers: all of that is DEVICE STATE here (the replayable K1 / K7, which every
# iteration runs, read eps, n_iter and the loop index from memory and update the iterate in place in `x_adv` / `x_old`) and
# the loss is chosen by the eager K2 launch between the two graphs.  So every run works in the buffers of exactly ONE owner
# (`_RunBuffers`), which also holds the pair that addresses them: the caller's tensors are copied in and never written, the
# results are copied out.  An owner cached on the model (`_graph_slot`) outlives its run: the pair is captured ONCE per (model
# weights, batch shape, classes, K2 or K2u) and replayed by every stage, loss and batch of equal shape; round 4 captured nine
# pairs per batch (3.7 % of the protocol's wall time).
# A run that gets no cached owner (eager loop, SEA_GRAPH_CACHE=0, a nested run, weights that moved between two runs, L2)
# constructs a private one sized for its own length, starts without a pair and frees pair and activation pool on release.
GRAPH_CACHE = os.environ.get("SEA_GRAPH_CACHE", "1") != "0"
GRAPH_SLOT_MIN_ITERS = 128      # capacity (iterations) of a cached owner's checkpoint table and loss history
_GRAPH_SLOTS = weakref.WeakKeyDictionary()   # model -> {shape key: _RunBuffers}; dies with the model


class _RunBuffers:
    """Every device buffer of one APGD run, at a fixed address for the lifetime of a captured graph pair, the pair itself,
    and the run-specific scalars (radius, run length, checkpoint table, loop index) as device words."""

    def __init__(self, x, num_classes, cap_iter, weights_key=None):
        dev, B = x.device, x.shape[0]
        self.weights_key, self.cap_iter = weights_key, cap_iter
        new = lambda: torch.empty_like(x, memory_format=torch.contiguous_format)  # noqa: E731
        self.x, self.x_adv, self.x_old, self.grad = new(), new(), new(), new()
        self.x_best, self.x_best_adv, self.grad_best = new(), new(), new()
        pred_dtype = torch.uint8 if num_classes <= 255 else torch.int16
        self.pred = torch.empty(B, x.shape[-2], x.shape[-1], dtype=pred_dtype, device=dev)
        self.pred_best = torch.empty_like(self.pred)
        self.stats = (torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev),
                      torch.empty(B, dtype=torch.int32, device=dev))
        self.ws = N.loss_workspace(B, x.shape[-2] * x.shape[-1], dev)
        self.ws_low = None          # K2u's workspace (sized by the low-resolution logits of the first fused launch)
        self.n_ignored = torch.empty(B, dtype=torch.int32, device=dev)
        self.st = ApgdState(B, cap_iter, 0.0, dev)
        self.it_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.cp_dev = torch.zeros(cap_iter, dtype=torch.int32, device=dev)
        self.eps_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        self.niter_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.dlogits = None         # K2's / K2u's gradient buffer (allocated by the first launch, see keep_k2_grad)
        self.graphs = None          # (graph A, graph B) once captured
        self.sig = None             # what else the captured pair bakes in (early_stop, deferred K2 sums, arithmetic)
        self.g_xin = self.g_logits = self.ws_pin = None
        self.busy = False           # a run is using the owner (runs are sequential; a nested one gets a private owner)

    def reset(self, eps, n_iter, cps):
        """the state of a fresh run (reference attacker.py:310-339), written in place"""
        st = self.st
        for t in (st.acc_cnt, st.acc, st.loss_best, st.loss_best_last, st.loss_steps, st.flags, st.done):
            t.zero_()
        st.reduced_last.fill_(1.0)
        st.step.fill_(2.0 * eps)
        tab = torch.zeros(self.cap_iter, dtype=torch.int32)
        for k, v in cps.items():
            tab[k] = v
        self.cp_dev.copy_(tab)
        self.it_dev.zero_()         # from here on the loop index is device state only: K1 reads it, K7 advances it
        self.eps_dev.fill_(eps)
        self.niter_dev.fill_(max(n_iter, 1))

    def k2u_workspace(self, low):
        if self.ws_low is None:
            self.ws_low = torch.empty(N.lib().sea_loss_upsampled_workspace_bytes(
                low.shape[0], low.shape[1], low.shape[2], low.shape[3], self.x.shape[-2], self.x.shape[-1], int(K2U_POW2)),
                dtype=torch.uint8, device=low.device)
        return self.ws_low

    def keep_k2_grad(self, dlogits):
        """the kernel wrapper allocates the gradient buffer on the first launch (in the logits' memory format); every later
        launch of this owner writes the same one, and graph B reads it"""
        self.dlogits = dlogits

    def keep_graphs(self, graphs, sig, g_xin, g_logits):
        self.graphs, self.sig, self.g_xin, self.g_logits = graphs, sig, g_xin, g_logits
        # the graphs bake in the address of the split-K workspace the model's GEMMs used: keep it alive while they may replay
        self.ws_pin = N.ksplit_workspace_pin(self.x.device)

    def drop_graphs(self):
        """the pair and the activations its private pool keeps alive (several GB at B=8, 512x512)"""
        self.graphs = self.sig = None
        self.g_xin = self.g_logits = self.ws_pin = None


def _weights_key(model):
    """identity, address and in-place version of every parameter and buffer: a captured graph is valid for exactly these"""
    return hash(tuple((id(t), t.data_ptr(), t._version) for t in list(model.parameters()) + list(model.buffers())))


def _arith_signature(model):
    """Everything process-global that a captured forward / backward bakes in besides addresses and weights: the arithmetic
    and kernel switches of the model modules and of the kernel bindings (every UPPER-CASE scalar global of semseg.models.* and
    semseg._native: GEMM_TERMS, GEMM_TERMS_BWD, WINOGRAD_TILE, WINOGRAD_MIN_PIXELS, USE_*, FUSE_MLP, WINO_SPLIT_MIN_TILES ...;
    GEMM_PIPE, GEMM_MFMA_SHAPE, DWCONV_AB ...; the in-process override of the GEMM terms), the attention arithmetic (read per
    call from the environment), this module's K2U_POW2, the autocast state and ``model.training``.  The library itself keeps no
    switch: which kernel runs is an argument of every call.  A cached pair whose signature differs is captured again instead
    of replaying the old arithmetic."""
    import sys
    sig = [bool(getattr(model, "training", False)), torch.is_autocast_enabled(),
           str(torch.get_autocast_dtype("cuda")) if torch.is_autocast_enabled() else None,
           N.attn_terms_fwd(), N.attn_terms_bwd(), K2U_POW2]
    for name in sorted(sys.modules):
        if name.startswith("semseg.models.") or name == N.__name__:
            mod = sys.modules[name]
            sig.append((name, tuple((k, v) for k, v in sorted(vars(mod).items())
                                    if k.isupper() and isinstance(v, (bool, int, float, str)))))
            if hasattr(mod, "_TERMS_OVERRIDE"):
                sig.append(tuple(mod._TERMS_OVERRIDE))
    return tuple(sig)


class _Volatile:
    """Marker in a model's slot table: the weights behind this shape changed between two runs (a training loop such as
    tools/train_rob_seg.py with ATTACK=apgd, whose every outer step moves the parameters' versions).  Such a run gets NO
    cached owner -- it captures its own pair and frees it with its activation pool on return, as before round 5 -- and one
    is attached again only once two consecutive runs saw the same weights."""

    def __init__(self, weights_key):
        self.weights_key = weights_key


GRAPH_SLOTS_PER_MODEL = 2       # shapes kept per model (an evaluation has at most a full and a ragged last batch)


def _graph_slot(model, x, num_classes, n_iter, fused):
    """the model's cached owner for this shape and loss kernel, or None: the run then constructs a private one"""
    if not (GRAPH_CACHE and isinstance(model, torch.nn.Module)):
        return None
    try:
        slots = _GRAPH_SLOTS.setdefault(model, {})
    except TypeError:
        return None
    # `fused`: K2u's gradient buffer is low-resolution, K2's is not, and the pair replays one of the two forwards
    key = (tuple(x.shape), x.dtype, x.device.index, num_classes, fused)
    wkey = _weights_key(model)
    own = slots.pop(key, None)              # (re-inserted below: the dict keeps the most recently used shape last)
    if isinstance(own, _Volatile):
        if own.weights_key != wkey:         # still moving: no cached owner, no several GB parked on the model
            own.weights_key = wkey
            slots[key] = own
            return None
        own = None                          # the weights held still for two runs: cache again
    elif own is not None and own.weights_key != wkey:
        # other weights (a training step, a loaded checkpoint): free the stale pair and its pool BEFORE anything new is
        # allocated, and let this run capture for itself
        own.drop_graphs()
        slots[key] = _Volatile(wkey)
        return None
    elif own is not None and own.busy:
        slots[key] = own
        return None                         # a nested run gets its own buffers
    elif own is not None and own.cap_iter < n_iter:
        own.drop_graphs()                   # a longer run than the tables were sized for: start over
        own = None
    if own is None:
        live = [k for k, v in slots.items() if isinstance(v, _RunBuffers)]
        while len(live) >= GRAPH_SLOTS_PER_MODEL:           # least recently used shape first
            old = slots.pop(live.pop(0))
            if old.busy:                                    # (its run is still going: leave it alone, take none)
                slots[key] = _Volatile(wkey)
                return None
            old.drop_graphs()
        own = _RunBuffers(x, num_classes, max(GRAPH_SLOT_MIN_ITERS, n_iter), wkey)
    slots[key] = own
    return own


def release_graph_cache(model=None):
    """drop the cached graph pairs (and the several GB of activations their pools hold) of ``model``, or of every model"""
    for m in ([model] if model is not None else list(_GRAPH_SLOTS.keys())):
        for slot in _GRAPH_SLOTS.pop(m, {}).values():
            if isinstance(slot, _RunBuffers):
                slot.drop_graphs()


def _owned(name):
    return property(lambda self: getattr(self.own, name))


class ApgdRun:
    """One APGD run as an object: ``start()`` is step 0 (reference lines 342-383), ``step(i)`` is loop
    iteration i (lines 385-569).  ``apgd_train`` drives it; bench.py times ``step`` directly.
    Nothing in ``step`` synchronises with the host.

    Every device buffer and all graph state belong to ``self.own``, the run's one ``_RunBuffers``: the model's cached one
    when the run is eligible (graph mode, contiguous input, weights that held still, not in use), else a private one.  ``x``
    and ``x_start`` are copied in and never written; ``result()`` hands out copies.  ``release_graphs()`` ends the run: a
    cached owner keeps its pair for the next run, a private one drops it; the buffers stay readable either way."""

    x, grad, pred, pred_best, st, ws, n_ignored, graphs = (_owned(k) for k in (
        "x", "grad", "pred", "pred_best", "st", "ws", "n_ignored", "graphs"))

    def __init__(self, model, x, y, eps, n_iter, loss, track_loss, early_stop, num_classes, weights, x_start,
                 fuse_upsample=None, norm="Linf"):
        self.model = model
        self.norm = norm               # "Linf" (K1) or "L2" (K1': four streaming passes, reference lines 412-436)
        self._l2_ws = self._l2_next = None
        # fuse the model's final bilinear upsample into the loss kernel when the model offers the hook
        if fuse_upsample is None:
            fuse_upsample = FUSE_UPSAMPLE
        if fuse_upsample and hasattr(model, "forward_lowres"):
            with torch.no_grad():
                probe = model.forward_lowres(x[:1])
            if probe is None:
                fuse_upsample = False
            elif fuse_upsample == "auto":
                full = 2 * 4 * x.shape[0] * probe[0].shape[1] * x.shape[-2] * x.shape[-1]  # logits + gradient, fp32
                lo = probe[0]
                pow2 = any(x.shape[-2] == r * lo.shape[-2] and x.shape[-1] == r * lo.shape[-1] for r in (4, 16))
                fast = (pow2 and FUSE_UPSAMPLE_MIN_CLASSES <= lo.shape[1] <= 192 and lo.dtype == torch.float32
                        and min(lo.shape[-2:]) >= 2 and K2U_POW2)
                fuse_upsample = fast or full > FUSE_UPSAMPLE_AUTO_BYTES
        else:
            fuse_upsample = False
        self.fused = bool(fuse_upsample)
        self.mode = N.MODE_BY_NAME[loss]
        self.tmode = N.MODE_BY_NAME[track_loss] if track_loss is not None else self.mode
        self.eps, self.n_iter, self.early_stop, self.num_classes = float(eps), n_iter, early_stop, num_classes
        self.y = y
        self.B, self.HW = x.shape[0], x.shape[-2] * x.shape[-1]
        self.yc = compact_labels(y, num_classes)
        self.w = None
        if weights is not None and (self.mode == 1 or self.tmode == 1):
            self.w = weights.to(device=x.device, dtype=torch.float32).contiguous()
        self.cps = apgd_checkpoints(n_iter)
        self.gscale = 1.0 / float(self.HW)
        self.defer = True      # K7 sums K2's per-block records itself (no finalize launch); off when verbose
        self.last = None       # K2 outputs of the latest iterate
        self.k2_events = None  # optional list of (start, end) event pairs, one per step (bench.py)
        # (capture costs ~3 eager iterations; the L2 step -- on no shipped entry point, SURVEY fact 2 -- keeps the eager loop)
        self.use_graph = USE_HIP_GRAPH and n_iter >= GRAPH_MIN_ITER and n_iter > 3 and norm == "Linf"
        self._gs = _capture_stream(x.device)
        self._caller_stream = None
        own = _graph_slot(model, x, num_classes, n_iter, self.fused) if (self.use_graph and x.is_contiguous()) else None
        self._private = own is None
        self.own = own = _RunBuffers(x, num_classes, max(n_iter, 1)) if own is None else own
        # a run that finds the pair already captured replays it from iteration 0
        self._first_graph_step = 0 if own.graphs is not None else 2
        self.x_adv, self.x_old = own.x_adv, own.x_old
        own.x.copy_(x)
        self.x_adv.copy_(x_start)
        N.count_ignored(self.yc, out=own.n_ignored)
        own.reset(self.eps, n_iter, self.cps)
        own.busy = True        # last: a constructor that raises leaves a cached owner free for the next run

    def _loss(self, logits, want_grad):
        o = self.own
        ev = None
        if self.k2_events is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        if self.fused:
            r = N.loss_fwd_bwd_upsampled(logits.detach().contiguous(), self.yc, self.w, self.mode, self.tmode,
                                         self.gscale, want_grad=want_grad, pred=o.pred, workspace=o.k2u_workspace(logits),
                                         out=o.stats, dlow=o.dlogits if want_grad else None, pow2=K2U_POW2)
        else:
            r = N.loss_fwd_bwd(logits.detach(), self.yc, self.w, self.mode, self.tmode, self.gscale,
                               want_grad=want_grad, pred=o.pred, workspace=o.ws, out=o.stats,
                               dlogits=o.dlogits if want_grad else None, defer=self.defer)
        if ev is not None:
            ev[1].record()
            self.k2_events.append(ev)
        if want_grad:
            o.keep_k2_grad(r["dlogits"])
        self.last = r
        return r

    def _select(self):
        o = self.own
        N.select_copy(o.st.flags, self.x_adv, o.grad, o.x_best, o.grad_best, o.x_best_adv, o.pred, o.pred_best)

    def start(self):
        o = self.own
        x_in, logits = _forward_logits(self.model, self.x_adv, True, self.fused)
        r = self._loss(logits, True)
        g = _input_grad(logits, x_in, r["dlogits"])
        del logits
        N.apgd_track(r, o.n_ignored, self.HW, 0, max(self.n_iter, 1), 0, False, True, o.st)
        o.grad.copy_(g)
        o.grad_best.copy_(g)
        o.pred_best.copy_(o.pred)
        for t in (o.x_best, o.x_best_adv, self.x_old):
            t.copy_(self.x_adv)

    def step(self, i: int):
        if self.use_graph:
            if self._first_graph_step <= i < self.n_iter - 1:
                return self._step_graph(i)
            if i == 1:
                # eager, but on the stream the graphs will be captured on: per-stream library state (MIOpen / hipBLASLt
                # handles and workspaces) must exist before a capture starts
                cur = torch.cuda.current_stream()
                self._gs.wait_stream(cur)
                with torch.cuda.stream(self._gs):
                    self._step_eager(i)
                cur.wait_stream(self._gs)
                return
        self._step_eager(i)

    # ---- one iteration = front, _loss, back: each written once, executed (eager) or recorded and replayed (HIP-graph mode) ----
    def _front(self, i: int, want_grad: bool, k1: bool = True):
        """gradient step (reference lines 389-456), in place, and the model forward on the new iterate"""
        o = self.own
        if k1 and self.norm == "Linf":
            N.apgd_linf_step_graph(o.x, self.x_adv, self.x_old, o.grad, o.st.step, o.eps_dev, o.it_dev)
        elif k1:
            self._l2_step(i)
        return _forward_logits(self.model, self.x_adv, want_grad, self.fused)

    def _back(self, x_in, logits, r, want_grad: bool = True):
        """model input-gradient, then the bookkeeping on the device (K7 decisions, K4 copies)"""
        o = self.own
        if want_grad:
            o.grad.copy_(_input_grad(logits, x_in, r["dlogits"]))   # the gradient buffer keeps its address (K1 / K4 read it)
        N.apgd_track_graph(r, o.n_ignored, self.HW, o.it_dev, o.cp_dev, o.niter_dev, self.early_stop, o.st)
        self._select()

    def _step_eager(self, i: int, k1: bool = True):
        want = i < self.n_iter - 1  # the reference skips the last backward (line 467)
        x_in, logits = self._front(i, want, k1)
        self._back(x_in, logits, self._loss(logits, want), want)

    def _l2_step(self, i: int):
        """K1' re-reads x_adv and x_old in four passes: it writes a third buffer and the three rotate (L2 never captures)"""
        o = self.own
        if self._l2_ws is None:
            self._l2_ws = torch.empty(N.lib().sea_apgd_l2_workspace_bytes(self.B) // 8, dtype=torch.float64, device=o.x.device)
            self._l2_next = torch.empty_like(o.x)
        N.apgd_l2_step(o.x, self.x_adv, self.x_old, o.grad, o.st.step, self.eps, 0.75 if i > 0 else 1.0, out=self._l2_next,
                       workspace=self._l2_ws)
        self.x_old, self.x_adv, self._l2_next = self.x_adv, self._l2_next, self.x_old

    # ---- HIP-graph mode ----------------------------------------------------------------------------------------
    # An iteration is ~360 kernel launches that the host needs 9-14 ms to enqueue (ConvNeXt-T, B=8) for 22 ms of GPU
    # work: hidden on one GPU, not with 8 ranks on one host or a faster model side.  With `use_graph` the middle
    # iterations (_first_graph_step <= i < n_iter - 1) replay the two recorded pieces around the one eager K2 launch:
    #     graph A = front (K1 in place + model forward)
    #     K2      = _loss, eager (so a caller can still bracket it with events; bench.py does)
    #     graph B = back (input-gradient backward + K7 + K4)
    # A run that has to capture executes iterations 0 and 1 first (library warm-up, iteration 1 on the capture stream); the
    # last iteration is always executed (no backward there).  Same calls, same kernels, same order in both modes: the
    # outputs are bitwise those of the eager loop (tested).
    def _graph_failed(self, exc):
        """A model whose forward / backward cannot be captured (a host sync such as .item(), a library that allocates or
        JIT-compiles on first use of a shape, ...) keeps working: the run continues with the eager loop, which is the same
        kernels in the same order.  Reported once per run on stderr."""
        import sys
        self.use_graph = False
        self.own.drop_graphs()
        # torch.cuda.graph.__exit__ does not leave its stream context when capture_end() itself raises (an invalidated
        # capture): put the caller's stream back
        torch.cuda.set_stream(self._caller_stream)
        print(f"[sea] HIP-graph capture of the attack step failed ({type(exc).__name__}: {str(exc).splitlines()[0][:160]}); "
              "continuing with the eager loop", file=sys.stderr)
        torch.cuda.synchronize()

    def _capture(self, i: int):
        """records front and back AND performs iteration i by replaying them; falls back to the eager loop when a capture fails"""
        o = self.own
        self._caller_stream = torch.cuda.current_stream()
        ga, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(ga, stream=self._gs):
                g_xin, g_logits = self._front(i, True)
        except Exception as exc:   # nothing of iteration i has run yet (a capture executes nothing)
            self._graph_failed(exc)
            return self._step_eager(i)
        ga.replay()
        r = self._loss(g_logits, True)                # eager, and it defines the (persistent) K2 output buffers
        try:
            with torch.cuda.graph(gb, pool=ga.pool(), stream=self._gs):
                self._back(g_xin, g_logits, r)
        except Exception as exc:   # K1 of iteration i is done (graph A replayed, in place): finish the iteration eagerly.
            # The failed capture has consumed the autograd graph of graph A's forward, so the forward is run again, on the
            # updated iterate (same kernels, same bits)
            self._graph_failed(exc)
            del g_xin, g_logits
            return self._step_eager(i, k1=False)
        gb.replay()
        o.keep_graphs((ga, gb), self._graph_sig(), g_xin, g_logits)

    def _graph_sig(self):
        """what a captured pair bakes in besides addresses and weights: K7's early-stop flag, where it finds K2's sums, and
        the process-global arithmetic state of the model's forward / backward (``_arith_signature``)"""
        return (bool(self.early_stop), bool(self.defer), _arith_signature(self.model))

    def _step_graph(self, i: int):
        o = self.own
        if o.graphs is not None and i == self._first_graph_step and o.sig != self._graph_sig():
            o.drop_graphs()                               # (a verbose run after a silent one: capture again)
        if o.graphs is None:
            self._capture(i)                              # captures AND performs iteration i
            return
        o.graphs[0].replay()
        self._loss(o.g_logits, True)
        o.graphs[1].replay()

    def release_graphs(self):
        """the run is over.  A private owner drops its captured graphs and the activations their pool keeps alive (several GB
        at B=8, 512x512; an evaluation creates three runs per batch and attack); a cached one keeps them for the next run and
        is free again.  The buffers stay readable."""
        if self._private:
            self.own.drop_graphs()
        self.own.busy = False

    def result(self):
        """copies: the buffers belong to the owner, and a cached owner to the next run"""
        o = self.own
        return o.x_best.clone(), o.st.acc.clone(), o.st.loss_best.clone(), o.x_best_adv.clone()


def apgd_train(model, x, y, norm, eps, n_iter=10, use_rs=False, loss="ce", verbose=False, is_train=False,
               early_stop=False, track_loss=None, logger=None, y_target=None, ignore_index=-1, x_init=None,
               num_classes=21, weights=None, gpuu=None, noise=None, poll_every: int = 8, return_pred: bool = False):
    """One APGD run (reference lines 260-571).  Returns ``(x_best, acc, loss_best, x_best_adv)``.

    Extra keyword arguments (all optional): ``gpuu`` is accepted and ignored (tools/train_rob_seg.py
    passes it); ``noise`` replaces ``torch.rand_like(x)`` of the random start so CPU and
    device runs can share it; ``poll_every`` = how often the host looks at the early-stop flag;
    ``return_pred`` appends the argmax map of ``x_best_adv`` (uint8 / int16, produced by the attack's own fused
    kernel on the forward that evaluated that iterate) to the returned tuple.
    """
    assert not model.training
    assert ignore_index == -1, "Only `ignore_index = 1` is supported."
    if norm == "L1":
        raise NotImplementedError("the L1 branch of apgd_train (reference semseg/attacker.py:437-454, 553-566: sparse steps, "
                                  "L1_projection, adaptive sparsity) is not built: no entry point of the reference reaches it "
                                  "(SURVEY fact 2; tools/infer.py and tools/train_rob_seg.py pass norm='Linf')")
    if norm not in ("Linf", "L2"):
        raise ValueError(f"norm {norm!r}: 'Linf' or 'L2'")
    if norm == "L2" and use_rs and x_init is None:
        # reference lines 288-297: the random start exists for L-inf only; there x_adv would be undefined (NameError)
        raise ValueError("apgd_train(norm='L2', use_rs=True) needs x_init: the reference draws a random start for L-inf only")
    if loss not in N.MODE_BY_NAME:
        raise KeyError(loss)
    if not x.is_cuda:
        raise N.SeaNativeError("apgd_train needs HIP device tensors (no CPU fallback)")
    device = x.device
    x = x.detach().contiguous().float()

    # ---- start point (reference lines 288-308); the RNG is consumed even when x_init overrides it
    if not use_rs or norm != "Linf":
        x_adv = x.clone()
    else:
        t = torch.rand_like(x) if noise is None else noise.to(device)
        x_adv = N.linf_random_start(x, t.contiguous(), float(eps))
    if x_init is not None:
        x_adv = x_init.detach().clone().contiguous().float()
    x_adv = x_adv.clamp_(0.0, 1.0)

    run = None
    try:
        run = ApgdRun(model, x, y, eps, n_iter, loss, track_loss, early_stop, num_classes, weights, x_adv, norm=norm)
        run.defer = not verbose  # the verbose log line reads the per-image sums on the host
        if logger is not None:
            # reference lines 302-306 log this whenever ignore labels exist (one host read per run, outside the loop)
            n_ign = int(run.n_ignored.sum())
            if n_ign > 0:
                logger.log(f"{n_ign / y.numel():.2%} pixels are masked out.")
        return _apgd_drive(run, y, n_iter, verbose, logger, early_stop, poll_every, num_classes, return_pred)
    finally:
        if run is not None:
            run.release_graphs()        # (also when the logging or a step raises: a cached owner must not stay busy)


def _apgd_drive(run, y, n_iter, verbose, logger, early_stop, poll_every, num_classes, return_pred):
    """the loop of ``apgd_train`` (reference lines 342-569) over a constructed run"""
    run.start()
    if verbose:
        m_acc, a_acc, m_iou = compute_iou_acc(run.pred_best.long(), y, num_classes)

    done_host = torch.zeros(1, dtype=torch.int32).pin_memory() if early_stop else None
    done_evt = None
    for i in range(n_iter):
        run.step(i)
        if verbose:
            st, r = run.st, run.last
            m_acc, a_acc, m_iou = compute_iou_acc(run.pred_best.long(), y, num_classes)
            if logger is not None:
                logger.log("iteration: {} - best loss: {:.6f} curr loss {:.6f} - mAcc={:.2%} aAcc={:.2%} "
                           "mIoU={:.2%} - step size: {:.5f}".format(
                               i, st.loss_best.sum().item(), (r["track_sum"].sum() / run.HW).item() / run.B, m_acc,
                               a_acc, m_iou, st.step.mean().item()))
        # ---- early stop (reference lines 568-569): the flag lives on the device and freezes all state
        # from the next iteration on, so looking at it late never changes the result.
        if early_stop:
            if done_evt is not None and done_evt.query():
                if int(done_host[0]) != 0:
                    break
                done_evt = None
            if done_evt is None and (i % poll_every) == poll_every - 1:
                done_host.copy_(run.st.done, non_blocking=True)
                done_evt = torch.cuda.Event()
                done_evt.record()
    out = run.result()
    if return_pred:
        out = out + (run.pred_best.clone(),)
    return out


def apgd_restarts(model, x, y, norm="Linf", eps=8.0 / 255.0, n_iter=10, loss="ce", verbose=False, n_restarts=1,
                  log_path=None, early_stop=False, eot_iter=0, track_loss=None, use_rs=False, ignore_index=-1,
                  noises=None):
    """APGD with restarts on the still-robust images (reference lines 574-659).  Not used by SEA
    (tools/infer.py uses apgd_largereps); kept for API parity.  Targeted losses are not implemented.
    Returns ``(x_adv, acc_of_last_run, acc)`` like the reference's ``(x_adv, _, acc)``.  ``noises[r]``
    (optional) replaces the uniform draw of restart r's random start (shape of the active sub-batch).

    The candidate's pixel accuracy (reference lines 631-634: a re-forward, ignored pixels counted as
    correct) comes from one no-gradient K2 launch on the re-forwarded logits."""
    if "targeted" in loss:
        raise NotImplementedError("targeted losses are outside the SEA hot path")
    logger = Logger(log_path)
    B, HW = x.shape[0], x.shape[-2] * x.shape[-1]
    acc = torch.ones(B, device=x.device)
    x_adv = x.clone()
    acc_last_run = None
    for r in range(n_restarts):
        rows = torch.nonzero(acc > 0).flatten()            # images that are still robust
        if rows.numel() == 0:
            continue
        xs, ys = x[rows], y[rows]
        _, acc_last_run, _, cand = apgd_train(model, xs, ys, n_iter=n_iter, use_rs=use_rs, verbose=verbose, loss=loss,
                                              eps=eps, norm=norm, logger=logger, early_stop=early_stop,
                                              track_loss=track_loss, y_target=None, ignore_index=ignore_index,
                                              noise=None if noises is None else noises[r])
        _, logits = _forward_logits(model, cand, False)
        yc = compact_labels(ys, logits.shape[1])
        st = N.loss_fwd_bwd(logits, yc, None, 3, 3, 0.0, want_grad=False)
        n_ign = N.count_ignored(yc)
        acc_cand = (st["n_correct"] + n_ign).float() / float(HW)
        better = acc_cand < acc[rows]
        x_adv[rows[better]] = cand[better]
        acc[rows[better]] = acc_cand[better]
        note = " (warning: this is only upper bound on aAcc)" if bool((n_ign > 0).any()) else ""
        logger.log(f"restart {r + 1} robust accuracy={acc.float().mean():.1%}{note}")
    return x_adv, acc_last_run, acc


def largereps_schedule(n_iter: int, eps: float):
    """Stage lengths [int(.3n), int(.3n), rest] and radii [2eps, 1.5eps, eps] (reference lines 693-695)."""
    n_iters = [int(c * n_iter) for c in [0.3, 0.3]]
    n_iters.append(n_iter - sum(n_iters))
    return n_iters, [c * eps for c in [2, 1.5, 1]]


def apgd_largereps(model, x, y, weights, norm="Linf", eps=8.0 / 255.0, n_iter=10, loss="ce", verbose=False,
                   n_restarts=1, log_path=None, early_stop=False, eot_iter=0, track_loss=None, use_rs=False,
                   ignore_index=-1, num_classes=21, noises=None, return_pred: bool = False):
    """The SEA attack schedule: three APGD stages at radii 2eps, 1.5eps, eps (reference lines 662-728).
    Returns ``(x_adv, None, acc)`` with x_adv the lowest-pixel-accuracy iterate of the last stage; with
    ``return_pred`` also the argmax map of x_adv (so callers such as tools/infer.py need not re-forward it,
    reference tools/infer.py:136-155 + 356-364)."""
    if norm != "Linf":
        raise NotImplementedError()     # (the reference's stage re-projection, lines 683-690, raises for every other norm)
    logger = Logger(log_path)
    n_iters, epss = largereps_schedule(n_iter, eps)
    acc = torch.ones([x.shape[0]], device=x.device)
    x_init = None
    xc = x.detach().contiguous().float()
    for s, (inner_it, inner_eps) in enumerate(zip(n_iters, epss)):
        if x_init is not None:
            x_init = N.linf_project(x_init.contiguous(), xc, float(inner_eps))  # reference lines 683-690
        _, acc, _, x_init, pred = apgd_train(model, xc, y, n_iter=inner_it, use_rs=use_rs, verbose=verbose, loss=loss,
                                             eps=inner_eps, norm=norm, logger=logger, early_stop=early_stop,
                                             track_loss=track_loss, y_target=None, ignore_index=ignore_index,
                                             x_init=x_init, num_classes=num_classes, weights=weights,
                                             noise=None if noises is None else noises[s], return_pred=True)
    if return_pred:
        return x_init, None, acc, pred
    return x_init, None, acc
