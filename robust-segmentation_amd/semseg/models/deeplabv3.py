"""DeepLabV3-ResNet50 (semseg/models/ddcat_psp.py:33-189 of the reference, on the dilated ResNet-50 of
backbones/resnet_ddcat.py with the deep-base stem): the second architecture of the DDC-AT / AT baselines on PASCAL-VOC.

Same modules, names and state-dict keys as the reference (376 keys, ``aux.*`` included), so a reference checkpoint loads
with ``strict=True``.  The backbone is ``PSPNet(clean=True)``'s, layer for layer (``pspnet._build_backbone`` /
``pspnet._native_backbone``).  Training mode, ``indicate == 1``, bf16 autocast and CPU tensors run the reference's forward
on plain torch ops and return what the reference returns (``(x.max(1)[1], main_loss, aux_loss, x)`` with labels).  The
frozen eval forward of a float32 device batch -- what SEA attacks -- and its input gradient run on the device kernels
("DeepLabV3"):

- the backbone as PSPNet's;
- the three dilated 3x3 branches of the ASPP (rates 6 / 12 / 18) as ONE product and a tap gather: Z = X . W_all^T on the
  un-shifted 2048-channel map through M8 (``_linear_frozen``; W_all = the 27 tap matrices of the three branches with the
  eval BatchNorm scale folded in, rows ordered as P5 reads them), then P5 (csrc/aspp_kernels.hip) sums the nine shifted
  256-channel rows of every branch, adds the BatchNorm shift, applies the ReLU and writes the 1280-channel channels_last
  concatenation in place.  Backward: P5's adjoint gather writes dZ, and one M8 product gives dX = dZ . W_all;
- ``convs[0]`` (1x1): a ``_pointwise`` call (M8 with bias + ReLU in its epilogue), copied into its slice;
- the pooling branch: the adaptive pool of M2'', ``_pointwise``, and P2 (align_corners=True; a 1 x 1 source is a
  broadcast) writing its slice;
- ``cls``: ``_pointwise`` 1280 -> 256, the M10 classifier GEMM (NCHW logits), then P2 (x8, align_corners=True).
Below ``GEMM_MIN_ROWS`` pixels the products fall back to the library as everywhere else; P5 still runs.  Nothing on this
path synchronises with the host, so the attack captures it into its HIP-graph pair.

``USE_NATIVE = False`` runs the plain torch forward (A/B runs, the stock yardstick of the tests)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .convnext_upernet import (_adaptive_pool, _classify, _dense_cl, _folded_bn, _fp32_bwd, _fp32_fwd, _linear_frozen,
                               _stable, _tkey)
from .pspnet import _CL, _UpsampleAC, _build_backbone, _cache, _native_backbone, _pointwise

USE_NATIVE = True


class ASPP(nn.Module):
    """ddcat_psp.py:33-81"""

    def __init__(self, in_channels, out_channels, atrous_rates, BatchNorm):
        super().__init__()
        mods = [nn.Sequential(nn.Conv2d(in_channels, out_channels, 1, bias=False), BatchNorm(out_channels), nn.ReLU())]
        mods += [nn.Sequential(nn.Conv2d(in_channels, out_channels, 3, padding=r, dilation=r, bias=False),
                               BatchNorm(out_channels), nn.ReLU()) for r in atrous_rates]
        mods.append(nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(in_channels, out_channels, 1, bias=False),
                                  BatchNorm(out_channels), nn.ReLU()))
        self.convs = nn.ModuleList(mods)

    def forward(self, x):
        res = [conv(x) for conv in self.convs[:-1]]
        res.append(F.interpolate(self.convs[-1](x), x.shape[2:], mode="bilinear", align_corners=True))
        return torch.cat(res, dim=1)


class DeepLabV3(nn.Module):
    """``DeepLabV3(50, classes=n_cls)`` of the reference (ddcat_psp.py:84-189; the second positional parameter is
    ``atrous_rates``).  ``pretrained`` is accepted and ignored (the reference reads fixed cluster paths there); only
    ``layers=50`` with the ASPP is built (the reference's ``use_aspp=False`` stops at an unbound name)."""

    def __init__(self, layers=50, atrous_rates=(6, 12, 18), dropout=0.1, classes=2, zoom_factor=8, use_aspp=True,
                 criterion=nn.CrossEntropyLoss(ignore_index=255), BatchNorm=nn.BatchNorm2d, pretrained=True):
        super().__init__()
        if layers != 50:
            raise ValueError(f"DeepLabV3: only layers=50 is built here, got {layers}")
        if not use_aspp:
            raise ValueError("DeepLabV3: use_aspp=False is not a model (the reference leaves cls without an input width)")
        assert classes > 1
        assert zoom_factor in [1, 2, 4, 8]
        self.zoom_factor = zoom_factor
        self.use_aspp = use_aspp
        self.criterion = criterion
        _build_backbone(self, BatchNorm, True)
        in_channels, out_channels = 2048, 256
        self.aspp = ASPP(in_channels, out_channels, atrous_rates, BatchNorm)
        fea_dim = out_channels * (len(atrous_rates) + 2)
        self.cls = nn.Sequential(nn.Conv2d(fea_dim, out_channels, kernel_size=1, bias=False), BatchNorm(out_channels),
                                 nn.ReLU(inplace=True), nn.Dropout2d(p=dropout),
                                 nn.Conv2d(out_channels, classes, kernel_size=1))
        if self.training:        # always true here: the reference's key list has aux.*
            self.aux = nn.Sequential(nn.Conv2d(in_channels // 2, out_channels, kernel_size=1, bias=False),
                                     BatchNorm(out_channels), nn.ReLU(inplace=True), nn.Dropout2d(p=dropout),
                                     nn.Conv2d(out_channels, classes, kernel_size=1))

    def _native_ok(self, x, indicate):
        return (USE_NATIVE and not self.training and indicate != 1 and x.is_cuda and x.dtype == torch.float32
                and x.dim() == 4 and not torch.is_autocast_enabled() and not any(p.requires_grad for p in self.parameters()))

    def forward(self, x, y=None, indicate=0):
        x_size = x.size()
        assert (x_size[2] - 1) % 8 == 0 and (x_size[3] - 1) % 8 == 0
        h = int((x_size[2] - 1) / 8 * self.zoom_factor + 1)
        w = int((x_size[3] - 1) / 8 * self.zoom_factor + 1)
        if self._native_ok(x, indicate):
            return _native_forward(self, x, (h, w))

        x = self.layer0(x)
        x = self.layer1(x)
        x = self.layer2(x)
        x_tmp = self.layer3(x)
        x = self.layer4(x_tmp)
        x = self.aspp(x)
        x = self.cls(x)
        if self.zoom_factor != 1:
            x = F.interpolate(x, size=(h, w), mode="bilinear", align_corners=True)
        if self.training or indicate == 1:
            aux = self.aux(x_tmp)
            if self.zoom_factor != 1:
                aux = F.interpolate(aux, size=(h, w), mode="bilinear", align_corners=True)
            main_loss = self.criterion(x, y)
            aux_loss = self.criterion(aux, y)
            return x.max(1)[1], main_loss, aux_loss, x
        return x


# ---------------------------------------------------------------------------------------------------- device path
class _AsppCat(torch.autograd.Function):
    """The ASPP's concatenation as one channels_last buffer, every branch written into its own channel slice:
    [y0 | P5(z) | up_ac(pooled)].  ``y0``: the 1x1 branch, (B, Cb, H, W); ``z``: the un-shifted product (B, H, W, 9 R Cb);
    ``pooled``: the pooling branch at its own (1 x 1) size.  Backward: the slices of the incoming gradient, P5's adjoint
    gather for ``z`` (gated by the saved buffer) and P2's gather for ``pooled``."""

    @staticmethod
    @_fp32_fwd
    def forward(ctx, y0, z, pooled, shift, rates):
        from .. import _native as N
        B, H, W, _ = z.shape
        c0, cz, cp = y0.shape[1], shift.numel(), pooled.shape[1]
        buf = torch.empty(B, H, W, c0 + cz + cp, dtype=torch.float32, device=z.device).permute(0, 3, 1, 2)
        buf[:, :c0].copy_(y0)
        N.aspp_tap_sum(z, rates, shift, out=buf[:, c0:c0 + cz])
        N.upsample_ac_cl(_dense_cl(pooled), (H, W), out=buf[:, c0 + cz:])
        ctx.cols, ctx.rates, ctx.pool_size = (c0, cz, cp), rates, tuple(pooled.shape[2:])
        ctx.save_for_backward(buf)
        return buf

    @staticmethod
    @_fp32_bwd
    def backward(ctx, g):
        from .. import _native as N
        (buf,) = ctx.saved_tensors
        c0, cz, cp = ctx.cols
        if N.cl_pixel_stride(g) is None:
            g = g.contiguous(memory_format=_CL)
        gz = N.aspp_tap_sum_backward(g[:, c0:c0 + cz], buf[:, c0:c0 + cz], ctx.rates)
        gp = N.upsample_ac_cl_backward(g[:, c0 + cz:], ctx.pool_size)
        return g[:, :c0].contiguous(memory_format=_CL), gz, gp, None, None


def _aspp_dilated_ok(branches, x):
    """what P5 and its product cover: R <= 4 frozen 3x3 convolutions of one width with dilation = padding = rate"""
    from .. import _native as N
    convs = [b[0] for b in branches]
    c = convs[0] if convs else None
    return (1 <= len(convs) <= N.ASPP_MAX_BRANCHES and c.out_channels % 4 == 0 and c.in_channels % 32 == 0
            and N.cl_pixel_stride(x) == x.shape[1]
            and all(m.kernel_size == (3, 3) and m.stride == (1, 1) and m.groups == 1 and m.padding_mode == "zeros"
                    and m.dilation[0] >= 1 and m.dilation == (m.dilation[0],) * 2 and m.padding == m.dilation
                    and m.weight.shape == c.weight.shape and m.weight.dtype == torch.float32 for m in convs))


def _aspp_packed(aspp, branches):
    """(W_all, shift) of the dilated branches, cached on the module until a weight or BatchNorm buffer changes.  W_all is
    (R * 9 * Cb, Cin): row (9 r + t) Cb + c = scale_r[c] * weight_r[c, :, ky, kx], t = 3 ky + kx, the column order of P5;
    shift is the R * Cb folded BatchNorm shifts."""
    cache = _cache(aspp)
    folded = [_folded_bn(b[1], b[0].bias, _cache(b[0])) for b in branches]
    key = tuple((_tkey(b[0].weight), _cache(b[0])["bn_key"]) for b in branches)
    if cache.get("taps_key") != key:
        with torch.no_grad():
            rows = [(b[0].weight * scale[:, None, None, None]).permute(2, 3, 0, 1).reshape(-1, b[0].in_channels)
                    for b, (scale, _) in zip(branches, folded)]
            cache.update(taps_key=key, taps_w=_stable(cache.get("taps_w"), torch.cat(rows).contiguous()),
                         taps_shift=_stable(cache.get("taps_shift"), torch.cat([s for _, s in folded]).contiguous()))
    return cache["taps_w"], cache["taps_shift"]


def aspp_forward(aspp, x):
    """``ASPP.forward`` of the frozen module for a dense channels_last float32 device map (module docstring)"""
    convs = aspp.convs
    first, branches, pool = convs[0], list(convs[1:-1]), convs[-1]
    x = _dense_cl(x)
    if not _aspp_dilated_ok(branches, x):
        raise ValueError("DeepLabV3: the ASPP's dilated branches are not the frozen 3x3 / dilation = padding convolutions "
                         "of one width (at most 4) that the device path is built for; set deeplabv3.USE_NATIVE = False")
    w_all, shift = _aspp_packed(aspp, branches)
    z = _linear_frozen(_cache(aspp), x.permute(0, 2, 3, 1), w_all, None)
    y0 = _pointwise(first[0], first[1], x, True)
    pooled = _pointwise(pool[1], pool[2], _adaptive_pool(pool[0], x), True)
    return _AsppCat.apply(y0, z.contiguous(), pooled, shift, tuple(b[0].dilation[0] for b in branches))


def _native_forward(model, x, size):
    x, _ = _native_backbone(model, x)
    x = aspp_forward(model.aspp, x)
    y = _pointwise(model.cls[0], model.cls[1], x, True)
    logits = _classify(model.cls[4], _dense_cl(y))
    if model.zoom_factor == 1:
        return logits
    return _UpsampleAC.apply(logits.contiguous(), size)
