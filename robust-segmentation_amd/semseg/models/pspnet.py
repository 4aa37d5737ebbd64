"""PSPNet-ResNet50 (semseg/models/ddcat_psp.py:372-486 of the reference, with the ResNet-50 of
backbones/resnet_ddcat.py:110-131) in both of the reference's shapes.  ``clean=True`` has the deep-base stem (three 3x3
convolutions): the VOC model of the reference's tools/infer.py (``eval(MODEL.NAME)(50, N_CLS)``,
configs/voc_pspnet_cais.yaml) and the architecture of the DDC-AT / CAIS baselines.  ``clean=False`` has the
torchvision-style stem (one 7x7 stride-2 convolution, ``layer1`` starting from 64 channels): the shape that takes a
robustly pre-trained ImageNet ResNet-50, which the reference's trainer builds for every config whose ``ADDENDUM`` does
not contain "clean" (tools/train_rob_seg.py:92-98), i.e. the PSPNet of PIR-AT.

Same modules, names and state-dict keys as the reference (370 keys for ``clean=True``, 358 for ``clean=False``, ``aux.*``
included), so a reference checkpoint loads with ``strict=True``.  ``indicate == 1``, bf16 autocast and CPU tensors run the
reference's forward on plain torch ops.  The
frozen eval forward of a float32 device batch -- what SEA attacks -- and its input gradient run on the device kernels
("PSPNet"):

- 1x1 convolutions (stride 1): M8 with the eval BatchNorm folded in (``_PointwiseRelu`` / ``_linear_frozen``);
- 3x3 stride-1 convolutions: the F(4x4,3x3) Winograd path (M1) with BatchNorm + ReLU in its epilogue;
- the dilated 3x3 convolutions of layer3 / layer4: P1 polyphase split -> Winograd on the d*d sub-images -> P1 merge;
- layer2's stride-2 1x1 downsample: P1 phase (0, 0), then M8;
- the bottleneck's ``relu(bn3(conv3(.)) + identity)``: M8 with the folded bias, then P3;
- PPM: the adaptive pool of M2'', M8, and P2 writing the align_corners=True up-sampling straight into the concatenation;
- ``cls``: Winograd 4096 -> 512, then the M10 classifier GEMM (NCHW logits), then P2 (x8, align_corners=True).
- the ``clean=False`` stem, convolution + BatchNorm + ReLU + max-pool: P4 (csrc/psp_stem.hip), one launch per direction, the
  pre-pool map never written (``STEM_FUSED``, read once from ``SEA_PSP_STEM_FUSED``, default 1; 0 = the library line).
The deep-base stem's stride-2 3-input-channel convolution and max-pool and layer2's stride-2 3x3 stay with the library
(about 1 % of the FLOPs).  There is deliberately no ``forward_lowres`` hook: K2u and K10b assume align_corners=False.

Training mode (PIR-AT's outer step, tools/train_rob_seg.py) of a float32 device batch keeps the reference's module order and
return value ``(main_loss, aux_loss, x)``; every BatchNorm runs on T1 (train-mode statistics, running-buffer update and
the following ReLU / residual add + ReLU in HIP) after the library convolution, the dilated 3x3 convolutions become P1
split -> dense 3x3 convolutions of the B*d*d sub-images -> P1 merge, and the align_corners=True up-samplings run on P2.

``TRAIN_CRITERION`` (read once from ``SEA_PSP_TRAIN_CRITERION``; ``torch`` | ``native`` | ``fused``, default ``torch``)
chooses the tail of that training forward when ``model.criterion`` is a plain mean ``nn.CrossEntropyLoss`` without label
smoothing (any other criterion keeps the torch line; ``weight`` and ``ignore_index`` are honoured):
- ``torch``: P2 on both heads, then ``model.criterion`` on the two full-resolution tensors;
- ``native``: P2 on both heads, then T2 (csrc/train_loss.hip) in place of the library's cross-entropy;
- ``fused``: T2u-ac (csrc/train_loss_up.hip, align_corners=True) on the heads' LOW-resolution logits: no full-resolution
  tensor is created, and the third element of the return value is ``None`` (as UperNet's ``(loss, None)``).  With
  ``zoom_factor == 1`` there is nothing to fuse and the mode is ``native``.

``USE_NATIVE = False`` runs the plain torch forward in both modes (A/B runs, the stock yardstick of the tests)."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import convnext_upernet as _M       # WINOGRAD_TILE / WINOGRAD_MIN_PIXELS are read from there at call time
from .convnext_upernet import (_PointwiseRelu, _WinoConv3x3, _classify, _adaptive_pool, _dense_cl, _folded_bn, _fp32_bwd,
                               _fp32_fwd, _linear_frozen, _split_ok, _stable, _tkey, _wino_ok)

USE_NATIVE = True
_CL = torch.channels_last
TRAIN_CRITERIA = ("torch", "native", "fused")
TRAIN_CRITERION = os.environ.get("SEA_PSP_TRAIN_CRITERION", "").strip() or "torch"
STEM_FUSED = os.environ.get("SEA_PSP_STEM_FUSED", "1").strip() != "0"     # P4 for the clean=False stem of the frozen model
if TRAIN_CRITERION not in TRAIN_CRITERIA:
    raise ValueError(f"SEA_PSP_TRAIN_CRITERION must be one of {TRAIN_CRITERIA}, got {TRAIN_CRITERION!r}")


# ---------------------------------------------------------------------------------------------------- modules
class Bottleneck(nn.Module):
    """resnet_ddcat.py:70-107"""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, BatchNorm=nn.BatchNorm2d):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = BatchNorm(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = BatchNorm(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = BatchNorm(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        residual = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            residual = self.downsample(x)
        out += residual
        return self.relu(out)


def _make_layer(inplanes, planes, blocks, stride, BatchNorm):
    """resnet_ddcat.py:146-166"""
    downsample = None
    if stride != 1 or inplanes != planes * Bottleneck.expansion:
        downsample = nn.Sequential(nn.Conv2d(inplanes, planes * Bottleneck.expansion, kernel_size=1, stride=stride,
                                             bias=False), BatchNorm(planes * Bottleneck.expansion))
    layers = [Bottleneck(inplanes, planes, stride, downsample, BatchNorm)]
    layers += [Bottleneck(planes * Bottleneck.expansion, planes, BatchNorm=BatchNorm) for _ in range(1, blocks)]
    return nn.Sequential(*layers)


class PPM(nn.Module):
    """ddcat_psp.py:8-30"""

    def __init__(self, in_dim, reduction_dim, bins, BatchNorm):
        super().__init__()
        self.features = nn.ModuleList(
            nn.Sequential(nn.AdaptiveAvgPool2d(b), nn.Conv2d(in_dim, reduction_dim, kernel_size=1, bias=False),
                          BatchNorm(reduction_dim), nn.ReLU(inplace=True)) for b in bins)

    def forward(self, x):
        size = x.shape[2:]
        return torch.cat([x] + [F.interpolate(f(x), size, mode="bilinear", align_corners=True) for f in self.features], 1)


def _conv3x3(cin, cout, stride=1):
    return nn.Conv2d(cin, cout, kernel_size=3, stride=stride, padding=1, bias=False)


def _build_backbone(model, BatchNorm, clean):
    """``layer0`` .. ``layer4`` of the reference's dilated ResNet-50 as children of ``model`` (which must have no other
    child yet: the initialisation walks ``model.modules()``), output stride 8"""
    if clean:
        model.layer0 = nn.Sequential(_conv3x3(3, 64, 2), BatchNorm(64), nn.ReLU(inplace=True),
                                    _conv3x3(64, 64), BatchNorm(64), nn.ReLU(inplace=True),
                                    _conv3x3(64, 128), BatchNorm(128), nn.ReLU(inplace=True),
                                    nn.MaxPool2d(kernel_size=3, stride=2, padding=1))
    else:                                                           # ddcat_psp.py:418-419
        model.layer0 = nn.Sequential(nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False), BatchNorm(64),
                                    nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2, padding=1))
    model.layer1 = _make_layer(128 if clean else 64, 64, 3, 1, BatchNorm)
    model.layer2 = _make_layer(256, 128, 4, 2, BatchNorm)
    model.layer3 = _make_layer(512, 256, 6, 2, BatchNorm)
    model.layer4 = _make_layer(1024, 512, 3, 2, BatchNorm)
    for m in model.modules():                                        # resnet_ddcat.py:139-144
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        elif isinstance(m, BatchNorm):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)
    for n, m in model.layer3.named_modules():                        # ddcat_psp.py:429-438
        if "conv2" in n:
            m.dilation, m.padding, m.stride = (2, 2), (2, 2), (1, 1)
        elif "downsample.0" in n:
            m.stride = (1, 1)
    for n, m in model.layer4.named_modules():
        if "conv2" in n:
            m.dilation, m.padding, m.stride = (4, 4), (4, 4), (1, 1)
        elif "downsample.0" in n:
            m.stride = (1, 1)


class PSPNet(nn.Module):
    """``PSPNet(50, n_cls)`` of the reference (ddcat_psp.py:372-486).  ``pretrained`` is accepted and ignored (the
    reference reads fixed cluster paths there); only ``layers=50`` is built.  ``clean`` chooses the stem: the deep-base one
    (True) or the torchvision-style one that a pre-trained ImageNet ResNet-50 fits (False: resnet_ddcat.py:115-131)."""

    def __init__(self, layers=50, classes=21, bins=(1, 2, 3, 6), dropout=0.1, zoom_factor=8, use_ppm=True,
                 criterion=nn.CrossEntropyLoss(ignore_index=-1), BatchNorm=nn.BatchNorm2d, pretrained=True, clean=True):
        super().__init__()
        if layers != 50:
            raise ValueError(f"PSPNet: only layers=50 is built here, got {layers}")
        assert 2048 % len(bins) == 0
        assert classes > 1
        assert zoom_factor in [1, 2, 4, 8]
        self.zoom_factor = zoom_factor
        self.use_ppm = use_ppm
        self.criterion = criterion
        _build_backbone(self, BatchNorm, clean)
        fea_dim = 2048
        if use_ppm:
            self.ppm = PPM(fea_dim, int(fea_dim / len(bins)), bins, BatchNorm)
            fea_dim *= 2
        self.cls = nn.Sequential(nn.Conv2d(fea_dim, 512, kernel_size=3, padding=1, bias=False), BatchNorm(512),
                                 nn.ReLU(inplace=True), nn.Dropout2d(p=dropout), nn.Conv2d(512, classes, kernel_size=1))
        if self.training:        # always true here: the reference's key list has aux.*
            self.aux = nn.Sequential(nn.Conv2d(1024, 256, kernel_size=3, padding=1, bias=False), BatchNorm(256),
                                     nn.ReLU(inplace=True), nn.Dropout2d(p=dropout), nn.Conv2d(256, classes, kernel_size=1))

    def _native_ok(self, x, indicate):
        return (USE_NATIVE and not self.training and indicate != 1 and x.is_cuda and x.dtype == torch.float32
                and x.dim() == 4 and not torch.is_autocast_enabled() and not any(p.requires_grad for p in self.parameters()))

    def _native_train_ok(self, x, indicate):
        return (USE_NATIVE and self.training and indicate != 1 and x.is_cuda and x.dtype == torch.float32
                and x.dim() == 4 and not torch.is_autocast_enabled())

    def forward(self, x, y=None, indicate=0):
        x_size = x.size()
        assert (x_size[2] - 1) % 8 == 0 and (x_size[3] - 1) % 8 == 0
        h = int((x_size[2] - 1) / 8 * self.zoom_factor + 1)
        w = int((x_size[3] - 1) / 8 * self.zoom_factor + 1)
        if self._native_ok(x, indicate):
            return _native_forward(self, x, (h, w))
        if self._native_train_ok(x, indicate):
            return _native_train_forward(self, x, y, (h, w))

        x = self.layer0(x)
        x = self.layer1(x)
        x = self.layer2(x)
        x_tmp = self.layer3(x)
        x = self.layer4(x_tmp)
        if self.use_ppm:
            x = self.ppm(x)
        x = self.cls(x)
        if self.zoom_factor != 1:
            x = F.interpolate(x, size=(h, w), mode="bilinear", align_corners=True)
        if self.training or indicate == 1:
            aux = self.aux(x_tmp)
            if self.zoom_factor != 1:
                aux = F.interpolate(aux, size=(h, w), mode="bilinear", align_corners=True)
            main_loss = self.criterion(x, y)
            aux_loss = self.criterion(aux, y)
            return main_loss, aux_loss, x
        return x


# ---------------------------------------------------------------------------------------------------- device path
class _Polyphase(torch.autograd.Function):
    """P1 split (x -> the d*d sub-images as one batch, or phase (0, 0) alone); backward = merge"""

    @staticmethod
    @_fp32_fwd
    def forward(ctx, x, d, first_only):
        from .. import _native as N
        ctx.size, ctx.d, ctx.first = tuple(x.shape[2:]), d, first_only
        return N.polyphase_split(_dense_cl(x), d, first_only)

    @staticmethod
    @_fp32_bwd
    def backward(ctx, g):
        from .. import _native as N
        return N.polyphase_merge(_dense_cl(g), ctx.size, ctx.d, ctx.first), None, None


class _PolyphaseMerge(torch.autograd.Function):
    """P1 merge (the d*d sub-images -> the full map, tails cropped); backward = split"""

    @staticmethod
    @_fp32_fwd
    def forward(ctx, y, size, d):
        from .. import _native as N
        ctx.d = d
        return N.polyphase_merge(_dense_cl(y), size, d)

    @staticmethod
    @_fp32_bwd
    def backward(ctx, g):
        from .. import _native as N
        return N.polyphase_split(_dense_cl(g), ctx.d), None, None


class _AddRelu(torch.autograd.Function):
    """P3: relu(a + r) of two dense channels_last maps; backward: the output-gated gradient, to both inputs"""

    @staticmethod
    @_fp32_fwd
    def forward(ctx, a, r):
        from .. import _native as N
        y = N.add_relu(_dense_cl(a), _dense_cl(r))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @_fp32_bwd
    def backward(ctx, g):
        from .. import _native as N
        (y,) = ctx.saved_tensors
        gx = N.add_relu_backward(g if g.stride() == y.stride() else g.contiguous(memory_format=_CL), y)
        return gx, gx


class _UpsampleAC(torch.autograd.Function):
    """P2: F.interpolate(x, size, mode="bilinear", align_corners=True) of NCHW logits, forward and input gradient"""

    @staticmethod
    @_fp32_fwd
    def forward(ctx, x, size):
        from .. import _native as N
        ctx.in_size = tuple(x.shape[2:])
        return N.upsample_ac(x.contiguous(), size)

    @staticmethod
    @_fp32_bwd
    def backward(ctx, g):
        from .. import _native as N
        return N.upsample_ac_backward(g.contiguous(), ctx.in_size), None


class _UpCatAC(torch.autograd.Function):
    """P2: torch.cat([x] + [up_ac(t) for t in ts], 1) as one channels_last buffer; every up-sampled branch is written
    straight into its channel slice, and its gradient is gathered straight out of the matching slice"""

    @staticmethod
    @_fp32_fwd
    def forward(ctx, size, x, *ts):
        from .. import _native as N
        B, Cx, (H, W) = x.shape[0], x.shape[1], size
        buf = torch.empty(B, Cx + sum(t.shape[1] for t in ts), H, W, dtype=torch.float32, device=x.device, memory_format=_CL)
        buf[:, :Cx].copy_(x)
        off = Cx
        for t in ts:
            N.upsample_ac_cl(_dense_cl(t), size, out=buf[:, off:off + t.shape[1]])
            off += t.shape[1]
        ctx.cx, ctx.shapes = Cx, [tuple(t.shape) for t in ts]
        return buf

    @staticmethod
    @_fp32_bwd
    def backward(ctx, g):
        from .. import _native as N
        if N.cl_pixel_stride(g) != g.shape[1]:
            g = g.contiguous(memory_format=_CL)
        grads, off = [None, g[:, :ctx.cx]], ctx.cx
        for shp in ctx.shapes:
            grads.append(N.upsample_ac_cl_backward(g[:, off:off + shp[1]], shp[2:]))
            off += shp[1]
        return tuple(grads)


def _cache(mod):
    if not hasattr(mod, "_psp_cache"):
        object.__setattr__(mod, "_psp_cache", {})
    return mod._psp_cache


def _pointwise(conv, bn, x, relu):
    """bn(conv1x1(x)) (+ ReLU) of a dense channels_last map through M8, the eval BatchNorm folded into the weights / bias"""
    cache = _cache(conv)
    scale, shift = _folded_bn(bn, conv.bias, cache)
    key = (_tkey(conv.weight), cache["bn_key"])
    if cache.get("pw_key") != key:
        with torch.no_grad():
            w = conv.weight
            cache.update(pw_key=key, pw_w=_stable(cache.get("pw_w"), (w.view(w.shape[0], -1) * scale[:, None]).contiguous()))
    x = _dense_cl(x)
    B, C, H, W = x.shape
    x4 = x.permute(0, 2, 3, 1)
    if relu:
        x2 = x4.reshape(B * H * W, C)
        if _split_ok(x2, C):
            y = _PointwiseRelu.apply(x2, cache["pw_w"], shift, cache, B)
        else:
            y = torch.relu_(torch.addmm(shift, x2, cache["pw_w"].t()))
        return y.view(B, H, W, -1).permute(0, 3, 1, 2)
    return _linear_frozen(cache, x4, cache["pw_w"], shift).permute(0, 3, 1, 2)


def _dilated_ok(conv, x):
    """the dilated 3x3 convolutions of layer3 / layer4 through P1 + Winograd.  Eligibility by the pixels of ONE image's
    d*d sub-images together (so an image's arithmetic does not depend on its batch partners)"""
    d = conv.dilation[0]
    hs, ws = -(-x.shape[2] // d), -(-x.shape[3] // d)
    return (d > 1 and conv.dilation == (d, d) and conv.padding == (d, d) and conv.stride == (1, 1)
            and conv.kernel_size == (3, 3) and conv.groups == 1 and conv.padding_mode == "zeros"
            and _M.WINOGRAD_TILE in (2, 4) and conv.in_channels % 4 == 0 and conv.out_channels % 4 == 0
            and d * d * hs * ws >= _M.WINOGRAD_MIN_PIXELS)


def dilated_conv3x3(x, weight, d, cache, scale=None, shift=None, relu=False):
    """act(scale[c] * conv2d(x, weight, padding=d, dilation=d) + shift[c]) for frozen 3x3 filters: P1 split -> the
    Winograd convolution of the B*d*d sub-images -> P1 merge, forward and input gradient (exact re-indexing: the zero
    tails of the sub-images are the convolution's zero padding).  ``relu`` needs ``scale`` / ``shift`` (as _WinoConv3x3)."""
    s = _Polyphase.apply(x, d, False)
    y = _WinoConv3x3.apply(s, weight, _M.WINOGRAD_TILE, cache, scale, shift, relu)
    return _PolyphaseMerge.apply(y, tuple(x.shape[2:]), d)


def _conv3x3_bn_relu(conv, bn, x):
    """relu(bn(conv(x))) for a 3x3 convolution of the frozen model"""
    if conv.stride == (1, 1) and conv.dilation == (1, 1) and _wino_ok(conv, x):
        scale, shift = _folded_bn(bn, conv.bias, _cache(conv))
        return _WinoConv3x3.apply(_dense_cl(x), conv.weight, _M.WINOGRAD_TILE, _cache(conv), scale, shift, True)
    if _dilated_ok(conv, x):
        scale, shift = _folded_bn(bn, conv.bias, _cache(conv))
        return dilated_conv3x3(x, conv.weight, conv.dilation[0], _cache(conv), scale, shift, True)
    return F.relu(bn(conv(x)))                      # library: stem conv1, layer2's strided 3x3, small maps


def _block(blk, x):
    out = _pointwise(blk.conv1, blk.bn1, x, True)
    out = _conv3x3_bn_relu(blk.conv2, blk.bn2, out)
    out = _pointwise(blk.conv3, blk.bn3, out, False)
    if blk.downsample is not None:
        conv, bn = blk.downsample[0], blk.downsample[1]
        if conv.stride == (1, 1):
            residual = _pointwise(conv, bn, x, False)
        elif conv.stride == (2, 2) and x.shape[1] % 4 == 0:
            residual = _pointwise(conv, bn, _Polyphase.apply(x, 2, True), False)
        else:
            residual = bn(conv(x))
    else:
        residual = x
    return _AddRelu.apply(out, residual)


class _RobustStem(torch.autograd.Function):
    """P4: maxpool3x3s2p1(relu(scale * conv7x7s2p3(x, w) + shift)) of the NCHW image as one launch, channels_last result;
    backward: the input gradient as a gather through the one-byte winner record (frozen weights: no other gradient)"""

    @staticmethod
    @_fp32_fwd
    def forward(ctx, x, weight, scale, shift):
        from .. import _native as N
        out, rec = N.psp_stem(x.contiguous(), weight, scale, shift, want_rec=ctx.needs_input_grad[0])
        ctx.size = tuple(x.shape[2:])
        ctx.save_for_backward(rec, weight, scale)
        return out

    @staticmethod
    @_fp32_bwd
    def backward(ctx, g):
        from .. import _native as N
        rec, weight, scale = ctx.saved_tensors
        return N.psp_stem_backward(_dense_cl(g), rec, weight, scale, *ctx.size), None, None, None


def _robust_stem_ok(l0):
    conv = l0[0]
    return (tuple(conv.weight.shape) == (64, 3, 7, 7) and conv.stride == (2, 2) and conv.padding == (3, 3)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == "zeros"
            and conv.weight.dtype == torch.float32 and conv.weight.is_contiguous() and isinstance(l0[3], nn.MaxPool2d)
            and (l0[3].kernel_size, l0[3].stride, l0[3].padding, l0[3].dilation, l0[3].ceil_mode) == (3, 2, 1, 1, False))


def _native_backbone(model, x):
    """``layer0`` .. ``layer4`` of the frozen dilated ResNet-50 on the device path (shared with DeepLabV3, whose backbone
    is this one layer for layer): (layer4's output, layer3's output), dense channels_last"""
    l0 = model.layer0
    if len(l0) == 4:                                # clean=False: conv7x7 s2, bn, relu, maxpool
        if STEM_FUSED and _robust_stem_ok(l0):
            scale, shift = _folded_bn(l0[1], l0[0].bias, _cache(l0[0]))
            x = _RobustStem.apply(x, l0[0].weight, scale, shift)
        else:
            x = _dense_cl(l0[3](F.relu(l0[1](l0[0](x.contiguous(memory_format=_CL))))))
    else:
        x = x.contiguous(memory_format=_CL)
        x = F.relu(l0[1](l0[0](x)))                 # stride 2, 3 input channels: the library (MIOpen)
        x = _conv3x3_bn_relu(l0[3], l0[4], x)
        x = _conv3x3_bn_relu(l0[6], l0[7], x)
        x = _dense_cl(l0[9](x))
    for layer in (model.layer1, model.layer2, model.layer3):
        for blk in layer:
            x = _block(blk, x)
    x_tmp = x
    for blk in model.layer4:
        x = _block(blk, x)
    return x, x_tmp


def _native_forward(model, x, size):
    x, _ = _native_backbone(model, x)
    if model.use_ppm:
        branches = [_pointwise(f[1], f[2], _adaptive_pool(f[0], x), True) for f in model.ppm.features]
        x = _UpCatAC.apply(tuple(x.shape[2:]), x, *branches)
    y = _conv3x3_bn_relu(model.cls[0], model.cls[1], x)
    logits = _classify(model.cls[4], _dense_cl(y))
    if model.zoom_factor == 1:
        return logits
    return _UpsampleAC.apply(logits.contiguous(), size)


# ---------------------------------------------------------------------------------------------------- training path
class _BNTrain(torch.autograd.Function):
    """T1: [relu](batch_norm(x, training=True) [+ r]) of a dense channels_last map.  gamma / beta are inputs (their
    gradients reach DDP's hooks); the running buffers of ``bn`` are updated in place."""

    @staticmethod
    def forward(ctx, x, weight, bias, r, bn, relu):
        from .. import _native as N
        x = _nhwc(x)
        y, mean, invstd, scale = N.bn_train_forward(x, weight, bias, bn.running_mean, bn.running_var,
                                                    bn.num_batches_tracked, bn.eps, bn.momentum, relu,
                                                    None if r is None else _nhwc(r))
        ctx.relu, ctx.res = relu, r is not None
        ctx.save_for_backward(x, y if relu else None, mean, invstd, scale)
        return y

    @staticmethod
    def backward(ctx, g):
        from .. import _native as N
        x, y, mean, invstd, scale = ctx.saved_tensors
        dx, dw, db, gr = N.bn_train_backward(_nhwc(g), x, y, mean, invstd, scale, ctx.relu, ctx.res)
        return dx, dw, db, gr, None, None


def _nhwc(t):
    """``t`` itself if its memory is dense NHWC (a 1 x 1 map in either stride form included), else a channels_last copy"""
    return t if t.is_contiguous(memory_format=_CL) else t.contiguous(memory_format=_CL)


def _t1_ok(bn, x):
    """what T1 covers: an affine BatchNorm2d on batch statistics with a float momentum, fp32 device maps, C % 4 == 0"""
    return (type(bn) is nn.BatchNorm2d and bn.training and bn.affine and bn.track_running_stats
            and bn.momentum is not None and bn.weight.dtype == torch.float32 and x.dtype == torch.float32 and x.is_cuda
            and x.dim() == 4 and x.shape[1] % 4 == 0 and x.shape[0] * x.shape[2] * x.shape[3] >= 2)


def _bn_train(bn, x, relu, r=None):
    """[relu](bn(x) [+ r]) in training mode: T1, or the torch modules where T1 does not apply"""
    if _t1_ok(bn, x):
        return _BNTrain.apply(x, bn.weight, bn.bias, r, bn, relu)
    y = bn(x)
    if r is not None:
        y = y + r
    return F.relu(y) if relu else y


def _dilated_train_ok(conv, x):
    d = conv.dilation[0]
    return (d > 1 and conv.dilation == (d, d) and conv.padding == (d, d) and conv.stride == (1, 1)
            and conv.kernel_size == (3, 3) and conv.groups == 1 and conv.padding_mode == "zeros" and conv.bias is None
            and x.is_cuda and x.dtype == torch.float32 and x.shape[1] % 4 == 0)


def dilated_conv3x3_train(x, weight, d):
    """conv2d(x, weight, padding=d, dilation=d) of a trainable 3x3 filter: P1 split -> the library's dense 3x3 / pad-1
    convolution of the B*d*d sub-images -> P1 merge.  The exact re-indexing of ``dilated_conv3x3``: the weight and input
    gradients flow through autograd, and the library only sees dense 3x3 convolutions."""
    s = _Polyphase.apply(x, d, False)
    return _PolyphaseMerge.apply(F.conv2d(s, weight, padding=1), tuple(x.shape[2:]), d)


def _conv_train(conv, x):
    if _dilated_train_ok(conv, x):
        return dilated_conv3x3_train(x, conv.weight, conv.dilation[0])
    return conv(x)


def _block_train(blk, x):
    out = _bn_train(blk.bn1, blk.conv1(x), True)
    out = _bn_train(blk.bn2, _conv_train(blk.conv2, out), True)
    out = blk.conv3(out)
    residual = x if blk.downsample is None else _bn_train(blk.downsample[1], blk.downsample[0](x), False)
    return _bn_train(blk.bn3, out, True, residual)


def _up_ac_train(t, size):
    return _UpsampleAC.apply(t.contiguous(), size)


def _native_train_forward(model, x, y, size):
    """``PSPNet.forward`` in training mode (ddcat_psp.py:453-478) on the device path: same modules in the same order"""
    l0 = model.layer0
    x = x.contiguous(memory_format=_CL)
    x = _bn_train(l0[1], l0[0](x), True)
    if len(l0) == 4:                                # clean=False: library convolution (weight gradient), T1, library pool
        x = l0[3](x)
    else:
        x = _bn_train(l0[4], _conv_train(l0[3], x), True)
        x = _bn_train(l0[7], _conv_train(l0[6], x), True)
        x = l0[9](x)
    for layer in (model.layer1, model.layer2, model.layer3):
        for blk in layer:
            x = _block_train(blk, x)
    x_tmp = x
    for blk in model.layer4:
        x = _block_train(blk, x)
    if model.use_ppm:
        branches = [_bn_train(f[2], f[1](f[0](x)), True) for f in model.ppm.features]
        x = _UpCatAC.apply(tuple(x.shape[2:]), _dense_cl(x), *[_dense_cl(b) for b in branches])
    cls, aux = model.cls, model.aux
    x = cls[4](cls[3](_bn_train(cls[1], _conv_train(cls[0], x), True)))
    a = aux[4](aux[3](_bn_train(aux[1], _conv_train(aux[0], x_tmp), True)))
    crit = _device_criterion(model.criterion, y)
    if crit is not None:
        y = y.contiguous()
    if crit is not None and TRAIN_CRITERION == "fused" and model.zoom_factor != 1:
        assert tuple(y.shape[-2:]) == tuple(size)      # (F.cross_entropy would refuse any other label size)
        return crit.upsampled(x, y, align_corners=True), crit.upsampled(a, y, align_corners=True), None
    if model.zoom_factor != 1:
        x = _up_ac_train(x, size)
        a = _up_ac_train(a, size)
    if crit is not None:
        return crit(x.contiguous(), y), crit(a.contiguous(), y), x
    return model.criterion(x, y), model.criterion(a, y), x


def _device_criterion(criterion, y):
    """``TRAIN_CRITERION`` native / fused: ``criterion`` as a ``semseg.losses.CrossEntropy(native=True)`` (T2 / T2u-ac) if it
    is a plain mean cross-entropy over int64 device labels, else None (the torch line).  Built per call: it holds no state
    but the criterion's own weight tensor."""
    if TRAIN_CRITERION not in TRAIN_CRITERIA:
        raise ValueError(f"pspnet.TRAIN_CRITERION must be one of {TRAIN_CRITERIA}, got {TRAIN_CRITERION!r}")
    if (TRAIN_CRITERION == "torch" or type(criterion) is not nn.CrossEntropyLoss or criterion.reduction != "mean"
            or criterion.label_smoothing != 0 or y is None or not y.is_cuda or y.dtype != torch.int64 or y.dim() != 3):
        return None
    from ..losses import CrossEntropy
    return CrossEntropy(criterion.ignore_index, criterion.weight, native=True)
