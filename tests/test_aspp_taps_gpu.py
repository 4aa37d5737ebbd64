"""P5, the ASPP tap sum and its adjoint (csrc/aspp_kernels.hip), on the device: bitwise against a torch restatement that
adds the shifted slices in tap order, bitwise gradient against autograd through that restatement, determinism, the
argument errors, and the ASPP module built on it (one product + P5 for the three dilated branches) against
F.conv2d(dilation=r) + BatchNorm + ReLU in float64."""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

_CL = torch.channels_last
SHAPES = ((2, 9, 9), (1, 8, 13), (2, 20, 20), (1, 17, 23))
RATES = ((6, 12, 18), (1, 2, 3))
PAD0, PAD1 = 8, 4              # channels in front of / behind the slice of the wider output buffer
ZCOL0, ZTAIL = 4, 8            # columns in front of / behind the branch columns of the wider product


def _restated(z, rates, shift, Cb):
    """the written-out sum: acc = 0; for t = 0 .. 8: acc += the slice of tap t shifted by ((ky-1) rate, (kx-1) rate) (zero
    where the source lies outside the map: acc + 0 leaves acc's bits); + shift; ReLU.  z: (B, H, W, 9 R Cb)"""
    B, H, W, _ = z.shape
    R = len(rates)
    zz = z.view(B, H, W, R, 9, Cb)
    outs = []
    for r, rate in enumerate(rates):
        acc = torch.zeros(B, H, W, Cb, dtype=z.dtype, device=z.device)
        for t in range(9):
            dy, dx = (t // 3 - 1) * rate, (t % 3 - 1) * rate
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            src = zz[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx, r, t]
            acc = acc + F.pad(src, (0, 0, x0, W - x1, y0, H - y1))
        outs.append(acc)
    return torch.relu(torch.cat(outs, -1) + shift)


def _inputs(B, H, W, Cb, rates, seed):
    g = torch.Generator().manual_seed(seed)
    R = len(rates)
    zfull = torch.randn(B, H, W, ZCOL0 + 9 * R * Cb + ZTAIL, generator=g).cuda()
    shift = (0.5 * torch.randn(R * Cb, generator=g)).cuda()
    gfull = torch.randn(B, H, W, PAD0 + R * Cb + PAD1, generator=g).cuda().permute(0, 3, 1, 2)
    return zfull, shift, gfull


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("Cb", [256, 12])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_tap_sum_and_its_adjoint_are_bitwise_the_restatement(B, H, W, Cb, rates):
    from semseg import _native as N
    R = len(rates)
    zfull, shift, gfull = _inputs(B, H, W, Cb, rates, seed=B + 3 * H + 5 * W + Cb + rates[0])
    z = zfull[..., ZCOL0:ZCOL0 + 9 * R * Cb].contiguous().requires_grad_(True)
    want = _restated(z, rates, shift, Cb)

    buf = torch.zeros(B, H, W, PAD0 + R * Cb + PAD1, device="cuda").permute(0, 3, 1, 2)
    sl = buf[:, PAD0:PAD0 + R * Cb]
    got = N.aspp_tap_sum(zfull, rates, shift, out=sl, z_col0=ZCOL0)
    assert got.data_ptr() == sl.data_ptr()
    assert torch.equal(sl.permute(0, 2, 3, 1), want.detach())
    assert not buf[:, :PAD0].any() and not buf[:, PAD0 + R * Cb:].any()            # nothing written outside the slice
    assert (sl > 0).any() and (sl == 0).any()
    # every branch has taps that are skipped at these sizes, and (but for the centre-only cases) taps that are not
    again = torch.zeros_like(buf)
    N.aspp_tap_sum(zfull, rates, shift, out=again[:, PAD0:PAD0 + R * Cb], z_col0=ZCOL0)
    assert torch.equal(again, buf)                                                  # determinism
    # a dense output of its own
    assert torch.equal(N.aspp_tap_sum(z.detach(), rates, shift), sl)

    gsl = gfull[:, PAD0:PAD0 + R * Cb]
    (gwant,) = torch.autograd.grad(want, [z], gsl.permute(0, 2, 3, 1))
    dz = torch.full_like(zfull, float("nan"))
    N.aspp_tap_sum_backward(gsl, sl, rates, z_col0=ZCOL0, out=dz)
    assert torch.equal(dz[..., ZCOL0:ZCOL0 + 9 * R * Cb], gwant)                    # one term per element: no tolerance
    assert dz[..., :ZCOL0].isnan().all() and dz[..., ZCOL0 + 9 * R * Cb:].isnan().all()
    dz2 = torch.full_like(zfull, float("nan"))
    N.aspp_tap_sum_backward(gsl, sl, rates, z_col0=ZCOL0, out=dz2)
    assert torch.equal(dz2[..., ZCOL0:ZCOL0 + 9 * R * Cb], dz[..., ZCOL0:ZCOL0 + 9 * R * Cb])
    assert torch.equal(N.aspp_tap_sum_backward(gsl.contiguous(memory_format=_CL), sl, rates), gwant)


def test_bad_arguments_return_the_argument_error_and_launch_nothing():
    from semseg import _native as N
    lib = N.lib()
    B, H, W, R, Cb = 1, 9, 9, 3, 12
    ldz, ldy = 9 * R * Cb, R * Cb
    z = torch.randn(B, H, W, ldz + 4, device="cuda")
    shift = torch.zeros(R * Cb, device="cuda")
    y = torch.full((B, H, W, ldy + 4), float("nan"), device="cuda")
    dy = torch.randn(B, H, W, ldy + 4, device="cuda")
    dz = torch.full((B, H, W, ldz + 4), float("nan"), device="cuda")
    good = (ctypes.c_int * 3)(6, 12, 18)
    zero = (ctypes.c_int * 3)(6, 0, 18)
    st = N._stream()

    def fwd(ldz_=ldz, ldy_=ldy, Cb_=Cb, rates=good, R_=R, zc=0, yc=0):
        return lib.sea_aspp_tap_sum(z.data_ptr(), ldz_, zc, shift.data_ptr(), y.data_ptr(), ldy_, yc, B, H, W, R_, Cb_, rates, st)

    def bwd(ldz_=ldz, ldy_=ldy, Cb_=Cb, rates=good, R_=R, zc=0, yc=0):
        return lib.sea_aspp_tap_sum_backward(dy.data_ptr(), ldy_, yc, y.data_ptr(), ldy_, yc, dz.data_ptr(), ldz_, zc, B, H, W,
                                             R_, Cb_, rates, st)

    for f in (fwd, bwd):
        assert f(rates=zero) == 1                       # a rate of 0
        assert f(Cb_=10) == 1                           # Cb % 4 != 0
        assert f(ldz_=ldz + 2) == 1                     # an unaligned stride
        assert f(ldy_=ldy + 2) == 1
        assert f(R_=5) == 1 and f(R_=0) == 1            # 1 <= R <= 4
        assert f(zc=8) == 1 and f(yc=8) == 1            # the branch columns would leave the pixel
        assert f(zc=2, ldz_=ldz + 4) == 1               # an unaligned first column
    torch.cuda.synchronize()
    assert y.isnan().all() and dz.isnan().all()         # nothing was launched
    with pytest.raises(N.SeaNativeError):
        N.aspp_tap_sum(z[..., :ldz].contiguous(), (6, 0, 18), shift)
    with pytest.raises(N.SeaNativeError):
        N.aspp_tap_sum(z[..., :ldz], (6, 12, 18), shift)                            # a strided product
    # the same calls with good arguments run
    assert fwd(ldz_=ldz + 4, ldy_=ldy + 4) == 0 and bwd(ldz_=ldz + 4, ldy_=ldy + 4) == 0
    torch.cuda.synchronize()
    assert not y[..., :ldy].isnan().any() and y[..., ldy:].isnan().all()
    assert not dz[..., :ldz].isnan().any() and dz[..., ldz:].isnan().all()


# ------------------------------------------------------------------------------------------------------------ the module
def _aspp(seed):
    from semseg.models.deeplabv3 import ASPP
    g = torch.Generator().manual_seed(seed)
    m = ASPP(2048, 256, (6, 12, 18), nn.BatchNorm2d)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.Conv2d):
                fan_in = mod.weight[0].numel()
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
            elif isinstance(mod, nn.BatchNorm2d):
                mod.weight.copy_(0.5 + torch.rand(mod.weight.shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
                mod.running_mean.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
                mod.running_var.copy_(0.5 + 1.5 * torch.rand(mod.bias.shape, generator=g))
    m.eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


NEAR_ZERO = 1e-5


@pytest.mark.parametrize("B,H,W", [(2, 20, 20), (2, 9, 9)])
def test_aspp_module_matches_fp64(B, H, W):
    """Forward and input gradient of the device ASPP against the module's own float64 forward on the CPU
    (F.conv2d(dilation=r) + BatchNorm + ReLU for every branch).  An output element whose float64 pre-activation lies
    within NEAR_ZERO of zero may have its ReLU gate on the other side in float32; such elements are taken out of the
    gradient comparison by zeroing the incoming gradient there, on both sides alike.  Their share is printed and capped."""
    from semseg.models.deeplabv3 import aspp_forward
    m = _aspp(seed=H)
    md = copy.deepcopy(m).double()
    g = torch.Generator().manual_seed(100 + H)
    x = torch.relu(torch.randn(B, 2048, H, W, generator=g))            # (layer4's output is a ReLU's)
    gy = torch.randn(B, 1280, H, W, generator=g)

    xd = x.double().requires_grad_(True)
    pre = [seq[1](seq[0](xd)) for seq in md.convs[:-1]]
    pooled_pre = md.convs[-1][2](md.convs[-1][1](md.convs[-1][0](xd)))
    yd = torch.cat([torch.relu(p) for p in pre]
                   + [F.interpolate(torch.relu(pooled_pre), (H, W), mode="bilinear", align_corners=True)], 1)
    near = torch.cat([p.detach().abs() <= NEAR_ZERO for p in pre]
                     + [(pooled_pre.detach().abs() <= NEAR_ZERO).expand(B, 256, H, W)], 1)
    share = near.float().mean().item()
    gy = torch.where(near, torch.zeros(()), gy)
    (gxd,) = torch.autograd.grad(yd, [xd], gy.double())

    xi = x.cuda().contiguous(memory_format=_CL).requires_grad_(True)
    y = aspp_forward(m.cuda(), xi)
    assert y.shape == (B, 1280, H, W) and y.is_contiguous(memory_format=_CL)
    (gx,) = torch.autograd.grad(y, [xi], gy.cuda())
    ef = (y.detach().cpu().double() - yd.detach()).abs().max().item() / yd.abs().max().item()
    eb = (gx.cpu().double() - gxd).abs().max().item() / gxd.abs().max().item()
    per_branch = yd.detach().view(B, 5, 256, H, W).abs().amax((0, 2, 3, 4))
    print(f"ASPP {B}x2048x{H}x{W}: forward {ef:.2e}, input gradient {eb:.2e}, excluded share {share:.2e}, "
          f"branch maxima {[round(v, 2) for v in per_branch.tolist()]}")
    assert per_branch.min().item() > 0.1
    assert share <= 0.01
    assert ef <= 3e-4 and eb <= 3e-4
