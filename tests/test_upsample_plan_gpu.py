"""Every kernel of the M2 / tap-gather family, reached through the default dispatch on the smallest shape that selects it
(the pinned rows of tests/test_upsample_plan_cpu.py; the cases and the direct calls of the C entries are those of
devtools/upsample_plan_bits.py): the plan names the kernel for the tensors actually passed, their real addresses included, and the
result agrees with F.interpolate / its gradient in float64 on the CPU at the tolerances of
test_kernels_gpu.py::test_upsample_bilinear_forward_backward and ::test_upsample_bilinear_channels_last; the tap gather against the
composition of ::test_tap_gather_is_conv3x3_of_the_upsampled_input.  Needs a real MI355X: run with `-m gpu`."""
import pytest
import torch
import torch.nn.functional as F

from devtools.upsample_plan_bits import CASES, dst_shape, run, src_shape

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    from semseg import _native
    _native.lib()  # raises if the extension is missing: no silent fallback
    return _native


def _up64(x, c):
    return F.interpolate(x, size=(c.H, c.W), mode="bilinear", align_corners=False)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_default_dispatch_reaches_the_kernel_and_the_values_hold(N, c):
    g = torch.Generator().manual_seed(c.h * 100 + c.H + len(c.name))
    nchw, fwd = c.op.startswith("nchw"), c.op.endswith("fwd")
    to_nchw = (lambda t: t) if nchw else (lambda t: t.permute(0, 3, 1, 2))   # the entry's layout -> (B, C, rows, columns)
    if c.op.startswith("tap"):
        # conv3x3(up(f)) == tap_gather(f @ W): the coarse per-tap maps G come from a coarse input f and a 3x3 weight
        Cin = 8
        f = torch.randn(c.B, Cin, c.h, c.w, generator=g)
        wt = torch.randn(c.C, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
        Wl = wt.permute(2, 3, 0, 1).reshape(9 * c.C, Cin).contiguous()
        fd = f.double().requires_grad_(True)
        ref = F.conv2d(_up64(fd, c), wt.double(), padding=1)
        if fwd:
            src_cpu = F.linear(f.permute(0, 2, 3, 1).contiguous(), Wl).view(c.B, c.h, c.w, 9, c.C)
        else:
            gz = torch.randn(c.B, c.C, c.H, c.W, generator=g)
            (gf_ref,) = torch.autograd.grad(ref, fd, gz.double())
            src_cpu = gz.permute(0, 2, 3, 1).contiguous()
    else:
        shape = (c.B, c.C, c.h, c.w) if fwd else (c.B, c.C, c.H, c.W)
        t = torch.randn(shape, generator=g)
        src_cpu = t if nchw else t.permute(0, 2, 3, 1).contiguous()
        xd = (t if fwd else torch.zeros(c.B, c.C, c.h, c.w)).double().requires_grad_(True)
        ref = _up64(xd, c)
        if not fwd:
            (gx_ref,) = torch.autograd.grad(ref, xd, t.double())
    assert tuple(src_cpu.shape) == src_shape(c)

    src, out = run(N, c, src_cpu)
    # 1. the default dispatch reaches the kernel of this case, with these tensors
    n = c.B * c.C if nchw else c.B
    plan = N.upsample_plan(c.op, n, c.h, c.w, c.H, c.W, C_=c.C, src_addr=src.data_ptr(), dst_addr=out.data_ptr())
    assert (plan["rc"], plan["kernel"], plan["S"]) == (0, c.kernel, c.S), plan
    assert src.data_ptr() % 16 == 4 * c.src_off and out.data_ptr() % 16 == 4 * c.dst_off
    # 2., 3. the values
    assert tuple(out.shape) == dst_shape(c) and not torch.isnan(out).any()
    got = out.cpu()
    if c.op == "tap_fwd":
        torch.testing.assert_close(to_nchw(got).double(), ref.detach(), rtol=2e-5, atol=2e-5)
    elif c.op == "tap_bwd":
        gf = torch.mm(got.view(c.B * c.h * c.w, -1), Wl).view(c.B, c.h, c.w, Cin).permute(0, 3, 1, 2)
        torch.testing.assert_close(gf.double(), gf_ref, rtol=1e-4, atol=1e-4)
    elif fwd:
        # float32 source indices (ATen's rule) carry ~1e-6 * src error in lambda for non-integer scales: tight against ATen's
        # own float32 result, a little looser against the float64 one
        torch.testing.assert_close(to_nchw(got), _up64(t, c), rtol=1e-5, atol=2e-5)
        torch.testing.assert_close(to_nchw(got).double(), ref.detach(), rtol=1e-5, atol=2e-4)
    else:
        fac = c.H // c.h                                                     # (by the shape, whichever kernel takes it)
        pow2 = nchw and fac in (2, 4, 8, 16) and c.H == fac * c.h and c.W == fac * c.w
        torch.testing.assert_close(to_nchw(got).double(), gx_ref, rtol=1e-5, atol=5e-5 if pow2 else 1e-3)
        assert torch.equal(out, run(N, c, src_cpu)[1])                       # deterministic gather


def test_refusals_are_the_plan_s_and_launch_nothing(N):
    """1x1 -> 40x40 has no tile for the NCHW backward; the tap gather needs a factor >= 3: SEA_ERR_ARG from the plan, and the
    same from the entry, which returns before any launch."""
    assert N.upsample_plan("nchw_bwd", 2, 1, 1, 40, 40)["rc"] == 1
    assert N.upsample_plan("tap_fwd", 1, 2, 2, 4, 4, C_=4)["rc"] == 1
    gy, gx = torch.zeros(2, 1, 40, 40, device="cuda"), torch.full((2, 1, 1, 1), 7.0, device="cuda")
    assert N.lib().sea_upsample_bilinear_bwd(gy.data_ptr(), gx.data_ptr(), 2, 1, 1, 40, 40, N._stream()) == 1
    G, extra = torch.zeros(1, 2, 2, 9, 4, device="cuda"), torch.full((1, 4, 4, 4), 7.0, device="cuda")
    assert N.lib().sea_tap_gather_fwd(G.data_ptr(), extra.data_ptr(), 0, 1, 4, 2, 2, 4, 4, 1, N._stream()) == 1
    assert (gx == 7).all() and (extra == 7).all()
