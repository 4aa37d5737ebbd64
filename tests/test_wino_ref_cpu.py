"""The float64 reference of the Winograd transforms (oracle/sea_oracle.py: wino_input_f64 / wino_filter_f64 /
wino_output_f64) pinned on the CPU, with no library: the three transforms around the Winograd-domain products ARE the 3 x 3 /
stride 1 / pad 1 convolution, to the rounding of float64.  tests/test_wino_transforms_gpu.py compares the kernels with it."""
import pytest
import torch
import torch.nn.functional as F

from oracle import sea_oracle as O

REL = 1e-12  # of max|reference| (a single tile measures 5e-16 at m = 2 and 3e-15 at m = 4)
SIZES = [(5, 7), (1, 1), (9, 6)]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _close(got_nhwc, want_nchw):
    want = _nhwc(want_nchw)
    assert got_nhwc.shape == want.shape
    err = (got_nhwc - want).abs().max().item()
    assert err <= REL * max(want.abs().max().item(), 1e-300), (err, want.abs().max().item())


def _conv(x_nhwc, U, B, H, W, m, **epilogue):
    V, _ = O.wino_input_f64(x_nhwc, m, epilogue.pop("gate", None), epilogue.pop("gate_scale", None))
    return O.wino_output_f64(torch.einsum("ktc,kcd->ktd", V, U), B, H, W, m, **epilogue)[0]


@pytest.mark.parametrize("m", [2, 4])
@pytest.mark.parametrize("size", SIZES)
def test_transforms_are_the_convolution(m, size):
    H, W = size
    B, Cin, Cout = 2, 3, 5
    g = torch.Generator().manual_seed(100 * H + W + m)
    x = torch.randn(B, Cin, H, W, dtype=torch.float64, generator=g).requires_grad_(True)
    w = torch.randn(Cout, Cin, 3, 3, dtype=torch.float64, generator=g)
    ref = F.conv2d(x, w, padding=1)
    U, _ = O.wino_filter_f64(w, m, False)
    assert U.shape == ((m + 2) ** 2, Cin, Cout)
    _close(_conv(_nhwc(x.detach()), U, B, H, W, m), ref.detach())
    # flip = 1: the input gradient of that convolution from its output gradient
    gy = torch.randn(B, Cout, H, W, dtype=torch.float64, generator=g)
    (gx,) = torch.autograd.grad(ref, x, gy)
    Ub, _ = O.wino_filter_f64(w, m, True)
    assert Ub.shape == ((m + 2) ** 2, Cout, Cin)
    _close(_conv(_nhwc(gy), Ub, B, H, W, m), gx)
    # ... which is the forward transform of the rotated, transposed filters
    assert torch.equal(Ub, O.wino_filter_f64(w.flip(2, 3).transpose(0, 1).contiguous(), m, False)[0])


@pytest.mark.parametrize("m", [2, 4])
@pytest.mark.parametrize("size", SIZES)
def test_gate_prologue_and_epilogue(m, size):
    H, W = size
    B, Cin, Cout = 2, 4, 3
    g = torch.Generator().manual_seed(7 * H + W + m)
    x = torch.randn(B, Cin, H, W, dtype=torch.float64, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, dtype=torch.float64, generator=g)
    gate = torch.randn(B, Cin, H, W, dtype=torch.float64, generator=g)
    gate[0, :, 0, 0] = 0.0
    gate[-1, :, -1, -1] = float("nan")
    gscale = torch.randn(Cin, dtype=torch.float64, generator=g)
    addend = torch.randn(B, Cout, H, W, dtype=torch.float64, generator=g)
    scale = torch.randn(Cout, dtype=torch.float64, generator=g)
    bias = torch.randn(Cout, dtype=torch.float64, generator=g)
    ch = lambda v: v[None, :, None, None]  # noqa: E731
    xin = torch.where(gate > 0, x * ch(gscale), torch.zeros_like(x))
    conv = F.conv2d(xin, w, padding=1)
    # the gate is a select: what x holds where it is closed does not matter
    xbad = x.clone()
    xbad[gate.isnan()] = float("inf")
    xbad[gate == 0] = float("nan")
    xbad[(gate < -1)] = float("-inf")
    U, _ = O.wino_filter_f64(w, m, False)
    for relu in (False, True):
        want = ch(scale) * (conv + addend) + ch(bias)
        got = _conv(_nhwc(xbad), U, B, H, W, m, gate=_nhwc(gate), gate_scale=gscale, addend=_nhwc(addend), scale=scale,
                    bias=bias, relu=relu)
        _close(got, torch.relu(want) if relu else want)
    # every part of the epilogue alone, and the gate without a scale
    _close(_conv(_nhwc(xbad), U, B, H, W, m, gate=_nhwc(gate)),
           F.conv2d(torch.where(gate > 0, x, torch.zeros_like(x)), w, padding=1))
    plain = F.conv2d(x, w, padding=1)
    _close(_conv(_nhwc(x), U, B, H, W, m, addend=_nhwc(addend)), plain + addend)
    _close(_conv(_nhwc(x), U, B, H, W, m, scale=scale), plain * ch(scale))
    _close(_conv(_nhwc(x), U, B, H, W, m, bias=bias), plain + ch(bias))
    _close(_conv(_nhwc(x), U, B, H, W, m, relu=True), torch.relu(plain))


@pytest.mark.parametrize("m", [2, 4])
def test_layouts_and_magnitudes(m):
    """tiles t = (b, ty, tx), k = i*A + j, zero halo; the magnitudes are the transforms of absolute values"""
    A = m + 2
    BT, G, AT = O.wino_matrices(m)
    assert BT.shape == (A, A) and G.shape == (A, 3) and AT.shape == (m, A)
    B, C, H, W = 2, 3, m + 1, 2 * m + 1
    nTh, nTw = 2, 3
    assert O.wino_tiles(B, H, W, m) == B * nTh * nTw
    g = torch.Generator().manual_seed(m)
    x = torch.randn(B, H, W, C, dtype=torch.float64, generator=g)
    V, mag = O.wino_input_f64(x, m)
    assert V.shape == mag.shape == (A * A, B * nTh * nTw, C)
    xp = torch.zeros(B, nTh * m + 2, nTw * m + 2, C, dtype=torch.float64)
    xp[:, 1:H + 1, 1:W + 1] = x
    for b, ty, tx, c in [(0, 0, 0, 0), (1, 1, 2, 2), (0, 1, 0, 1), (1, 0, 1, 0)]:
        d = xp[b, ty * m:ty * m + A, tx * m:tx * m + A, c]
        t = (b * nTh + ty) * nTw + tx
        assert torch.allclose(V[:, t, c].reshape(A, A), BT @ d @ BT.t(), rtol=0, atol=1e-13)
        assert torch.allclose(mag[:, t, c].reshape(A, A), BT.abs() @ d.abs() @ BT.abs().t(), rtol=0, atol=1e-13)
    assert (mag >= V.abs() - 1e-13).all()
    w = torch.randn(4, C, 3, 3, dtype=torch.float64, generator=g)
    for flip in (False, True):
        U, umag = O.wino_filter_f64(w, m, flip)
        o, c = 3, 1
        gg = w[o, c].flip(0, 1) if flip else w[o, c]
        got = (U[:, o, c] if flip else U[:, c, o]).reshape(A, A)
        assert torch.allclose(got, G @ gg @ G.t(), rtol=0, atol=1e-14)
        assert (umag >= U.abs() - 1e-14).all() and torch.equal(umag, O.wino_filter_f64(w.abs(), m, flip)[1])
    M = torch.randn(A * A, B * nTh * nTw, C, dtype=torch.float64, generator=g)
    y, ymag = O.wino_output_f64(M, B, H, W, m)
    assert y.shape == ymag.shape == (B, H, W, C)
    b, ty, tx, c = 1, 1, 2, 1
    tile = AT @ M[:, (b * nTh + ty) * nTw + tx, c].reshape(A, A) @ AT.t()
    assert torch.allclose(y[b, ty * m:, tx * m:, c], tile[:H - ty * m, :W - tx * m], rtol=0, atol=1e-13)
    assert (ymag >= y.abs() - 1e-13).all()
    # a closed gate leaves magnitude 0: the kernels must return exact zeros there
    gate = torch.ones(B, H, W, C)
    gate[0] = -1.0
    V0, mag0 = O.wino_input_f64(x, m, gate, None)
    per = nTh * nTw
    assert (V0[:, :per] == 0).all() and (mag0[:, :per] == 0).all() and torch.equal(V0[:, per:], V[:, per:])
    with pytest.raises(ValueError):
        O.wino_matrices(3)
