"""The three Winograd transform kernels (csrc/wino_kernels.hip; include/sea_hip.h, M4) compared directly with their float64
restatement (oracle/sea_oracle.py: wino_input_f64 / wino_filter_f64 / wino_output_f64), every variant, through the wrappers
that the shipped convolution uses.  The whole-convolution tests (test_kernels_gpu.py) are sized for the products in between
and never look at V, U, the per-tile scale words or the epilogue branches themselves.

Tolerances (derived, not tuned).  u = 2^-24; a two-stage transform L d L^T in fp32 has at most A = m + 2 roundings per stage
(at most A - 1 fused multiply-adds and the rounding of a non-dyadic coefficient: 1/6, 1/24; the per-channel scale of the gate
prologue is one of them), so

    |computed - exact| <= 2A u (|L| |d| |L^T|)     elementwise: 8u at m = 2, 12u at m = 4,

and the output transform adds one rounding for the addend and one for the scale / shift:

    |computed - exact| <= (2A + 2) u (|scale| (|A^T| |M| |A| + |addend|) + |bias|).

The oracle returns the magnitudes in brackets.  Where the magnitude is 0 the bound is 0 and the result must be an exact
zero.  ReLU is 1-Lipschitz, so the bound of the pre-activation holds for the activation as well (where the float64
pre-activation lies within the bound of 0, either side's value passes).  An fp32 emulation of the kernels' order on the CPU
stays below 2.8u (m = 2) and 4.0u (m = 4); a wrong coefficient, a transposed index or a misplaced halo is off by about 1/u
times the bound.  Every check prints its worst error in units of u x magnitude ("[wino ratio]")."""
import functools

import pytest
import torch

from oracle import sea_oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = -12345.5

# (B, C, H, W): each the smallest shape that reaches its path
SHAPES = [
    (1, 4, 1, 1),     # one tile, all halo
    (3, 4, 2, 3),     # odd tile count, partially active last wave
    (2, 8, 5, 7),     # ragged in both axes
    (1, 12, 9, 6),    # three channel groups: a wave's lanes span several tiles
    (1, 64, 8, 8),    # sixteen groups, four tiles per wave
    (2, 256, 5, 4),   # C/4 = 64: one wave is one tile, the wave-uniform scale-word branch (C/2 = 128 at vec4 = 0)
    (1, 384, 6, 6),   # 96 groups: waves straddle tile boundaries with all lanes active
]
VARIANTS = [(2, 1), (4, 0), (4, 1)]  # (m, vec4); vec4 only matters at m = 4
ids_shape = lambda s: "x".join(map(str, s))  # noqa: E731
ids_variant = lambda v: f"m{v[0]}v{v[1]}"  # noqa: E731
shapes = pytest.mark.parametrize("shape", SHAPES, ids=ids_shape)
variants = pytest.mark.parametrize("variant", VARIANTS, ids=ids_variant)


@pytest.fixture(scope="module")
def N():
    from semseg import _native
    _native.lib()  # raises if the library is missing: no fallback
    return _native


def cl(t_nhwc):
    """(B,H,W,C) memory as the channels_last (B,C,H,W) tensor that the wrappers take"""
    return t_nhwc.permute(0, 3, 1, 2)


def rand(shape, g, zeros=0.1):
    """magnitudes spread over 2^-8 .. 2^8, with exact zeros"""
    t = torch.randn(shape, generator=g) * torch.exp2(torch.randint(-8, 9, shape, generator=g).float())
    t[torch.rand(shape, generator=g) < zeros] = 0.0
    return t


def check(got, ref, mag, k, what):
    """|got - ref| <= k u mag elementwise (exact zeros where mag is 0, nothing non-finite); prints the worst ratio"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    ratio = torch.where(mag > 0, err / (U * mag), torch.zeros_like(err))
    print(f"[wino ratio] {what}: {ratio.nan_to_num(nan=float('inf')).max().item():.2f} u of {k} u")
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    bad = ~(err <= k * U * mag)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} beyond {k} u x magnitude, worst "
                           f"{ratio.max().item():.3g} u, first at {tuple(bad.nonzero()[0].tolist())}")


def words_of(V):
    """float bits of max|V[.][t][.]|, one int32 word per tile"""
    return V.abs().amax(dim=(0, 2)).view(torch.int32)


# ------------------------------------------------------------------------------------------------ inputs and references
@functools.lru_cache(maxsize=None)
def input_case(shape):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(1000 * C + 10 * H + W)
    x = rand((B, H, W, C), g)
    x2 = rand((B, H, W, C), g) * 3.0
    gate = torch.randn(B, H, W, C, generator=g)
    flat = gate.view(-1)
    flat[0], flat[1], flat[2], flat[3] = 0.0, -0.0, float("nan"), 0.75
    gscale = torch.randn(C, generator=g)
    closed = ~(gate > 0)
    # every pixel behind a closed gate holds something that a multiplication would not survive
    xbad = x.clone()
    xbad[closed] = torch.tensor([float("inf"), float("-inf"), float("nan")])[torch.arange(int(closed.sum())) % 3]
    xzero = torch.where(closed, torch.zeros_like(x), x)
    return dict(x=x, x2=x2, gate=gate, gscale=gscale, xbad=xbad, xzero=xzero)


@functools.lru_cache(maxsize=None)
def input_ref(shape, m, gated):
    c = input_case(shape)
    if gated == "no":
        return O.wino_input_f64(c["x"], m)
    return O.wino_input_f64(c["xzero"], m, c["gate"], c["gscale"] if gated == "scale" else None)


@functools.lru_cache(maxsize=None)
def input_dev(shape):
    return {k: v.cuda() for k, v in input_case(shape).items()}


# ------------------------------------------------------------------------------------------------ 3a input transform
@shapes
@variants
def test_input_transform_matches_float64(N, shape, variant):
    m, v4 = variant
    B, C, H, W = shape
    d = input_dev(shape)
    ref, mag = input_ref(shape, m, "no")
    V = N.wino_input_transform(cl(d["x"]), m, vec4=v4)
    assert V.shape == ((m + 2) ** 2, O.wino_tiles(B, H, W, m), C) and V.is_contiguous()
    check(V, ref, mag, 2 * (m + 2), f"input m={m} vec4={v4} {shape}")
    assert torch.equal(V, N.wino_input_transform(cl(d["x"]), m, vec4=v4))  # deterministic


@shapes
@variants
def test_input_gate_is_a_select_not_a_multiply(N, shape, variant):
    """gate <= 0 (exact 0, -0.0, negative) or NaN: the pixel contributes 0 whatever x holds there (inf, -inf, NaN)"""
    m, v4 = variant
    d = input_dev(shape)
    for gated in ("scale", "only"):
        ref, mag = input_ref(shape, m, gated)
        V = N.wino_input_transform(cl(d["xbad"]), m, gate=cl(d["gate"]), gate_scale=d["gscale"] if gated == "scale" else None,
                                   vec4=v4)
        check(V, ref, mag, 2 * (m + 2), f"input gate-{gated} m={m} vec4={v4} {shape}")
        V0 = N.wino_input_transform(cl(d["xzero"]), m, gate=cl(d["gate"]), gate_scale=d["gscale"] if gated == "scale" else None,
                                    vec4=v4)
        assert torch.equal(V, V0)  # the same bits as with zeros behind the closed gates


@shapes
@variants
def test_input_channel_slices(N, shape, variant):
    m, v4 = variant
    B, C, H, W = shape
    d = input_dev(shape)
    V = N.wino_input_transform(cl(d["x"]), m, vec4=v4)
    # in: x is channels [4, 4 + C) of a wider buffer whose other channels are NaN
    wide = torch.full((B, H, W, C + 8), float("nan"), device="cuda")
    wide[..., 4:4 + C] = d["x"]
    assert torch.equal(N.wino_input_transform(cl(wide)[:, 4:4 + C], m, vec4=v4), V)
    # out: V is channels [4, 4 + C) of a wider V; the other channels keep their sentinel
    wideV = torch.full((V.shape[0], V.shape[1], C + 8), SENTINEL, device="cuda")
    out = wideV[:, :, 4:4 + C]
    assert N.wino_input_transform(cl(d["x"]), m, vec4=v4, out=out) is out
    assert torch.equal(out, V)
    assert (wideV[:, :, :4] == SENTINEL).all() and (wideV[:, :, 4 + C:] == SENTINEL).all()
    # both at once, with the gate prologue
    Vg = N.wino_input_transform(cl(d["xbad"]), m, gate=cl(d["gate"]), gate_scale=d["gscale"], vec4=v4)
    wide[..., 4:4 + C] = d["xbad"]
    wideV.fill_(SENTINEL)
    N.wino_input_transform(cl(wide)[:, 4:4 + C], m, gate=cl(d["gate"]), gate_scale=d["gscale"], vec4=v4, out=out)
    assert torch.equal(out, Vg)
    assert (wideV[:, :, :4] == SENTINEL).all() and (wideV[:, :, 4 + C:] == SENTINEL).all()


@shapes
@variants
def test_input_scale_words_are_the_tile_maxima(N, shape, variant):
    """the amax entry: V keeps its bits and word t holds exactly the float bits of max|V[.][t][.]|"""
    m, v4 = variant
    B, C, H, W = shape
    d = input_dev(shape)
    T = O.wino_tiles(B, H, W, m)
    for kw in ({}, dict(gate=cl(d["gate"]), gate_scale=d["gscale"])):
        x = cl(d["xbad"] if kw else d["x"])
        V = N.wino_input_transform(x, m, vec4=v4, **kw)
        V1, w1 = N.wino_input_transform(x, m, vec4=v4, amax=True, **kw)
        assert w1.dtype == torch.int32 and w1.shape == (T,)
        assert torch.equal(V1, V)
        assert torch.equal(w1, words_of(V))
        # pre-zeroed words of the caller; the second launch repeats the first bit for bit
        w2 = torch.zeros(T, dtype=torch.int32, device="cuda")
        V2, w2r = N.wino_input_transform(x, m, vec4=v4, amax=w2, **kw)
        assert w2r is w2 and torch.equal(V2, V) and torch.equal(w2, w1)
    # two calls fill two channel slices of one V and share the words: the maximum over both
    Va = N.wino_input_transform(cl(d["x"]), m, vec4=v4)
    Vb, wb = N.wino_input_transform(cl(d["x2"]), m, vec4=v4, amax=True)
    both = torch.full((Va.shape[0], T, 2 * C), SENTINEL, device="cuda")
    words = torch.zeros(T, dtype=torch.int32, device="cuda")
    N.wino_input_transform(cl(d["x"]), m, vec4=v4, amax=words, out=both[:, :, :C])
    assert torch.equal(words, words_of(Va)) and (both[:, :, C:] == SENTINEL).all()
    N.wino_input_transform(cl(d["x2"]), m, vec4=v4, amax=words, out=both[:, :, C:])
    assert torch.equal(both[:, :, :C], Va) and torch.equal(both[:, :, C:], Vb)
    assert torch.equal(words, words_of(both)) and torch.equal(words, torch.maximum(words_of(Va), wb))


@shapes
def test_input_variants_give_the_same_bits(N, shape):
    """F(4,3) with two channels per lane (vec4 = 0) against the shipped four-channel kernel; None is the module default"""
    d = input_dev(shape)
    for kw in ({}, dict(gate=cl(d["gate"]), gate_scale=d["gscale"])):
        x = cl(d["xbad"] if kw else d["x"])
        V0, w0 = N.wino_input_transform(x, 4, vec4=0, amax=True, **kw)
        V1, w1 = N.wino_input_transform(x, 4, vec4=1, amax=True, **kw)
        assert torch.equal(V0, V1) and torch.equal(w0, w1)
        assert torch.equal(N.wino_input_transform(x, 4, **kw), V1)
    assert N.WINO_IN_VEC4 & 1 == 1  # what ships


# ------------------------------------------------------------------------------------------------ 3b filter transform
@pytest.mark.parametrize("m", [2, 4])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("chans", [(1, 1), (3, 5), (8, 12), (64, 32)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_filter_transform_matches_float64(N, chans, flip, m):
    Cout, Cin = chans
    g = torch.Generator().manual_seed(100 * Cout + Cin)
    w = rand((Cout, Cin, 3, 3), g)
    ref, mag = O.wino_filter_f64(w, m, flip)
    Uw = N.wino_filter(w.cuda(), m, flip)
    check(Uw, ref, mag, 2 * (m + 2), f"filter m={m} flip={int(flip)} {chans}")
    assert torch.equal(Uw, N.wino_filter(w.cuda(), m, flip))
    if flip:  # the rotated filters with the channel roles swapped, through the forward layout: the same bits
        assert torch.equal(Uw, N.wino_filter(w.flip(2, 3).transpose(0, 1).contiguous().cuda(), m, False))


# ------------------------------------------------------------------------------------------------ 3c output transform
ALL16_SHAPE = (2, 8, 5, 7)
EPILOGUES = [(s, v, e) for s in SHAPES for v in VARIANTS for e in (range(16) if s == ALL16_SHAPE else (0, 15))]
PARTS = ("addend", "scale", "bias", "relu")


@functools.lru_cache(maxsize=None)
def output_case(shape, m):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(77 * C + 5 * H + W + m)
    M = rand(((m + 2) ** 2, O.wino_tiles(B, H, W, m), C), g)
    addend = rand((B, H, W, C), g) * 4.0
    scale = torch.randn(C, generator=g)
    bias = torch.randn(C, generator=g)
    return M, addend, scale, bias


@functools.lru_cache(maxsize=None)
def output_ref(shape, m, mask):
    B, C, H, W = shape
    M, addend, scale, bias = output_case(shape, m)
    return O.wino_output_f64(M, B, H, W, m, addend if mask & 1 else None, scale if mask & 2 else None,
                             bias if mask & 4 else None, bool(mask & 8))


def run_output(N, shape, m, v4, mask):
    """the output transform into a flat buffer with one image row of sentinel before and after y; returns y (B,H,W,C)"""
    B, C, H, W = shape
    M, addend, scale, bias = (t.cuda() for t in output_case(shape, m))
    guard, n = W * C, B * H * W * C
    buf = torch.full((guard + n + guard,), SENTINEL, device="cuda")
    y = buf[guard:guard + n].view(B, H, W, C)
    r = N.wino_output_transform(M, (B, C, H, W), m, addend=cl(addend) if mask & 1 else None, scale=scale if mask & 2 else None,
                                bias=bias if mask & 4 else None, relu=bool(mask & 8), vec4=v4, out=cl(y))
    assert r.data_ptr() == y.data_ptr()
    # rows and columns beyond H, W belong to no one: a write there lands in the next row, the next image or a guard
    assert (buf[:guard] == SENTINEL).all() and (buf[guard + n:] == SENTINEL).all(), "a sentinel guard was overwritten"
    return y


@pytest.mark.parametrize("shape,variant,mask", EPILOGUES,
                         ids=[f"{ids_shape(s)}-{ids_variant(v)}-" + ("+".join(p for i, p in enumerate(PARTS) if e >> i & 1) or "plain")
                              for s, v, e in EPILOGUES])
def test_output_transform_matches_float64(N, shape, variant, mask):
    m, v4 = variant
    ref, mag = output_ref(shape, m, mask)
    y = run_output(N, shape, m, v4, mask)
    check(y, ref, mag, 2 * (m + 2) + 2, f"output m={m} vec4={v4} {shape} epilogue {mask:04b}")
    assert torch.equal(y, run_output(N, shape, m, v4, mask))


@shapes
def test_output_variants_give_the_same_bits(N, shape):
    B, C, H, W = shape
    for mask in ((0, 15) if shape != ALL16_SHAPE else range(16)):
        y0, y1 = run_output(N, shape, 4, 0, mask), run_output(N, shape, 4, 1, mask)
        assert torch.equal(y0, y1), f"epilogue {mask:04b}"
    # None is the module default (two channels per lane ships), and without `out` the result is a fresh channels_last tensor
    M, addend, scale, bias = (t.cuda() for t in output_case(shape, 4))
    y = N.wino_output_transform(M, (B, C, H, W), 4, addend=cl(addend), scale=scale, bias=bias, relu=True)
    assert y.shape == (B, C, H, W) and N.cl_pixel_stride(y) == C and torch.equal(y, cl(y1))
    assert (N.WINO_IN_VEC4 >> 1) & 1 == 0


# ------------------------------------------------------------------------------------------------ 3d grid-stride wrap
WRAP = (2, 2048, 46, 46)  # m = 2: 529 tiles x 512 groups = 270 848 items per image, 541 696 > 2048 blocks x 256 lanes in the batch


def test_input_transform_grid_stride_wrap(N):
    """the batch wraps the grid-stride loop, a single image does not: same V and scale words, image by image"""
    B, C, H, W = WRAP
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(B, H, W, C, device="cuda", generator=g)
    V, words = N.wino_input_transform(cl(x), 2, amax=True)
    per = V.shape[1] // B
    assert per * (C // 4) <= 2048 * 256 < B * per * (C // 4)
    for b in range(B):
        Vb, wb = N.wino_input_transform(cl(x[b:b + 1]), 2, amax=True)
        assert torch.equal(V[:, b * per:(b + 1) * per], Vb) and torch.equal(words[b * per:(b + 1) * per], wb)
        assert torch.equal(wb, words_of(Vb))


def test_output_transform_grid_stride_wrap(N):
    B, C, H, W = WRAP
    g = torch.Generator(device="cuda").manual_seed(4)
    T = O.wino_tiles(B, H, W, 2)
    per = T // B
    M = torch.randn(16, T, C, device="cuda", generator=g)
    addend = torch.randn(B, H, W, C, device="cuda", generator=g)
    scale, bias = torch.randn(C, device="cuda", generator=g), torch.randn(C, device="cuda", generator=g)
    y = N.wino_output_transform(M, (B, C, H, W), 2, addend=cl(addend), scale=scale, bias=bias, relu=True)
    for b in range(B):
        yb = N.wino_output_transform(M[:, b * per:(b + 1) * per].contiguous(), (1, C, H, W), 2, addend=cl(addend[b:b + 1]),
                                     scale=scale, bias=bias, relu=True)
        assert torch.equal(y[b:b + 1], yb)


# ------------------------------------------------------------------------------------------------ 3e refusals
def test_refusals_write_nothing(N):
    """bad arguments come back as an error of the C entry point (raised as SeaNativeError) before anything is launched"""
    L = N.lib()
    B, C, H, W, m = 1, 8, 4, 4, 2
    T, A2 = 4, 16
    x = torch.randn(B, H, W, C + 8, device="cuda")
    gate = torch.ones(B, H, W, C + 8, device="cuda")
    V = torch.full((A2 * T * (C + 8) + 8,), SENTINEL, device="cuda")
    y = torch.full((B * H * W * C + 8,), SENTINEL, device="cuda")
    Mx = torch.randn(A2 * T * C + 8, device="cuda")
    words = torch.zeros(T, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    px, pv, pg, py, pm, pw = (t.data_ptr() for t in (x, V, gate, y, Mx, words))

    def inp(x=px, xps=C, gate=None, V=pv, vts=C, C=C, m=m, vec4=1):
        return L.sea_wino_input_transform(x, xps, gate, None, V, vts, B, C, H, W, m, vec4, st)

    def inp_amax(amax, **kw):
        a = dict(x=px, xps=C, gate=None, V=pv, vts=C, C=C, m=m, vec4=1)
        a.update(kw)
        return L.sea_wino_input_transform_amax(a["x"], a["xps"], a["gate"], None, a["V"], a["vts"], B, a["C"], H, W, a["m"],
                                               a["vec4"], amax, st)

    def out(M=pm, addend=None, y=py, C=C, m=m, vec4=0):
        return L.sea_wino_output_transform(M, addend, None, None, 0, y, B, C, H, W, m, vec4, st)

    refused = {
        "C % 4 != 0": lambda: inp(C=6, xps=8, vts=8),
        "x_pixel_stride < C": lambda: inp(xps=C - 4),
        "x_pixel_stride % 4 != 0": lambda: inp(xps=C + 2),
        "v_tile_stride < C": lambda: inp(vts=C - 4),
        "v_tile_stride % 4 != 0": lambda: inp(vts=C + 2),
        "m = 3": lambda: inp(m=3),
        "m = 3, F(4,3) kernels": lambda: inp(m=3, vec4=0),
        "x offset by 4 bytes": lambda: inp(x=px + 4),
        "V offset by 4 bytes": lambda: inp(V=pv + 4),
        "gate offset by 4 bytes": lambda: inp(gate=pg + 4),
        "x NULL": lambda: inp(x=None),
        "V NULL": lambda: inp(V=None),
        "amax NULL on the amax entry": lambda: inp_amax(None),
        "amax entry, C % 4 != 0": lambda: inp_amax(pw, C=6, xps=8, vts=8),
        "amax entry, V offset by 4 bytes": lambda: inp_amax(pw, V=pv + 4),
        "amax entry, m = 3": lambda: inp_amax(pw, m=3),
        "output, C % 4 != 0": lambda: out(C=6),
        "output, m = 3": lambda: out(m=3),
        "output, M offset by 4 bytes": lambda: out(M=pm + 4),
        "output, y offset by 4 bytes": lambda: out(y=py + 4),
        "output, addend offset by 4 bytes": lambda: out(addend=px + 4),
        "output, y NULL": lambda: out(y=None),
    }
    for what, call in refused.items():
        rc = call()
        assert rc != 0, what
        with pytest.raises(N.SeaNativeError):
            N._check(rc, what)
    torch.cuda.synchronize()
    assert (V == SENTINEL).all() and (y == SENTINEL).all() and (words == 0).all()
    # the same arguments, made valid, are accepted (the refusals above are not an entry point that refuses everything)
    assert inp(xps=C + 8, gate=None, vts=C + 8) == 0 and inp_amax(pw) == 0 and out() == 0
    torch.cuda.synchronize()
    assert not (V == SENTINEL).all() and not (y == SENTINEL).all() and (words != 0).any()
    # ... and through the wrappers
    ok = torch.randn(1, 4, 4, 8, device="cuda")
    sent = torch.full((16, 4, 8), SENTINEL, device="cuda")
    for bad in (lambda: N.wino_input_transform(cl(torch.randn(1, 4, 4, 6, device="cuda")), 2),
                lambda: N.wino_input_transform(cl(ok), 3, out=sent),
                lambda: N.wino_input_transform(cl(ok), 2, out=sent[:, :, :4]),
                lambda: N.wino_input_transform(cl(ok), 2, out=sent[:, :2]),
                lambda: N.wino_input_transform(ok, 2, out=sent),  # NCHW memory
                lambda: N.wino_input_transform(cl(ok), 2, gate=cl(x)[:, :8], out=sent),  # gate must be dense
                lambda: N.wino_input_transform(cl(ok), 2, amax=torch.zeros(3, dtype=torch.int32, device="cuda"), out=sent),
                lambda: N.wino_input_transform(cl(ok), 2, amax=torch.zeros(4, device="cuda"), out=sent),
                lambda: N.wino_output_transform(sent, (1, 8, 4, 4), 3),
                lambda: N.wino_output_transform(sent, (1, 8, 4, 5), 2),
                lambda: N.wino_output_transform(sent, (1, 8, 4, 4), 2, out=ok),
                lambda: N.wino_output_transform(sent, (1, 8, 4, 4), 2, addend=ok)):
        with pytest.raises(N.SeaNativeError):
            bad()
    assert (sent == SENTINEL).all()


def test_tile_count(N):
    L = N.lib()
    for m in (2, 4):
        for B, H, W in [(1, 1, 1), (3, 2, 3), (2, 5, 7), (1, 9, 6), (2, 46, 46), (8, 128, 128), (1, 4, 8)]:
            assert L.sea_wino_tiles(B, H, W, m) == B * -(-H // m) * -(-W // m) == O.wino_tiles(B, H, W, m)
    for bad in [(0, 4, 4, 2), (1, 0, 4, 2), (1, 4, 0, 4), (1, 4, 4, 3), (1, 4, 4, 0), (-1, 4, 4, 2), (1, 4, 4, 6)]:
        assert L.sea_wino_tiles(*bad) == 0


# ------------------------------------------------------------------------------------------------ 3f end to end
def test_scale_words_consumed_by_the_matrix_core_products(N, monkeypatch):
    """wino_conv3x3_cl(gemm_terms=22) at the smallest shape that takes the matrix-core path with ragged tiles: 16 tiles per
    image (= WINO_SPLIT_MIN_TILES), 1 pixel of ragged edge; plain, with gate / gate_scale, and with one tile gated off
    entirely (scale word 0).  Yardstick of test_winograd_products_on_the_matrix_cores: error <= 2 x the fp32-bmm Winograd path's
    own error + 1e-6, relative to max|y|, both against float64 conv2d."""
    B, Cin, Cout, H, W, m = 2, 32, 8, 13, 13, 4
    assert O.wino_tiles(1, H, W, m) == N.WINO_SPLIT_MIN_TILES == 16 and N.AMAX_FROM_PRODUCERS
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(B, H, W, Cin, generator=g) * 3).cuda()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)).cuda()
    gate = torch.randn(B, H, W, Cin, generator=g).cuda()
    gscale = (torch.rand(Cin, generator=g) + 0.5).cuda()
    gate_off = gate.clone()
    gate_off[0, 3:9, 3:9] = -1.0  # the whole 6 x 6 patch of tile (b 0, ty 1, tx 1)
    t_off = 1 * 4 + 1
    Uw = N.wino_filter(w, m, False)
    calls = []
    real = N.wino_input_transform

    def spy(*a, **kw):
        calls.append(kw.get("amax") is not None)
        return real(*a, **kw)

    monkeypatch.setattr(N, "wino_input_transform", spy)
    for what, gt, gs in (("plain", None, None), ("gate", gate, gscale), ("gate only", gate, None), ("tile gated off", gate_off, gscale)):
        xin = x.double()
        if gt is not None:
            xin = torch.where(gt > 0, xin * (gs.double() if gs is not None else 1.0), torch.zeros_like(xin))
        ref = torch.nn.functional.conv2d(cl(xin), w.double(), padding=1)
        kw = dict(gate=None if gt is None else cl(gt), gate_scale=gs)
        del calls[:]
        y0 = N.wino_conv3x3_cl(cl(x), Uw, m, **kw)
        assert calls == [False]
        y1 = N.wino_conv3x3_cl(cl(x), Uw, m, gemm_terms=22, **kw)
        assert calls == [False, True], "the amax entry did not run"
        e0 = (y0.double() - ref).abs().max().item() / ref.abs().max().item()
        e1 = (y1.double() - ref).abs().max().item() / ref.abs().max().item()
        print(f"[wino e2e] {what}: max err / max|y| vs float64 conv2d: fp32 GEMM {e0:.2e}, fp16 x 2 {e1:.2e}")
        assert torch.isfinite(y1).all() and e1 <= 2.0 * e0 + 1e-6, (what, e0, e1)
    V, words = real(cl(x), m, gate=cl(gate_off), gate_scale=gscale, amax=True)
    assert (V[:, t_off] == 0).all() and words[t_off] == 0  # the gated-off tile contributes exactly 0
    assert (words[:t_off] != 0).all() and (words[t_off + 1:] != 0).all() and torch.equal(words, words_of(V))
