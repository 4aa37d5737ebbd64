"""K2 without gradient (sea_loss_fwd_bwd with dlogits = NULL): every evaluation kernel against a float64 reference.

Every accuracy and mIoU figure goes through these kernels, and which one runs depends on shape, dtype, layout and
alignment, so the same integers and the same losses are asked of all of them.  The reference is
oracle.sea_oracle.loss_eval_f64 (pinned on the CPU by tests/test_loss_nograd_ref_cpu.py): float64 from the logits as given
-- a 16-bit tensor is its own rounded input --, labels outside [0, C) ignored, torch.max's index (first NaN, else first
maximum).  Inputs follow test_kernels_gpu._rand_case (randn * 3, +6 on the label class at 70 % of the pixels, exact
two-class ties at 2 %, 5 % ignored) plus ~1 % labels equal to C or C + 3 where the label type holds them.

Bars (head of test_kernels_gpu.py and its golden test): pred and n_correct exact; loss_sum / HW and track_sum / HW
rtol 3e-5, atol 1e-6; loss_px rtol 2e-5, atol 2e-6; the same for 16-bit logits (the kernels compute in fp32 from the same
rounded inputs).  Every launch runs twice and the two results are equal bit for bit (fixed-order reductions).

Which kernel a case reaches (loss_plan of csrc/loss_plan.h; tests/test_loss_plan_cpu.py pins these rows without a device;
force_vec is a word of _native.k2_variant).  "even" = 48 x 52 = 2496 pixels, a multiple of 8: three tiles of 1024 pixels at four pixels per lane,
two of 2048 at eight, the last one ragged; "odd" = 47 x 53 = 2491 pixels: one pixel per lane, no 16-byte plane alignment.

  layout  H*W   C / force_vec                      kernel
  ------  ----  ---------------------------------  -----------------------------------------------------------------------
  NCHW    even  C > 32, force_vec 0                loss_nchw_fwd<T, 4, 5|4>  (streaming, CH = 4)
  NCHW    even  any C, force_vec = v << 8          loss_nchw_fwd<T, CH, .>, CH = 4, 8, 6, 2 for v = 1, 2, 3, 4
  NCHW    even  C <= 32, force_vec 0 | 4           loss_nchw_reg<T, CPAD, 4, false, C == CPAD>, CPAD = 8, 16, 19, 21, 24, 32
                                                   (fp32 C = 21, force_vec 0: the TUNE = 6 instantiation)
  NCHW    even  C <= 64, force_vec 2               loss_nchw_reg<T, CPAD, 2, false, .>
  NCHW    even  C <= 192, force_vec 1              loss_nchw_reg<T, CPAD, 1, false, .>
  NCHW    odd   C <= 192                           loss_nchw_reg<T, CPAD, 1, false, .>, CPAD = 8 ... 32, 48, 64, 96, 128, 150,
                                                   151, 160, 192  (C = 60 -> 64, 100 -> 128, 171 -> 192)
  NCHW    odd   C > 192                            loss_nchw_stream<T, false>  (two-pass fallback)
  NHWC    any   C <= 159                           loss_nhwc_lds<T, false>
  NHWC    any   C >= 160                           wrapper: NCHW copy, rows above; C entry: SEA_ERR_ARG, nothing written

Chunk loop of loss_nchw_fwd (nfull = C / CH full chunks, ntail = C % CH; two chunks per trip, buffers A and B):
  exit 1  nfull odd,  no tail      last full chunk reduced from A
  exit 2  nfull odd,  tail         tail loaded into B
  exit 3  nfull even, no tail      loop ends with both buffers consumed
  exit 4  nfull even, tail         tail loaded into A inside the last trip (nfull == 0: loaded in the final branch)

Two deliberate mistakes in loss_nchw_fwd, tried once on a scratch build, and what they trip:
  `z > mm` -> `z >= mm` (last maximum instead of first): 49 cases -- every streaming case whose input holds ties
      (chunk_loop_exits 33 ... 171, variants at C = 5, 21, 37, all of mode_pairs, types, no_class_weights at C = 40, masked
      classes, the deferred reduction, the register-vs-streaming comparison) and non_finite_logits[streaming*];
  the final `else if (ntail)` branch without its reduce_chunk: exactly the eleven exit-4 cases -- chunk_loop_exits[33, 171],
      variants[2-5, 2-21, 2-37, 2-151, 3-5, 3-37, 4-5, 4-21, 4-37].
"""
import functools

import pytest
import torch

from oracle import sea_oracle as O

pytestmark = pytest.mark.gpu

SUM_TOL = dict(rtol=3e-5, atol=1e-6)
PX_TOL = dict(rtol=2e-5, atol=2e-6)
EVEN, ODD = (48, 52), (47, 53)
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
I64, I32, I16, U8 = torch.int64, torch.int32, torch.int16, torch.uint8
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def N():
    from semseg import _native
    _native.lib()  # raises if the extension is missing: no silent fallback
    return _native


# ------------------------------------------------------------------------------------------------ inputs and reference
def _labels_as(y, dtype):
    """int64 labels with -1 = ignored -> the label type handed to the kernel (uint8: 255 = ignored)"""
    if dtype == U8:
        return torch.where(y < 0, torch.full_like(y, 255), y).to(U8)
    return y.to(dtype)


@functools.lru_cache(maxsize=None)
def _case(B, C, hw, seed, dtype=F32, ydtype=I64, masked=False):
    """test_kernels_gpu._rand_case's recipe + out-of-range labels; ``masked``: classes 0..7 are -inf on every pixel and so
    are a scattered 10 % of the other logits, never the label's own"""
    H, W = hw
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, H, W, generator=g) * 3
    y = torch.randint(8 if masked else 0, C, (B, H, W), generator=g)
    boost = (torch.rand(B, H, W, generator=g) < 0.7).float() * 6
    logits.scatter_add_(1, y.unsqueeze(1), boost.unsqueeze(1))
    tie = torch.rand(B, H, W, generator=g) < 0.02
    lo = 8 if masked else 0
    logits[:, lo + 1][tie] = logits[:, lo][tie]
    if masked:
        logits[:, :8] = -INF
        scat = torch.rand(B, C, H, W, generator=g) < 0.1
        scat.scatter_(1, y.unsqueeze(1), False)
        logits[scat] = -INF
    y[torch.rand(B, H, W, generator=g) < 0.05] = -1
    oob = torch.rand(B, H, W, generator=g) < 0.01
    big = torch.where(torch.rand(B, H, W, generator=g) < 0.5, torch.full_like(y, C), torch.full_like(y, C + 3))
    if ydtype == U8:
        oob &= big <= 255          # (255 itself is the ignore value of a uint8 map)
    y = torch.where(oob, big, y)
    w = torch.rand(C, generator=g) + 0.01
    return logits.to(dtype), _labels_as(y, ydtype), w


@functools.lru_cache(maxsize=None)
def _ref(key, mode, tmode):
    logits, y, w = _case(*key)
    return O.loss_eval_f64(logits, y, w, mode, tmode)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _run(N, logits, y, w, mode, tmode, pred_dtype=I64, force_vec=0, channels_last=False, want_grad=False):
    """two launches on the same device buffers; outputs pre-filled (a pixel the kernel skips shows), the second equal to
    the first bit for bit"""
    B, C, H, W = logits.shape
    ld = logits.cuda()
    if channels_last:
        ld = ld.contiguous(memory_format=torch.channels_last)
    yd, wd = y.cuda(), None if w is None else w.cuda()
    outs = []
    for _ in range(2):
        pred = torch.full((B, H, W), 255 if pred_dtype == U8 else -1, dtype=pred_dtype, device="cuda")
        lpx = torch.full((B, H, W), NAN, device="cuda")
        r = N.loss_fwd_bwd(ld, yd, wd, mode, tmode, 1.0 / (H * W), want_grad=want_grad, pred=pred, loss_px=lpx,
                           force_vec=force_vec)
        torch.cuda.synchronize()
        outs.append(dict(pred=pred.cpu(), loss_px=lpx.cpu(), loss_sum=r["loss_sum"].cpu(), track_sum=r["track_sum"].cpu(),
                         n_correct=r["n_correct"].cpu()))
    for k in outs[0]:
        assert torch.equal(_bits(outs[0][k]), _bits(outs[1][k])), f"{k}: second run differs from the first"
    return outs[0]


def _worst(got, ref, rtol, atol):
    return ((got - ref).abs() / (atol + rtol * ref.abs())).max().item() if got.numel() else 0.0


def _check(got, ref, HW, images=None, ints_of=None, tag=""):
    """``images``: the images whose floats are asserted (all by default); ``ints_of``: those whose integers are"""
    fl = list(range(got["pred"].shape[0])) if images is None else list(images)
    it = fl if ints_of is None else list(ints_of)
    sums = {k: (got[k].double()[fl] / HW, ref[k][fl] / HW) for k in ("loss_sum", "track_sum")}
    px = (got["loss_px"].double()[fl], ref["loss_px"][fl])
    used = dict(loss_px=_worst(*px, **PX_TOL), **{k: _worst(*v, **SUM_TOL) for k, v in sums.items()})
    if not max(used.values()) <= 1.0:      # (figures for a bar that is missed: NaN included)
        print(f"[k2 no-grad] {tag}: fraction of the bar used: " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    assert torch.equal(got["pred"].long()[it], ref["pred"][it])
    assert torch.equal(got["n_correct"].long()[it], ref["n_correct"][it])
    for k, (g, r) in sums.items():
        assert torch.isfinite(g).all(), k
        torch.testing.assert_close(g, r, **SUM_TOL)
    assert torch.isfinite(px[0]).all()
    torch.testing.assert_close(*px, **PX_TOL)


def _go(N, key, mode=1, tmode=3, use_w=True, **kw):
    logits, y, w = _case(*key)
    got = _run(N, logits, y, w if use_w else None, mode, tmode, **kw)
    _check(got, _ref(key, mode, tmode), key[2][0] * key[2][1], tag=f"{key[1:]} {mode}/{tmode} {kw}")
    return got


# ------------------------------------------------------------------------------------------------ 1-3 streaming kernel
@pytest.mark.parametrize("C", [33, 36, 40, 150, 151, 171, 200, 255, 300])
def test_streaming_kernel_chunk_loop_exits(N, C):
    """loss_nchw_fwd<float, CH = 4>, fp32, mode 1 / track 3.  Branches by C (nfull = C / 4, ntail = C % 4):
      C =  33  nfull  8 even, tail 1   exit 4 (tail in buffer A, loaded in the loop's last trip)
      C =  36  nfull  9 odd,  no tail  exit 1
      C =  40  nfull 10 even, no tail  exit 3
      C = 150  nfull 37 odd,  tail 2   exit 2 (tail in buffer B)
      C = 151  nfull 37 odd,  tail 3   exit 2
      C = 171  nfull 42 even, tail 3   exit 4
      C = 200  nfull 50 even, no tail  exit 3
      C = 255  nfull 63 odd,  tail 3   exit 2; uint8 labels and uint8 pred: 254 is the last class, 255 is "ignored"
      C = 300  nfull 75 odd,  no tail  exit 1; int16 labels and int16 pred
    A change of CH moves these: re-derive the list with it."""
    yd = {255: U8, 300: I16}.get(C, I64)
    _go(N, (2, C, EVEN, 100 + C, F32, yd), pred_dtype=yd)


@pytest.mark.parametrize("C", [5, 21, 37, 151])
@pytest.mark.parametrize("v", [1, 2, 3, 4])
def test_streaming_kernel_variants(N, v, C):
    """force_vec = v << 8: CH = 4, 8, 6, 2; bits 8..11 also send C <= 32 to the streaming kernel.  (nfull, ntail):
      C =   5   CH 4: (1, 1) exit 2    CH 8: (0, 5) exit 4, nfull == 0    CH 6: (0, 5) exit 4, nfull == 0    CH 2: (2, 1) exit 4
      C =  21   CH 4: (5, 1) exit 2    CH 8: (2, 5) exit 4                CH 6: (3, 3) exit 2                CH 2: (10, 1) exit 4
      C =  37   CH 4: (9, 1) exit 2    CH 8: (4, 5) exit 4                CH 6: (6, 1) exit 4                CH 2: (18, 1) exit 4
      C = 151   CH 4: (37, 3) exit 2   CH 8: (18, 7) exit 4               CH 6: (25, 1) exit 2               CH 2: (75, 1) exit 2
    Where variant 0 streams as well (C > 32) the integers equal its integers; the floats meet the bars against the
    reference (another CH is another summation order)."""
    key = (2, C, EVEN, 200 + C, F32, I64)
    got = _go(N, key, force_vec=v << 8)
    if C > 32:
        base = _go(N, key)
        assert torch.equal(got["pred"], base["pred"]) and torch.equal(got["n_correct"], base["n_correct"])


@pytest.mark.parametrize("dtype,ydtype,pdtype", [(F32, I32, I16), (F32, U8, I32), (BF16, I64, U8), (BF16, I16, I64),
                                                 (F16, I64, I32), (F16, U8, I16), (F16, I16, U8)])
def test_streaming_kernel_types(N, dtype, ydtype, pdtype):
    """logit type x label width x pred width at C = 151 (16-bit logits: eight pixels per lane, two tiles)"""
    _go(N, (2, 151, EVEN, 31, dtype, ydtype), mode=0, tmode=2, pred_dtype=pdtype)


@pytest.mark.parametrize("tmode", [0, 1, 2, 3])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_streaming_kernel_mode_pairs(N, mode, tmode):
    _go(N, (2, 40, EVEN, 140, F32, I64), mode=mode, tmode=tmode)


@pytest.mark.parametrize("mode,tmode", [(0, 3), (2, 0), (3, 2), (3, 3)])
@pytest.mark.parametrize("C", [21, 40])
def test_no_class_weights_where_no_mode_needs_them(N, C, mode, tmode):
    _go(N, (2, C, EVEN, 140 if C == 40 else 321, F32, I64), mode=mode, tmode=tmode, use_w=False)


# ------------------------------------------------------------------------------------------------ 4-5 register kernels, C > 192
@pytest.mark.parametrize("fv", [0, 1, 2])
@pytest.mark.parametrize("C", [2, 8, 9, 16, 19, 21, 24, 27, 32])
def test_register_kernel_small_class_counts(N, C, fv):
    """loss_nchw_reg<float, CPAD, VEC, false, C == CPAD> at 48 x 52: VEC = 4 (force_vec 0), 1, 2; CPAD = 8 (C = 2, 8),
    16 (9, 16), 19, 21, 24, 32 (27, 32)"""
    _go(N, (2, C, EVEN, 300 + C, F32, I64), force_vec=fv)


@pytest.mark.parametrize("C,dtype,fv", [(21, F32, 4), (21, BF16, 0), (19, F16, 0), (27, BF16, 0), (21, F16, 2)])
def test_register_kernel_plain_and_16bit_instantiations(N, C, dtype, fv):
    """force_vec 4 reaches the plain loss_nchw_reg<float, 21, 4, false, true> (force_vec 0 takes its TUNE = 6 twin); 16-bit
    logits at 48 x 52 with C <= 32 run the register kernel at four pixels per lane (force_vec 2: at two)"""
    _go(N, (2, C, EVEN, 300 + C, dtype, I64), force_vec=fv)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("C", [19, 21, 60, 100, 150, 151, 171])
def test_register_kernel_odd_image(N, C, dtype):
    """47 x 53: one pixel per lane and no streaming kernel; CPAD = 19, 21, 64, 128, 150, 151, 192"""
    _go(N, (2, C, ODD, 400 + C, dtype, I64))


def test_register_kernel_where_the_streaming_one_would_run(N):
    key = (2, 151, EVEN, 251, F32, I64)         # (the case of test_streaming_kernel_chunk_loop_exits[151])
    reg, stream = _go(N, key, force_vec=1), _go(N, key)
    assert torch.equal(reg["pred"], stream["pred"]) and torch.equal(reg["n_correct"], stream["n_correct"])


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_two_pass_kernel_beyond_192_classes(N, dtype):
    """loss_nchw_stream<T, false>: C = 200 at 47 x 53"""
    _go(N, (2, 200, ODD, 600, dtype, I64))


# ------------------------------------------------------------------------------------------------ 6 channels_last
@pytest.mark.parametrize("hw", [EVEN, ODD])
@pytest.mark.parametrize("dtype", [F32, BF16, F16])
@pytest.mark.parametrize("C", [5, 21, 151, 159])
def test_channels_last(N, C, dtype, hw):
    """loss_nhwc_lds<T, false>; C = 159 is the widest row the 160 KB of LDS hold"""
    logits, _, _ = _case(2, C, hw, 700 + C, dtype, I64)
    assert N.logits_layout(logits.cuda().contiguous(memory_format=torch.channels_last))[1] == N.LAYOUT_NHWC
    _go(N, (2, C, hw, 700 + C, dtype, I64), channels_last=True)


def test_channels_last_one_byte_labels_and_pred(N):
    _go(N, (2, 151, EVEN, 851, F32, U8), mode=2, tmode=1, pred_dtype=U8, channels_last=True)


def test_channels_last_160_classes_through_the_wrapper(N):
    """logits_layout falls back to an NCHW copy: the same answer (from the streaming kernel)"""
    logits, _, _ = _case(2, 160, EVEN, 860, F32, I64)
    assert N.logits_layout(logits.cuda().contiguous(memory_format=torch.channels_last))[1] == N.LAYOUT_NCHW
    _go(N, (2, 160, EVEN, 860, F32, I64), channels_last=True)


def test_channels_last_160_classes_entry_point_rejects(N):
    """the C entry with layout = 1 and C = 160 returns 1 (invalid argument) and writes nothing"""
    logits, y, _ = _case(2, 160, EVEN, 860, F32, I64)
    B, C, (H, W) = 2, 160, EVEN
    ld = logits.cuda().permute(0, 2, 3, 1).contiguous()          # (B, H, W, C) in memory
    yd = y.cuda()
    pred = torch.full((B, H, W), -7, dtype=I64, device="cuda")
    lpx = torch.full((B, H, W), -7.0, device="cuda")
    sums = [torch.full((B,), -7.0, device="cuda"), torch.full((B,), -7.0, device="cuda"),
            torch.full((B,), -7, dtype=I32, device="cuda")]
    ws = N.loss_workspace(B, H * W, "cuda")
    rc = N.lib().sea_loss_fwd_bwd(ld.data_ptr(), N.DTYPE_CODE[F32], N.LAYOUT_NHWC, yd.data_ptr(), 8, None, 3, 3, B, C, H * W,
                                  1.0, None, pred.data_ptr(), 8, lpx.data_ptr(), ws.data_ptr(), ws.numel(),
                                  sums[0].data_ptr(), sums[1].data_ptr(), sums[2].data_ptr(), N._stream())
    torch.cuda.synchronize()
    assert rc == 1
    assert (pred == -7).all() and (lpx == -7).all() and all((s == -7).all() for s in sums)


# ------------------------------------------------------------------------------------------------ 7 masked classes
FIVE = [  # name, C, image, dtype, channels_last, force_vec
    ("streaming", 151, EVEN, F32, False, 0),
    ("streaming-16bit", 40, EVEN, BF16, False, 0),
    ("register-4px", 21, EVEN, F32, False, 0),
    ("register-1px", 151, ODD, F32, False, 0),
    ("two-pass", 200, ODD, F32, False, 0),
    ("channels-last", 21, EVEN, F32, True, 0),
]


@pytest.mark.parametrize("name,C,hw,dtype,cl,fv", FIVE, ids=[f[0] for f in FIVE])
def test_masked_classes_give_finite_results(N, name, C, hw, dtype, cl, fv):
    """classes 0..7 = -inf on every pixel (two whole leading chunks of the streaming kernel: its running maximum stays
    -inf) and 10 % of the other logits; the label's logit is finite on every valid pixel, so every output is finite"""
    key = (2, C, hw, 900 + C, dtype, I64, True)
    logits = _case(*key)[0]
    assert torch.isinf(logits[:, :8]).all() and 0.05 < torch.isinf(logits[:, 8:]).float().mean() < 0.15
    for mode, tmode in ((1, 3), (2, 0)):
        _go(N, key, mode=mode, tmode=tmode, channels_last=cl, force_vec=fv)


# ------------------------------------------------------------------------------------------------ 8 non-finite logits
ROWS = ([1, NAN, 5, NAN], [INF, 2, INF, 0], [-INF] * 4, [NAN, INF, 1, 2], [1, INF, NAN, INF], [-INF, 3, 3, -INF])


def _row_classes(C):
    """the four classes that carry a row's values: for C = 151 the second and the third sit in different halves of
    loss_nchw_split's class vector (76 + 75) and in different chunks of the streaming kernel"""
    return [C // 5, C // 2 - 1, C // 2 + 2, C - 1] if C >= 12 else [0, 1, 2, 3]


@functools.lru_cache(maxsize=None)
def _nonfinite_case(C, hw, dtype):
    """B = 3; image 1 carries the six rows (tests/test_loss_nograd_ref_cpu.py pins their indices 1, 0, 0, 0, 2, 1): a NaN
    before and after the finite maximum, +inf twice, all -inf, NaN before +inf, +inf before NaN, ties next to -inf.  Each row
    at each of the eight positions of a lane's pixel vector, in three runs of 48 pixels that start in the tiles [0, 1024),
    [1024, 2048) and [2048, HW) -- three tiles at four pixels per lane, both tiles at eight.  Half of those pixels are
    labelled with the expected index, so n_correct sees it too."""
    logits, y, w = _case(3, C, hw, 1000 + C, F32, I64)
    logits, y = logits.clone(), y.clone()
    H, W = hw
    cls = _row_classes(C)
    z1, y1 = logits[1].view(C, H * W), y[1].view(H * W)
    for base in (0, 1024 + 8, 2048 + 16):
        for j in range(48):
            p, r = base + j, (j // 8) % 6
            col = z1[:, p].clamp(max=2.0)          # the row's 5 and 3 stay the finite maxima
            if r == 2:
                col[:] = -INF
            else:
                col[cls] = torch.tensor(ROWS[r])
            z1[:, p] = col
            if j % 2 == 0:
                y1[p] = int(col.to(dtype).max(0)[1])
    return logits.to(dtype), y, w


NONFINITE = [  # name, C, image, dtype, channels_last, want_grad
    ("streaming", 151, EVEN, F32, False, False),
    ("streaming-16bit", 151, EVEN, BF16, False, False),
    ("register-4px", 21, EVEN, F32, False, False),
    ("register-1px", 151, ODD, F32, False, False),
    ("two-pass", 200, ODD, F32, False, False),
    ("channels-last", 21, EVEN, F32, True, False),
    ("grad-register", 21, EVEN, F32, False, True),
    ("grad-register-16bit", 21, EVEN, F16, False, True),
    ("grad-split", 151, EVEN, F32, False, True),
    ("grad-split-16bit", 151, EVEN, BF16, False, True),
    ("grad-channels-last", 21, EVEN, F32, True, True),
]


@pytest.mark.parametrize("name,C,hw,dtype,cl,grad", NONFINITE, ids=[f[0] for f in NONFINITE])
def test_non_finite_logits(N, name, C, hw, dtype, cl, grad):
    """pred and n_correct of the image with NaN / +inf / -inf logits follow torch.max (the first NaN, else the first
    maximum); the two images that share the launch keep finite sums inside the bars.  The float sums of the image with
    non-finite logits are not asserted: the header promises nothing for them."""
    logits, y, w = _nonfinite_case(C, hw, dtype)
    ref = O.loss_eval_f64(logits, y, w, 1, 3)
    special = ~torch.isfinite(logits[1].float()).all(0)
    assert int(special.sum()) == 3 * 48 and 0 < int(ref["n_correct"][1])
    assert sorted(set(ref["pred"][1][special].tolist())) == sorted({_row_classes(C)[i] for i in (0, 1, 2)} | {0})
    got = _run(N, logits, y, w, 1, 3, channels_last=cl, want_grad=grad)
    _check(got, ref, hw[0] * hw[1], images=(0, 2), ints_of=(0, 1, 2), tag=name)


def _bilinear_taps(n_in, n_out):
    """ATen's align_corners=False source index rule in float32 (what K2u restates)"""
    r = torch.tensor(float(n_in)) / torch.tensor(float(n_out))
    src = (r * (torch.arange(n_out, dtype=torch.float32) + 0.5) - 0.5).clamp(min=0)
    i0 = src.floor().long().clamp(max=n_in - 1)
    return i0, (i0 + 1).clamp(max=n_in - 1), src - i0.float()


@pytest.mark.parametrize("row", range(6))
@pytest.mark.parametrize("pow2", [True, False], ids=["lanes-along-classes", "gather"])
def test_non_finite_logits_fused_upsample(N, pow2, row):
    """K2u, both kernels (x4: the power-of-two kernel, or the general gather kernel with pow2 = False), gradient on.  The
    non-finite values sit in the LOW-resolution logits of image 1.  Interpolating between a non-finite and another pixel
    gives values that depend on the order of the arithmetic (inf - inf, 0 * inf), so pred is compared only at
    full-resolution pixels whose four source taps are all finite -- and, as in test_fused_upsample_loss_kernel, whose top-2
    margin exceeds float noise -- or are one and the same non-finite pixel.  Under ATen's tap rule (i1 = min(i0 + 1, n - 1))
    that is the bottom-right corner alone: at the top and left edges the second tap is the neighbour, with weight 0.  There
    the interpolation is ATen's expression (1 - l) * v + l * v with 0 < l < 1, evaluated here in float32 tap by tap; each of
    the six rows is placed there in turn and must give its index (1, 0, 0, 0, 2, 1 of the row's four classes).  Three more
    rows sit in the other corners and three non-finite pixels inside: they are never compared, they only must not disturb
    their neighbours.  The other pixels of image 1 are labelled "ignored", so n_correct counts the compared pixels only.
    Images 0 and 2 keep K2u's own bars."""
    B, C, h, wl, H, W = 3, 21, 12, 13, 48, 52
    g = torch.Generator().manual_seed(77)
    low = torch.randn(B, C, h, wl, generator=g) * 3
    cls = _row_classes(C)
    for (i, j), r in zip(((0, 0), (0, wl - 1), (h - 1, 0), (h - 1, wl - 1)), (0, 1, 4, row)):
        low[1, :, i, j] = low[1, :, i, j].clamp(max=2.0)
        if r == 2:
            low[1, :, i, j] = -INF
        else:
            low[1, cls, i, j] = torch.tensor(ROWS[r])
    low[1, :, 5, 5] = -INF
    low[1, 3, 7, 3] = NAN
    low[1, 9, 3, 8] = INF
    (y0, y1, ly), (x0, x1, lx) = _bilinear_taps(h, H), _bilinear_taps(wl, W)
    tap = lambda a, b: low[:, :, a][:, :, :, b]  # noqa: E731
    ly, lx = ly.view(1, 1, H, 1), lx.view(1, 1, 1, W)
    hi = (1 - ly) * ((1 - lx) * tap(y0, x0) + lx * tap(y0, x1)) + ly * ((1 - lx) * tap(y1, x0) + lx * tap(y1, x1))
    fin = torch.isfinite(low).all(1)                                              # (B, h, wl)
    fin4 = fin[:, y0][:, :, x0] & fin[:, y0][:, :, x1] & fin[:, y1][:, :, x0] & fin[:, y1][:, :, x1]
    same = ((y0 == y1).view(H, 1) & (x0 == x1).view(1, W)).expand(B, H, W)
    top2 = torch.where(torch.isfinite(hi), hi, torch.zeros_like(hi)).topk(2, dim=1)[0]
    compare = (fin4 & ((top2[:, 0] - top2[:, 1]) > 1e-4)) | (same & ~fin4)
    corner = (same & ~fin4)[1]
    assert int(corner.sum()) == 4 and corner[-2:, -2:].all() and not (same & ~fin4)[[0, 2]].any()
    assert (hi[1].max(0)[1][corner] == [cls[1], cls[0], 0, cls[0], cls[2], cls[1]][row]).all()
    y = hi.max(1)[1]
    flip = torch.rand(B, H, W, generator=g) < 0.3
    y[flip] = torch.randint(0, C, (int(flip.sum()),), generator=g)
    y[1][~compare[1]] = -1
    wts = torch.rand(C, generator=g) + 0.01
    ref1 = O.loss_eval_f64(hi[1:2], y[1:2], wts, 1, 3)
    outs = []
    for _ in range(2):
        pred = torch.full((B, H, W), -1, dtype=I64, device="cuda")
        r = N.loss_fwd_bwd_upsampled(low.cuda(), y.cuda(), wts.cuda(), 1, 3, 1.0 / (H * W), want_grad=True, pred=pred,
                                     pow2=pow2)
        torch.cuda.synchronize()
        outs.append({k: r[k].cpu() for k in ("pred", "n_correct", "loss_sum", "track_sum")})
    for k in outs[0]:
        assert torch.equal(_bits(outs[0][k]), _bits(outs[1][k])), k
    got = outs[0]
    assert torch.equal(got["pred"][1][compare[1]], ref1["pred"][0][compare[1]])
    assert int(got["n_correct"][1]) == int(ref1["n_correct"][0]) > 0
    keep = [0, 2]
    ref = O.loss_fwd_bwd_upsampled(low[keep], y[keep], wts, 1, 3, with_grad=False)
    safe = compare[keep]
    assert torch.equal(got["pred"][keep][safe], ref["pred"][safe])
    assert ((got["n_correct"][keep].long() - ref["n_correct"]).abs() <= (~safe).view(2, -1).sum(-1)).all()
    for k, rk in (("loss_sum", "loss_img"), ("track_sum", "track_img")):
        assert torch.isfinite(got[k][keep]).all()
        torch.testing.assert_close(got[k][keep] / (H * W), ref[rk], rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------------ 9 deferred reduction
def test_deferred_reduction_feeds_the_apgd_bookkeeping(N):
    """loss_sum = track_sum = n_correct = NULL leaves the per-block records in the workspace; sea_apgd_track(init = 1) sums
    them.  Streaming kernel, C = 151, bf16: two tiles of eight pixels per lane where the register kernels would have ten
    of one -- a consumer that assumed the wrong grid would read records that were never written."""
    from semseg import attacker as A
    key = (2, 151, EVEN, 31, BF16, U8)
    logits, y, w = _case(*key)
    B, HW = 2, EVEN[0] * EVEN[1]
    ld, yd, wd = logits.cuda(), y.cuda(), w.cuda()
    eager = N.loss_fwd_bwd(ld, yd, wd, 1, 3, 1.0 / HW, want_grad=False)
    ref = _ref(key, 1, 3)
    assert torch.equal(eager["n_correct"].cpu().long(), ref["n_correct"])
    states = []
    for _ in range(2):
        ws = N.loss_workspace(B, HW, "cuda")
        ws.fill_(0xFF)                                   # (records the kernel does not write would be NaN / -1)
        d = N.loss_fwd_bwd(ld, yd, wd, 1, 3, 1.0 / HW, want_grad=False, workspace=ws, defer=True)
        assert d["loss_sum"] is None and d["track_sum"] is None and d["n_correct"] is None and d["workspace"] is ws
        st = A.ApgdState(B, 1, 8.0 / 255, "cuda")
        N.apgd_track(d, None, HW, 0, 1, 0, False, True, st)
        torch.cuda.synchronize()
        states.append(st)
    st = states[0]
    assert torch.equal(st.acc_cnt, eager["n_correct"])
    assert torch.equal(st.acc, eager["n_correct"].float() / HW)
    torch.testing.assert_close(st.loss_best, eager["track_sum"] / HW, rtol=1e-6, atol=0)
    torch.testing.assert_close(st.loss_best.double().cpu(), ref["track_sum"] / HW, **SUM_TOL)
    for k in ("acc_cnt", "acc", "loss_best", "loss_best_last"):
        assert torch.equal(_bits(getattr(st, k)), _bits(getattr(states[1], k))), k
