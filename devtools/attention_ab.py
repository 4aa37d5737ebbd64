#!/usr/bin/env python3
"""Two builds of libsea_hip.so side by side on the attention entries (M7 / M7b): bits and time, in one process on one device.

    python devtools/attention_ab.py PARENT_LIB NEW_LIB [--bits] [--time] [--rounds 12]       (default: both parts)

Both libraries are loaded by path with ctypes (each keeps its own kernels: the handles are local), and the four C entries
(sea_attention_fwd_terms, _bwd_terms, _fwd_f16, _bwd_f16) are called directly on seeded inputs, so nothing of
semseg/_native.py's dispatch takes part and the tool runs unchanged on a build from before or after a change of the kernels.

Bits: every arithmetic (22 = fp16 x 2, 3 / 2 = bf16 terms, 0 = fp32 MFMA), forward and the backward on the forward of the same
arithmetic, on shapes that reach every edge of the launch geometry; one line per case with the SHA-256 of out + lse or of the
packed dqkv of each build and `equal` / `DIFFERENT`.
Time: B = 8, H = 6, T = 1025 / 1175, arithmetics 22 and 3, forward and backward apart; both builds warmed, then interleaved rounds
parent, new, parent, new, ... with event timing over 4 calls per round; median and minimum per build.  `ok` = the new build's
median is at most 1.02 x the parent's from the same run (the noise of an attention A/B in one process is about 2 %).
Exit status 1 if any line reads DIFFERENT or SLOWER.
"""
import argparse
import ctypes as C
import hashlib
import statistics
import sys

import torch

D = 64
# (B, H, T): one row (every other lane clamped); ragged first tile; exactly one tile; second tile with one key; second block
# with one row (three idle waves); two blocks, ragged; the workload's T
BIT_SHAPES = [(2, 2, 1), (2, 2, 33), (2, 2, 64), (2, 2, 65), (2, 2, 129), (2, 3, 130), (1, 6, 1025)]
ARITHS = (22, 3, 2, 0)
TIME_SHAPES = [(8, 6, 1025), (8, 6, 1175)]
TIME_ARITHS = (22, 3)
BOUND = 1.02


def load(path):
    h = C.CDLL(path)
    for name in ("sea_attention_fwd_terms", "sea_attention_bwd_terms", "sea_attention_fwd_f16", "sea_attention_bwd_f16"):
        getattr(h, name).restype = C.c_int
    return h


def _p(t):
    return C.c_void_p(t.data_ptr())


def _i64(v):
    return C.c_int64(v)


class Case:
    """Seeded inputs and the buffers of one (B, H, T); forward() / backward() call one build's entries on them."""

    def __init__(self, B, H, T, seed):
        g = torch.Generator().manual_seed(seed)
        self.B, self.H, self.T = B, H, T
        qkv = torch.randn(B, T, 3, H, D, generator=g)
        qkv[:, :, 0] *= 1.5
        self.qkv = qkv.cuda()
        self.gout = torch.randn(B, T, H * D, generator=g).cuda()
        self.scale = D ** -0.5
        self.out = torch.zeros(B, T, H * D, device="cuda")
        self.lse = torch.zeros(B, H, T, device="cuda")
        self.delta = torch.zeros(B, H, T, device="cuda")
        self.dqkv = torch.zeros_like(self.qkv)
        self.ws = torch.zeros(4 * B * H, dtype=torch.int32, device="cuda")
        self.strides = (_i64(T * 3 * H * D), _i64(D), _i64(3 * H * D))

    def _triple(self, t):
        p = t.data_ptr()
        return C.c_void_p(p), C.c_void_p(p + 4 * self.H * D), C.c_void_p(p + 8 * self.H * D)

    def forward(self, lib, arith):
        head = (*self._triple(self.qkv), *self.strides, self.B, self.H, self.T, D, C.c_float(self.scale))
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if arith == 22:
            rc = lib.sea_attention_fwd_f16(*head, _p(self.ws), _p(self.out), _p(self.lse), st)
        else:
            rc = lib.sea_attention_fwd_terms(*head, _p(self.out), _p(self.lse), arith, st)
        if rc != 0:
            raise RuntimeError(f"forward, arithmetic {arith}: the entry returned {rc}")

    def backward(self, lib, arith):
        head = (*self._triple(self.qkv), *self.strides, self.B, self.H, self.T, D, C.c_float(self.scale), _p(self.out),
                _p(self.gout), _p(self.lse), _p(self.delta))
        tail = (*self._triple(self.dqkv), *self.strides)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if arith == 22:
            rc = lib.sea_attention_bwd_f16(*head, _p(self.ws), *tail, st)
        else:
            rc = lib.sea_attention_bwd_terms(*head, *tail, arith, st)
        if rc != 0:
            raise RuntimeError(f"backward, arithmetic {arith}: the entry returned {rc}")


def _sha(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def bits(libs):
    bad = 0
    for i, (B, H, T) in enumerate(BIT_SHAPES):
        c = Case(B, H, T, 100 + i)
        for arith in ARITHS:
            sums = {"fwd": [], "bwd": []}
            for lib in libs:
                for t in (c.out, c.lse, c.delta, c.dqkv):
                    t.fill_(float("nan"))
                c.forward(lib, arith)
                sums["fwd"].append(_sha(c.out, c.lse))
                c.backward(lib, arith)
                sums["bwd"].append(_sha(c.dqkv))
            for what in ("fwd", "bwd"):
                same = sums[what][0] == sums[what][1]
                bad += not same
                print(f"bits {what} arith={arith:<2d} B={B} H={H} T={T:<4d} parent {sums[what][0]} new {sums[what][1]} "
                      f"{'equal' if same else 'DIFFERENT'}", flush=True)
    return bad


def _timed(fn, calls=4):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3   # us per call


def times(libs, rounds):
    bad = 0
    for i, (B, H, T) in enumerate(TIME_SHAPES):
        c = Case(B, H, T, 200 + i)
        for arith in TIME_ARITHS:
            c.forward(libs[0], arith)           # the backward runs on this forward's out / lse
            for what in ("fwd", "bwd"):
                fns = [(lambda lib=lib: (c.forward if what == "fwd" else c.backward)(lib, arith)) for lib in libs]
                for fn in fns:                   # warm both builds
                    _timed(fn)
                    _timed(fn)
                t = [[], []]
                for _ in range(rounds):
                    for k, fn in enumerate(fns):
                        t[k].append(_timed(fn))
                med = [statistics.median(x) for x in t]
                ok = med[1] <= BOUND * med[0]
                bad += not ok
                print(f"time {what} arith={arith:<2d} B={B} H={H} T={T} rounds={rounds} us/call: parent median {med[0]:.1f} min {min(t[0]):.1f} | "
                      f"new median {med[1]:.1f} min {min(t[1]):.1f} | new/parent {med[1] / med[0]:.4f} "
                      f"{'ok' if ok else 'SLOWER'}", flush=True)
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_lib")
    ap.add_argument("new_lib")
    ap.add_argument("--bits", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--rounds", type=int, default=12)
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("--rounds: at least 10")
    libs = [load(a.parent_lib), load(a.new_lib)]
    print(f"device {torch.cuda.get_device_name(0)}; parent {a.parent_lib}; new {a.new_lib}", flush=True)
    both = not (a.bits or a.time)
    bad = 0
    if a.bits or both:
        bad += bits(libs)
    if a.time or both:
        bad += times(libs, a.rounds)
    print("attention_ab:", "all equal / ok" if bad == 0 else f"{bad} line(s) DIFFERENT or SLOWER")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
