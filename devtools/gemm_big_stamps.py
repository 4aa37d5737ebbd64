#!/usr/bin/env python3
"""Where does the per-tile fixed cost of M8's 256 x 256 kernel go?  A diagnostic build of csrc/gemm_split_big.hip
(-DSEA_GEMM_BIG_DIAG -> devtools/_knock/libbigdiag.so; never part of the product library) in which wave 0 of every block
stamps the 100 MHz clock at entry, first load (after the first round's stagger wait), first MFMA, end of the K loop, last C
store issued and stores drained (s_waitcnt vmcnt(0)), and records the CU it ran on (HW_ID, XCC_ID), plus the knock-outs
"no C stores" (1) and "non-temporal C stores" (64) and a run-time stagger step.
    python devtools/gemm_big_stamps.py --build                     (CPU, cross-compiles)
    python devtools/gemm_big_stamps.py [G M K N] [--steps=0,93,..]  (GPU; prints markdown)
Per shape, on a GPU kept busy for two seconds first: (a) the stamps of one launch in the middle of ten back to back, for
the full kernel without and with stagger and for both knock-outs: segment medians, the gap between a block's end and its
successor's entry on the same CU, and per round the p10-p90 span of the K loops' end times over the CUs (phase lock = a
span far below the tile time); (b) launch times of knock-outs x stagger steps, the rounds of all cells taken in turn."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "robust-segmentation_amd")
SO = os.path.join(ROOT, "devtools", "_knock", "libbigdiag.so")

if "--build" in sys.argv:
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-fPIC", "-shared", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize",
                    "-DSEA_GEMM_BIG_DIAG", os.path.join(PKG, "csrc", "gemm_split_big.hip"), "-o", SO], check=True)
    print(SO)
    sys.exit(0)

sys.path[:0] = [ROOT, PKG]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from semseg import _native as N  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("-")]
G, M, K, Nn = [int(v) for v in (args[:4] if len(args) >= 4 else (36, 8192, 512, 512))]
STEPS = next(([int(v) for v in a[8:].split(",")] for a in sys.argv if a.startswith("--steps=")), [0, 93, 186, 372, 690])
L = C.CDLL(SO)
L.sea_gemm_big_diag.restype = C.c_int
L.sea_gemm_big_diag.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
A = torch.randn(G, M, K, device="cuda")
W = torch.randn(G, Nn, K, device="cuda") / K ** 0.5
Wp = N.gemm_split_pack(W, terms=22)
out = torch.empty(G, M, Nn, device="cuda")
amax = torch.empty(M, dtype=torch.int32, device="cuda")
N.lib().sea_absmax_bits(N._p(A[0]), K, M, K, 1, 0, 1, N._p(amax), N._stream())
TILES = G * ((M + 255) // 256) * (Nn // 256)
stamps = torch.zeros(TILES, 8, dtype=torch.int64, device="cuda")
CUS = torch.cuda.get_device_properties(0).multi_processor_count


def launch(ko, step, st=None):
    rc = L.sea_gemm_big_diag(A.data_ptr(), K, Wp.data.data_ptr(), out.data_ptr(), Nn, M, Nn, K, G, M * K, Wp.stride, M * Nn,
                             amax.data_ptr(), 1, ko, step, st.data_ptr() if st is not None else None, N._stream())
    assert rc == 0, rc


def timed(ko, step, reps=20):
    launch(ko, step)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch(ko, step)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def us(ticks):
    return np.asarray(ticks, dtype=np.float64) / 100.0


def warm(seconds=2.0):   # the clocks of an idle GPU take a second to come up: stamps and timings are taken on a busy one
    import time
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(50):
            launch(0, 0)
        torch.cuda.synchronize()


def stamp_table(ko, step):
    warm(0.5)
    for i in range(10):   # the stamped launch sits in the middle of ten: its neighbours are the unstamped kernel
        launch(ko, step, stamps if i == 5 else None)
    torch.cuda.synchronize()
    s = stamps.cpu().numpy().astype(np.int64)
    t = s[:, :6] - s[:, 0].min()
    cu = ((s[:, 6] >> 32) & 0xf) * 256 + ((s[:, 6] >> 8) & 0xff)
    seg = {"entry -> first load (stagger wait)": t[:, 1] - t[:, 0], "first load -> first MFMA (prologue)": t[:, 2] - t[:, 1],
           "K loop": t[:, 3] - t[:, 2], "K loop end -> last store issued": t[:, 4] - t[:, 3],
           "last store issued -> drained": t[:, 5] - t[:, 4], "whole block": t[:, 5] - t[:, 0]}
    print(f"\nko={ko} step={step} ticks: {len(np.unique(cu))} distinct CUs, launch span {us(t[:, 5].max()):.1f} us\n")
    print("| segment (wave 0) | median us | p10 | p90 |\n|---|---|---|---|")
    for name, v in seg.items():
        print(f"| {name} | {np.median(us(v)):.2f} | {np.percentile(us(v), 10):.2f} | {np.percentile(us(v), 90):.2f} |")
    gaps, rounds = [], {}
    for c in np.unique(cu):
        rows = t[cu == c]
        rows = rows[np.argsort(rows[:, 0])]
        gaps += list(rows[1:, 0] - rows[:-1, 5])
        for r, row in enumerate(rows):
            rounds.setdefault(r, []).append(row)
    g = us(gaps)
    print(f"| block end -> successor's entry, same CU | {np.median(g):.2f} | {np.percentile(g, 10):.2f} | {np.percentile(g, 90):.2f} |")
    print("\n| round on its CU | blocks | K-loop end: p10-p90 span over CUs, us | median block us | median K loop us | median K loop end -> stores issued us |\n|---|---|---|---|---|---|")
    for r in sorted(rounds):
        rows = np.array(rounds[r])
        if len(rows) < 16:
            continue
        e = us(rows[:, 3])
        print(f"| {r} | {len(rows)} | {np.percentile(e, 90) - np.percentile(e, 10):.1f} | {np.median(us(rows[:, 5] - rows[:, 0])):.1f} |"
              f" {np.median(us(rows[:, 3] - rows[:, 2])):.1f} | {np.median(us(rows[:, 4] - rows[:, 3])):.2f} |")


print(f"## G={G} M={M} K={K} N={Nn}: {TILES} tiles, {CUS} CUs, {K // 32} K steps, C = {G * M * Nn * 4 / 1e6:.0f} MB")
warm()
stamp_table(0, 0)
stamp_table(0, 186)
stamp_table(1, 0)
stamp_table(64, 0)
warm(0.5)
print("\n| 20 launches back to back, median [min - max] of five rounds taken in turn | full kernel us | non-temporal C stores us | no C stores us |\n|---|---|---|---|")
res = {(ko, step): [] for step in STEPS for ko in (0, 64, 1)}
for _ in range(5):
    for key in res:
        res[key].append(timed(*key))
for step in STEPS:
    cells = " | ".join(f"{np.median(res[ko, step]):.1f} [{min(res[ko, step]):.1f} - {max(res[ko, step]):.1f}]" for ko in (0, 64, 1))
    print(f"| stagger step {step} ticks (spread {step * 8 / 100:.1f} us) | {cells} |", flush=True)
