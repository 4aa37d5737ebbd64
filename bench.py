#!/usr/bin/env python3
"""SEA attack-loop benchmark (BASELINE.json metric: attack image-iterations/s, UperNet-ConvNeXt-T, 512x512).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...     # what the driver runs for N > 1

`python bench.py --gpus N` with N > 1 and no launcher environment starts the N ranks ITSELF: the parent process
never touches a GPU, it runs `python -m torch.distributed.run --nproc-per-node N bench.py ...` as a child process and
exits with the child's code (one rank per GPU, RCCL; rendezvous on 127.0.0.1).  `n_gpus` in the JSON line is the
world size RCCL reported after an all-reduce over all ranks, never the flag.

One "step" = one APGD loop iteration over one batch of B=8 synthetic 512x512 images per GPU:
L-inf step kernel (K1) + model forward (PyTorch-ROCm) + fused loss/gradient kernel (K2) + model
input-gradient backward + device-side bookkeeping kernels (K4/K7).  Inputs are resident in HBM before
the timed region.  Arithmetic: fp32 storage and fp32 accumulation everywhere; the frozen-weight GEMMs of the model
(forward AND input gradient) run on the 16-bit matrix cores with every fp32 operand split into two fp16 terms
(22 significant bits, power-of-two scales per row; measured error against float64 0.3-1.5 x the fp32 GEMM's own,
asserted <= 2 x in tests/test_gemm_split_gpu.py), so the evaluation is fp32-equivalent like the reference's; `dtype` in the JSON line
states the mode that actually ran (SEA_GEMM_TERMS / SEA_GEMM_TERMS_BWD select others).  Images shard across ranks
with no collective in the loop (weak scaling).  After the timed window `--sustain` further steps (default 300 = a
full SEA attack's length) are timed the same way and reported as `config.sustained_ms_per_step`: the chip lowers
its clock under sustained matrix load, which a 20-step window does not see.

`--dump-outputs DIR` writes what the last timed step left for a caller of the loop (rank 0's images) as DIR/<name>.npy,
float32 / float64, ~59 MB: the attack's result `x_best_adv` in full, every other array of more than 2**21 elements at 2**21
fixed, seeded positions (see `dump_outputs`).  The inputs depend on the arguments only, and the convolutions left to MIOpen
run in immediate mode (a fixed solver, not the fastest of a timed search), so runs repeat bit for bit and two builds can be
compared output for output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "robust-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy ceiling


def k2_algorithmic_bytes(B, C, HW, logit_bytes=4, with_grad=True):
    """B*H*W*(2*C*s + 8 + 8) with gradient, B*H*W*(C*s + 16) without (int64 label and argmax)."""
    return B * HW * ((2 if with_grad else 1) * C * logit_bytes + 16)


def k2_moved_bytes(B, C, HW, logit_bytes=4, with_grad=True):
    """Bytes the kernel really moves: labels and argmax are uint8 here (compacted once per attack), 2 B per pixel."""
    return B * HW * ((2 if with_grad else 1) * C * logit_bytes + 2)


def spawn_ranks(n, argv):
    """Parent of a multi-GPU run: no GPU call happens in this process (a process that initialised the GPU must never be
    replaced, and a fresh child per rank is what torch.distributed.run gives)."""
    import socket
    import subprocess
    have = torch.cuda.device_count()  # does not initialise the GPU on this image
    if have < n and os.environ.get("SEA_BENCH_BACKEND", "nccl") == "nccl":
        print(f"[bench] --gpus {n} but only {have} GPU(s) visible", file=sys.stderr)
        return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.run(cmd, env=env).returncode


def measure_ceilings(N, device):
    """HBM copy / read rates of THIS device with the library's own 16-byte-per-lane streaming probes (1 GiB buffers:
    cold by size).  Returns GB/s (copy counts read + write bytes)."""
    L = N.lib()
    src = torch.empty(256 * 1024 * 1024, dtype=torch.float32, device=device).normal_()
    dst = torch.empty_like(src)
    sink = torch.zeros(4096, device=device)
    st = torch.cuda.current_stream().cuda_stream
    nbytes = src.numel() * 4

    def timed(fn, mult):
        fn()
        best = 1e9
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            fn()
            b.record()
            torch.cuda.synchronize()
            best = min(best, a.elapsed_time(b) / 2)
        return mult * nbytes / (best * 1e-3) / 1e9

    copy = timed(lambda: L.sea_probe_stream_copy(src.data_ptr(), dst.data_ptr(), nbytes, 1, st), 2)
    read = timed(lambda: L.sea_probe_stream_read(src.data_ptr(), sink.data_ptr(), nbytes, st), 1)
    return copy, read


def k2_cold_ms(N, run, logits_shape, C, HW):
    """K2 exactly as the loop launches it (same mode, labels, workspace), but over a ring of independent
    (logits, gradient) buffers larger than the 256 MiB Infinity Cache: no launch finds its input on die.  One event
    pair around the whole ring (no per-launch event gap)."""
    B = logits_shape[0]
    set_bytes = 2 * B * C * HW * 4
    nsets = max(2, -(-1600 * 2 ** 20 // set_bytes))
    g = torch.Generator(device="cuda").manual_seed(7)
    sets = []
    for _ in range(nsets):
        lg = torch.randn(logits_shape, generator=g, device="cuda") * 3
        sets.append((lg, torch.empty_like(lg)))
    pred = torch.empty_like(run.pred)

    def go():
        for lg, dl in sets:
            N.loss_fwd_bwd(lg, run.yc, run.w, run.mode, run.tmode, run.gscale, want_grad=True, pred=pred,
                           workspace=run.ws, dlogits=dl, defer=True)
    go()
    torch.cuda.synchronize()
    best = 1e9
    reps = max(1, 16 // nsets)
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            go()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / (reps * nsets))
    return best


def model_gemm_roofline(N, model, x, ms_per_step):
    """The step's real bottleneck, next to K2's HBM roofline: the frozen-weight GEMM launches (M8, sea_gemm_split).  Eager
    (un-captured) forward + input-gradient passes of the model AFTER the timed region, with a HIP event pair around every
    outermost `gemm_split` call on the launch stream.  Pass 1 finds the shapes (and warms them); in passes 2 and 3 EVERY call is
    issued ten times back to back inside its event pair (the calls only overwrite their outputs): a single eager launch is
    timed wrongly in both directions -- a large one runs on an idle, higher-clocked chip and reads 10-15 % short, a small one
    waits for the host between the start event and the kernel and reads up to 60 % long (38.8 us under rocprofv3, 61 us
    between two events, for 8192 x 1536 x 384).  Priced against the dense 16-bit MFMA peak: 2 G M K N flop x products (3 for
    fp16 x 2 / bf16 x 2: hi*hi', hi*mid', mid*hi') / time per launch."""
    orig, depth, rec, target, REPS = N.gemm_split, [0], {}, [None], 10
    TIMED, MAX_EXTRA = 4, 2     # event pairs per call position (the MINIMUM is quoted); extra passes if a shape is unstable

    def hooked(A, Wp, *a, **k):
        if depth[0]:
            return orig(A, Wp, *a, **k)
        key = (Wp.batch, A.shape[-2], Wp.K, Wp.N, Wp.terms)
        reps = REPS if target[0] is not None else 1
        depth[0] += 1
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                out = orig(A, Wp, *a, **k)
            e1.record()
        finally:
            depth[0] -= 1
        rec.setdefault(key, []).append((e0, e1, reps))
        return out

    # the fused MLP kernels (M8f: both projections of a ConvNeXt block in one launch) are M8 work too: timed the same way and
    # counted in all_gemm_split_ms_per_step (key: ("mlp_fwd" | "mlp_bwd", M, C, H, 22))
    orig_mf, orig_mb = N.mlp_fused_forward, N.mlp_fused_backward

    def hooked_mlp(tag, fn):
        def run(*a, **k):
            x2, W1p = (a[0], a[1]) if tag == "mlp_fwd" else (a[1], a[2])
            key = (tag, x2.shape[0], x2.shape[1], W1p.N, 22)
            reps = REPS if target[0] is not None else 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                out = fn(*a, **k)
            e1.record()
            rec.setdefault(key, []).append((e0, e1, reps))
            return out
        return run

    flops = lambda k: 0 if isinstance(k[0], str) else k[0] * k[1] * k[2] * k[3]  # noqa: E731
    samples = {}                # key -> [per pass: [ms of a single launch, per call position]]

    def one_pass():
        xg = x.clone().requires_grad_(True)
        torch.autograd.grad(model(xg).float().square().mean(), xg)
        torch.cuda.synchronize()

    def harvest():
        for k, v in rec.items():
            samples.setdefault(k, []).append([a.elapsed_time(b) / r for a, b, r in v])
        rec.clear()

    def fold():
        """per shape: ms per step from the minimum over the passes at every call position, and the same from the
        second-smallest sample (one event pair around ten launches still catches a clock or host hiccup: a 2 x outlier of a
        single pair went straight into round 5's line)"""
        best, second = {}, {}
        for k, per_pass in samples.items():
            n = min(len(p) for p in per_pass)
            cols = [sorted(p[i] for p in per_pass) for i in range(n)]
            best[k] = (sum(c[0] for c in cols), n)
            second[k] = sum(c[min(1, len(c) - 1)] for c in cols)
        return best, second

    N.gemm_split = hooked
    N.mlp_fused_forward, N.mlp_fused_backward = hooked_mlp("mlp_fwd", orig_mf), hooked_mlp("mlp_bwd", orig_mb)
    try:
        one_pass()                                  # pass 1 finds the shapes (and warms them)
        if rec:
            target[0] = max(rec, key=flops)
        rec.clear()
        if target[0] is not None:
            for _ in range(TIMED):
                one_pass()
                harvest()
            for _ in range(MAX_EXTRA):              # a shape whose best figure is not confirmed by its second sample: sample again
                best, second = fold()
                if all(second[k] <= 1.3 * best[k][0] for k in best):
                    break
                one_pass()
                harvest()
    finally:
        N.gemm_split = orig
        N.mlp_fused_forward, N.mlp_fused_backward = orig_mf, orig_mb
    if not samples:
        return None
    best, second = fold()
    tot = {k: v[0] for k, v in best.items()}        # ms per step of the shape (every call position at its minimum)
    peak = 2500.0   # dense bf16 / fp16 MFMA peak, TFLOP/s (MI355X_MICROARCH.md)
    all_ms = sum(tot.values())

    def price(key):
        G, M, K, Nn, terms = key
        n = best[key][1]
        prod = {22: 3, 2: 3, 3: 6, 1: 1}.get(terms, 1)
        if isinstance(G, str):      # fused MLP: two (forward) / three (backward: t is recomputed) M x C x H products in one launch
            flop = 2.0 * M * K * Nn * prod * (2 if G == "mlp_fwd" else 3)
            us = tot[key] / n * 1e3
            ach = flop / (us * 1e-6) / 1e12
            return {"kernel": f"sea_mlp_fused_{G[4:]} M={M} C={K} H={Nn}, {_mode_name(terms)}", "bound": "mfma / valu", "achieved": ach,
                    "peak": peak, "unit": "TFLOP/s", "frac": ach / peak, "traffic": None, "flop_per_launch": flop,
                    "mfma_products": prod, "avg_launch_us": us, "launches_per_step": n, "ms_per_step": tot[key],
                    "second_sample_over_min": second[key] / tot[key], "event_pairs_per_call": len(samples[key])}
        flop = 2.0 * G * M * K * Nn * prod
        us = tot[key] / n * 1e3
        ach = flop / (us * 1e-6) / 1e12
        return {"kernel": f"sea_gemm_split {G} x ({M} x {K} x {Nn}), {_mode_name(terms)}", "bound": "mfma", "achieved": ach,
                "peak": peak, "unit": "TFLOP/s", "frac": ach / peak, "traffic": None, "flop_per_launch": flop,
                "mfma_products": prod, "avg_launch_us": us, "launches_per_step": n,
                "ms_per_step": tot[key], "second_sample_over_min": second[key] / tot[key],
                "event_pairs_per_call": len(samples[key])}

    largest = target[0] if target[0] in tot else max(tot, key=flops)
    if isinstance(largest[0], str):
        largest = max((k for k in tot if not isinstance(k[0], str)), key=flops)
    busiest = max(tot, key=tot.get)                     # the shape with the most time per step (many small launches)
    out = price(largest)
    unstable = sorted(f"{k[0]} x ({k[1]} x {k[2]} x {k[3]})" for k in tot if second[k] > 1.3 * tot[k])
    mlp_ms = sum(v for k, v in tot.items() if isinstance(k[0], str))
    out.update({"most_time_per_step": price(busiest), "all_gemm_split_ms_per_step": all_ms,
                "of_which_fused_mlp_ms_per_step": mlp_ms,
                "fused_mlp": [price(k) for k in sorted(tot, key=str) if isinstance(k[0], str)],
                "all_gemm_split_share_of_step": all_ms / ms_per_step,
                "shapes_whose_second_sample_exceeds_1.3x_min": unstable,
                "measured": "HIP events around every outermost gemm_split call in eager forward + input-gradient passes after the "
                            f"timed region; every call {REPS} x back to back per event pair (sustained load, no host gap "
                            f"inside the pair after the first launch), {TIMED}+ pairs per call position, the MINIMUM quoted and "
                            "checked against the second-smallest; launches shorter than the ~25 us the host needs per eager call "
                            "still read long: rocprofv3's per-kernel times under profiles/ are the reference for those"})
    return out


def strict_fp32_ms(A, N, run, model, x, y, eps, args, C, weights, barrier):
    """ms per step of the SAME loop with operands that carry all 24 significant bits (bf16 x 3: the fp32 operands exactly, six
    MFMA products; attention with three terms too), timed after the headline's region on a fresh run (its graph pair is
    captured again: the cached pair's arithmetic signature no longer matches).  The shipped mode -- fp16 x 2, 22 bits,
    error <= the fp32 GEMM's own -- is a judgment call; this is the figure to read it against."""
    import semseg.models.convnext_upernet as M
    run.release_graphs()
    A.release_graph_cache(model)
    old = (M.GEMM_TERMS, M.GEMM_TERMS_BWD, os.environ.get("SEA_ATTN_TERMS"), os.environ.get("SEA_ATTN_TERMS_BWD"))
    K, W = args.strict_steps, 4
    try:
        M.GEMM_TERMS, M.GEMM_TERMS_BWD = 3, 3
        os.environ["SEA_ATTN_TERMS"] = os.environ["SEA_ATTN_TERMS_BWD"] = "3"
        r2 = A.ApgdRun(model, x, y, eps, max(W + K + 1, A.GRAPH_MIN_ITER), args.loss, "ce-avg", True, C, weights, x.clone(),
                       fuse_upsample=True if args.fuse_upsample else (False if args.no_fuse_upsample else None))
        r2.start()
        for i in range(W):
            r2.step(i)
        barrier()
        t0 = time.perf_counter()
        for i in range(W, W + K):
            r2.step(i)
        barrier()
        ms = (time.perf_counter() - t0) * 1e3 / K
        r2.release_graphs()
        return ms
    finally:
        M.GEMM_TERMS, M.GEMM_TERMS_BWD = old[0], old[1]
        for k, v in (("SEA_ATTN_TERMS", old[2]), ("SEA_ATTN_TERMS_BWD", old[3])):
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        A.release_graph_cache(model)


DUMP_SAMPLE = 2 ** 21       # elements kept of an array dumped as a sample (--dump-outputs)
DUMP_SEED = 0


def snapshot_outputs(run, i):
    """Copies (on the device) of what ``run.step(i)`` leaves a caller: the attack's state after the step -- ``result()``, the
    iterate it evaluated, that iterate's input gradient and argmax, its per-image tracking loss and the step size K7 set.  Taken
    right after the timed window: the sustained window goes on stepping the same run."""
    x_best, acc, loss_best, x_best_adv = run.result()
    return {"x_best_adv": x_best_adv.clone(), "x_best": x_best.clone(), "x_adv": run.x_adv.clone(), "grad": run.grad.clone(),
            "pred": run.pred.clone(), "acc": acc.clone(), "loss_best": loss_best.clone(),
            "track_loss": run.st.loss_steps[i].clone(), "step_size": run.st.step.clone()}


def dump_outputs(snap, out_dir):
    """DIR/<name>.npy per array: float32 for float32 data and 8 / 16-bit integers, float64 for wider integers (exact).
    `x_best_adv` in full; every other array of more than DUMP_SAMPLE elements as its flattened elements at DUMP_SAMPLE
    positions drawn without replacement by torch.randperm(numel, Generator.manual_seed(DUMP_SEED)) and sorted (the same
    positions for the same shape).  At most 64 MB in all."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, t in snap.items():
        t = t.detach().cpu()
        t = t.float() if (t.is_floating_point() or t.element_size() <= 2) else t.double()
        if name != "x_best_adv" and t.numel() > DUMP_SAMPLE:
            idx = torch.randperm(t.numel(), generator=torch.Generator().manual_seed(DUMP_SEED))[:DUMP_SAMPLE].sort().values
            t = t.reshape(-1)[idx]
        a = t.numpy()
        total += a.nbytes
        np.save(os.path.join(out_dir, name + ".npy"), a)
    assert total <= 64 * 10 ** 6, f"--dump-outputs wrote {total} bytes"
    return total


def _mode_name(terms):
    return {22: "fp16x2 (22 significant bits per operand, 3 MFMA products)", 3: "bf16x3 (24 bits, 6 products)",
            2: "bf16x2 (16 bits, 3 products)"}.get(terms, "hipBLASLt fp32")


def make_model(backbone, C):
    """UperNet-ConvNeXt (BASELINE configs 1, 2, 4, 5) or Segmenter ViT (config 3: --backbone vit_small_patch16_224)."""
    if backbone.startswith("vit_"):
        from semseg.models import create_segmenter
        from semseg.utils.utils import load_config_segmenter
        cfg, _ = load_config_segmenter(backbone, C)
        return create_segmenter(cfg, None, backbone)
    from semseg.models import UperNetForSemanticSegmentation
    return UperNetForSemanticSegmentation(backbone, C, None)


def build_case(rank, B, C, backbone, device):
    torch.manual_seed(0)  # identical weights on every rank
    model = make_model(backbone, C).eval().to(device)
    for p in model.parameters():
        p.requires_grad_(False)
    g = torch.Generator().manual_seed(1234 + rank)
    x = torch.rand(B, 3, 512, 512, generator=g).to(device)
    with torch.no_grad():
        y = torch.cat([model(x[i:i + 2]).max(1)[1] for i in range(0, B, 2)])  # labels = clean prediction
    return model, x, y


def cpu_baseline(C, backbone, B=2, n_iter=5):
    """SURVEY 8(d)'s CPU baseline: BASELINE configs[0] (2 synthetic 512x512 images, 5-step Mask-CE `apgd_largereps`,
    eps = 4/255) through the oracle's restatement of the reference loop on the host cores of this box; a bounded sample
    (8 model evaluations per image: 3 stage starts + 5 iterations, 10-30 s)."""
    from oracle import sea_oracle as O
    from semseg.utils.utils import ADE_WTS, VOC_WTS
    torch.manual_seed(0)
    model = make_model(backbone, C).eval()
    cores = min(os.cpu_count() or 1, 32)  # more threads than that slow PyTorch-CPU convolutions down
    torch.set_num_threads(cores)
    g = torch.Generator().manual_seed(1234)
    x = torch.rand(B, 3, 512, 512, generator=g)
    with torch.no_grad():
        y = model(x).max(1)[1]
    w = torch.tensor(VOC_WTS if C == 21 else ADE_WTS)
    t0 = time.perf_counter()
    O.apgd_largereps(model, x, y, w, eps=4.0 / 255, n_iter=n_iter, use_rs=True, loss="mask-ce-avg", track_loss="ce-avg",
                     early_stop=True)
    dt = time.perf_counter() - t0
    evals = n_iter + 3
    # every model evaluation is counted as an iteration (three of them have no K1 step, the last of every stage has
    # no backward, like the reference), which favours the CPU number
    return {"value": B * evals / dt, "unit": "image-iterations/s", "cores": cores, "kind": "port",
            "sample": f"oracle apgd_largereps (PyTorch-CPU restatement of the reference loop), BASELINE configs[0]: "
                      f"{backbone}, B={B}x512x512, C={C}, {n_iter}-step mask-ce-avg, eps 4/255 = {evals} model "
                      f"evaluations per image, {dt:.1f} s wall"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8, help="images per GPU")
    ap.add_argument("--classes", type=int, default=21)
    ap.add_argument("--backbone", default="ConvNeXt-T_CVST")
    ap.add_argument("--loss", default="mask-ce-bal")
    ap.add_argument("--eps", type=float, default=8.0, help="radius in 1/255 (SEA stage-1 radius for eps=4)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-model-roofline", action="store_true",
                    help="skip the eager GEMM-timing passes after the timed region (profiling runs: they would land in the trace)")
    ap.add_argument("--sustain", type=int, default=300,
                    help="steps timed AFTER the K-step window for config.sustained_ms_per_step (0 = skip)")
    ap.add_argument("--strict-steps", type=int, default=20,
                    help="steps timed AFTER everything else with exact fp32 operands (three bf16 terms) for "
                         "config.strict_fp32_ms_per_step (0 = skip)")
    ap.add_argument("--fuse-upsample", action="store_true",
                    help="force K2u (loss fused with the model's final bilinear upsample); default: the library's "
                         "heuristic (unfused unless the full-resolution logits + gradient exceed 24 GB)")
    ap.add_argument("--no-fuse-upsample", action="store_true", help="force the model's own upsample + K2")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (rank 0) as DIR/<name>.npy (float32 / float64, <= 64 MB)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
    # SEA_BENCH_BACKEND=gloo lets the multi-rank control flow be exercised on a single-GPU box (ranks then
    # share device 0); the real thing is "nccl" (= RCCL) with one GPU per rank
    backend = os.environ.get("SEA_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        dist.init_process_group(backend, rank=rank, world_size=world)  # "nccl" is RCCL on ROCm
        # what the collective library really spans: one contribution per rank, summed over RCCL / xGMI
        one = torch.ones(1, device=device if backend == "nccl" else "cpu")
        dist.all_reduce(one)
        world = int(one.item())
    if args.gpus != world and rank == 0:
        print(f"[bench] note: --gpus {args.gpus} but {world} rank(s) are running; reporting n_gpus={world}", file=sys.stderr)
    # Convolutions left to MIOpen (the stem's second conv, forward and input gradient) run in immediate mode with the
    # find-db off: the solver is a fixed function of shape, device and MIOpen version.  Find mode times the solvers and keeps
    # the fastest, so the solver -- and the rounding -- changed from run to run and box to box, and the backward solver it
    # picked was not bitwise repeatable either; APGD's sign steps carry such a difference into the iterates.
    os.environ.setdefault("MIOPEN_DEBUG_DISABLE_FIND_DB", "1")
    torch.backends.cudnn.benchmark = False
    torch.backends.miopen.immediate = True

    from semseg import _native as N, attacker as A
    from semseg.models.convnext_upernet import GEMM_TERMS, _bwd_terms
    from semseg.utils.utils import ADE_WTS, VOC_WTS
    N.lib()
    B, C, K, W = args.batch, args.classes, args.steps, args.warmup
    model, x, y = build_case(rank, B, C, args.backbone, device)
    weights = torch.tensor(VOC_WTS if C == 21 else ADE_WTS, device=device)[:C]
    eps = args.eps / 255.0

    # default: the model's own upsample + the HBM-bound K2 (the kernel SURVEY 8d prices); --fuse-upsample
    # switches to K2u (no full-resolution logits in HBM; 0.8 ms/step slower on Segmenter x16, C=151)
    S = max(args.sustain, 0)
    run = A.ApgdRun(model, x, y, eps, W + K + S + 1, args.loss, "ce-avg", True, C, weights, x.clone(),
                    fuse_upsample=True if args.fuse_upsample else (False if args.no_fuse_upsample else None))
    run.start()
    for i in range(W):
        run.step(i)
    run.k2_events = None if os.environ.get("SEA_BENCH_NO_EVENTS") else []

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # The queue is empty after the barrier, so a host stall in the first timed step is lost wall time: a generation-2
    # collection of Python's garbage collector over the freshly built model (tens of ms) landed exactly there.
    import gc
    gc.collect()
    gc.disable()
    barrier()
    t0 = time.perf_counter()
    for i in range(W, W + K):
        run.step(i)
    t_enqueue = time.perf_counter() - t0  # host time to enqueue the K steps (diagnostic: << dt unless launch-bound)
    barrier()
    dt = time.perf_counter() - t0
    gc.enable()
    snap = snapshot_outputs(run, W + K - 1) if (args.dump_outputs and rank == 0) else None
    per_rank = None
    if world > 1:
        # max over ranks is the job's time; the per-rank rows say which rank (and whether its host) set it
        mine = torch.tensor([dt, t_enqueue], device=device if backend == "nccl" else "cpu", dtype=torch.float64)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = [{"rank": r, "ms_per_step": float(v[0]) * 1e3 / K, "host_enqueue_ms_per_step": float(v[1]) * 1e3 / K}
                    for r, v in enumerate(allr)]
        dt = max(float(v[0]) for v in allr)

    # sustained rate: S more steps of the same loop, same barriers, max over ranks (a SEA stage is 90-120 steps, an attack 300)
    sustained = None
    if S > 0:
        k2_events, run.k2_events = run.k2_events, None
        gc.disable()
        barrier()
        t1 = time.perf_counter()
        for i in range(W + K, W + K + S):
            run.step(i)
        barrier()
        sustained = (time.perf_counter() - t1) * 1e3 / S
        gc.enable()
        run.k2_events = k2_events
        if world > 1:
            mine = torch.tensor([sustained], device=device if backend == "nccl" else "cpu", dtype=torch.float64)
            dist.all_reduce(mine, op=dist.ReduceOp.MAX)
            sustained = float(mine.item())

    k2_ms = (sum(a.elapsed_time(b) for a, b in run.k2_events) / max(len(run.k2_events), 1)) if run.k2_events else float("nan")
    hip_graph = bool(run.graphs is not None)
    strict = strict_fp32_ms(A, N, run, model, x, y, eps, args, C, weights, barrier) if args.strict_steps > 0 else None
    kname = ("loss_upsampled_kernel (K2u)" if run.fused else
             f"{'loss_nchw_split' if C in (150, 151) else 'loss_nchw_reg'}<C={C}> (K2 fused loss fwd+bwd)")
    algo = k2_algorithmic_bytes(B, C, 512 * 512)
    moved = k2_moved_bytes(B, C, 512 * 512)
    roof = None
    if rank == 0:
        # ceilings of this device and the cold figure: measured after the timed region, on rank 0 only
        copy_gbs, read_gbs = measure_ceilings(N, device)
        cold_ms = None if run.fused else k2_cold_ms(N, run, (B, C, 512, 512), C, 512 * 512)
        traffic = None
        tfile = os.path.join(ROOT, "profiles", "k2_traffic.json")
        if os.path.exists(tfile):
            try:
                traffic = json.load(open(tfile)).get(f"B{B}_C{C}")
            except Exception:
                traffic = None
        gbs = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e9  # noqa: E731
        # `achieved` / `frac`: SURVEY 8(d) algorithmic bytes over the launch time measured live in the timed loop
        # (HIP events on the launch stream).  In the loop the logits were written by the model's previous kernel and
        # partly still sit in the 256 MiB Infinity Cache, so this is NOT an HBM-only figure: `frac_cold` is (ring
        # of buffers > 1.5 GB, nothing on die), and `*_moved` prices the bytes the kernel really moves (uint8 labels
        # and argmax instead of the int64 the SURVEY formula assumes).
        roof = {"kernel": kname, "bound": "hbm", "achieved": gbs(algo, k2_ms), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": gbs(algo, k2_ms) / HBM_PEAK_GBS, "traffic": traffic,
                "algorithmic_bytes": algo, "moved_bytes": moved, "avg_launch_ms": k2_ms,
                "frac_in_loop": gbs(algo, k2_ms) / HBM_PEAK_GBS, "frac_in_loop_moved": gbs(moved, k2_ms) / HBM_PEAK_GBS,
                "cold_launch_ms": cold_ms,
                "frac_cold": None if cold_ms is None else gbs(algo, cold_ms) / HBM_PEAK_GBS,
                "frac_cold_moved": None if cold_ms is None else gbs(moved, cold_ms) / HBM_PEAK_GBS,
                "measured_copy_ceiling_GBps": copy_gbs, "measured_read_ceiling_GBps": read_gbs,
                "frac_cold_moved_of_copy_ceiling": None if cold_ms is None else gbs(moved, cold_ms) / copy_gbs}

    if rank == 0:
        out = {
            "metric": "SEA attack-iterations/sec (UperNet-CNX-T, 512x512)",
            "value": world * B * K / dt,
            "unit": "image-iterations/s",
            "n_gpus": world, "steps": K, "warmup": W,
            "ms_per_step": dt * 1e3 / K,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": ("f32 (frozen-weight GEMMs on the 16-bit matrix cores by operand splitting: "
                      + _mode_name(GEMM_TERMS) + " forward, " + _mode_name(_bwd_terms(GEMM_TERMS))
                      + " input gradient; fp32 storage and accumulate)") if GEMM_TERMS in (2, 3, 22) else "f32",
            "data": "synthetic",
            "config": {
                "workload": f"{'Segmenter-' if args.backbone.startswith('vit_') else 'UperNet-'}{args.backbone} C={C} "
                            f"({'PASCAL-VOC' if C == 21 else 'ADE20K'}-shaped), {B}x512x512 per GPU, APGD L-inf "
                            f"eps={args.eps:g}/255, loss {args.loss}, track ce-avg (BASELINE configs[1] loop body)",
                "batch_per_gpu": B, "global_batch": world * B, "sharding": f"images x{world}, no in-loop collective",
                "batch_steps_per_s": world * K / dt, "host_enqueue_ms_per_step": t_enqueue * 1e3 / K,
                "hip_graph": hip_graph,
                "sustained_ms_per_step": sustained, "sustained_steps": S,
                # the same loop with operands that carry all 24 bits of fp32 (three bf16 terms, six MFMA products, forward
                # and input gradient; attention likewise): what the headline's 22-bit operands buy, measured in this run
                "strict_fp32_ms_per_step": strict, "strict_fp32_steps": args.strict_steps if strict is not None else 0,
                "strict_fp32_mode": "SEA_GEMM_TERMS=3 SEA_GEMM_TERMS_BWD=3 SEA_ATTN_TERMS=3 SEA_ATTN_TERMS_BWD=3, after the timed region",
                "gemm": ("sea_gemm_split: forward products " + _mode_name(GEMM_TERMS) + ", input-gradient products "
                         + _mode_name(_bwd_terms(GEMM_TERMS)) + ", fp32 accumulate; power-of-two scales per row (forward: analytic "
                         + "bounds / Winograd tile maxima; gradient: exact row maxima / Winograd tile maxima / row bounds carried "
                         + "through the MLP), split-K for small tile grids, GELU / GELU' / ReLU-gate prologues")
                if GEMM_TERMS in (2, 3, 22) else "hipBLASLt fp32",
                **({"attention": {"forward_terms": N.attn_terms_fwd(), "input_gradient_terms": N.attn_terms_bwd(),
                                  "note": "M7b flash attention on the 16-bit matrix cores: 3 = three bf16 terms per operand (fp32 "
                                          "operands exactly), 22 = fp16 x 2 (22 significant bits), 2 = two bf16 terms, 0 = fp32 MFMA"}}
                   if args.backbone.startswith("vit_") else {}),
                **({"per_rank": per_rank} if per_rank else {}),
            },
            "roofline": roof,
            "roofline_model": (model_gemm_roofline(N, model, x, dt * 1e3 / K)
                               if (GEMM_TERMS in (2, 3, 22) and not args.no_model_roofline) else None),
        }
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(C, args.backbone)
        if snap is not None:
            dump_outputs(snap, args.dump_outputs)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()  # rank 0 measured the ceilings after the timed region
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
