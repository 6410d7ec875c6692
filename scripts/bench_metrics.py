#!/usr/bin/env python3
"""Times structural similarity of an 800x800x3 frame and of a stack of 20 such frames three ways (one JSON line):

    python scripts/bench_metrics.py [--repeats 30] [--warmup 5] [--out profiles/metrics_bench.json]

  hip     metrics.structural_similarity: the windowed-moments kernel and its finish kernel (csrc/mnrf_metrics.hip)
  torch   the same formula in float64 torch operations on the same GPU: avg_pool2d over x, y, x^2, y^2, xy, then S and the
          mean -- the only fair yardstick on the device
  host    the status quo: the frame copied to the host, then the float64 numpy restatement of tests/ssim_ref.py there
Milliseconds of host time around work that ends in torch.cuda.synchronize(), the median of `repeats` (host: `host_repeats`)
runs after `warmup` untimed ones, with the extremes.  `hip_launch_pair_events_ms` is the time between two torch.cuda.Event
records around one direct mnrf_ssim call on pre-allocated buffers: the two launches with the gap between them, not the
kernels alone.  The three routes are also compared: `abs_diff_*` is |hip - route| on the timed inputs.

The kernels' own time comes from a profiler run, which is a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_metrics.py --profile 30
    python scripts/bench_metrics.py --reduce_trace DIR --out profiles/metrics_bench.json

`--profile N` only launches (N times the frame, then N times the stack); `--reduce_trace` reads the kernel trace, takes the
median duration of ssim_tile_kernel and ssim_finish_kernel per grid size (the frame's launch and the stack's differ in
nothing else) and adds `kernel_trace` to the JSON of --out: microseconds, registers and LDS as the trace reports them, and
`tile_bytes_per_s` = the 2 x 7.68 MB of float32 that a frame's two images hold, per frame, over the tile kernel's time.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_route(pred, gt, win_size=7):
    """(F, H, W, C) float32 -> (F,) float32; float64 throughout, one avg_pool2d over the five products."""
    import torch
    x, y = pred.permute(0, 3, 1, 2).double(), gt.permute(0, 3, 1, 2).double()
    F, C = x.shape[:2]
    m = torch.nn.functional.avg_pool2d(torch.cat([x, y, x * x, y * y, x * y], 1), win_size, stride=1)
    ux, uy, uxx, uyy, uxy = m.split(C, 1)
    n = win_size * win_size
    cov, c1, c2 = n / (n - 1.0), 1e-4, 9e-4
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    S = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return S.mean((1, 2, 3)).float()


def reduce_trace(root, out, size):
    """Median duration per (kernel, grid) of the ssim kernels in a rocprofv3 kernel trace; merged into the JSON of `out`."""
    import csv
    import glob
    rows = []
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += [r for r in csv.DictReader(fh) if "ssim_" in r["Kernel_Name"]]
    if not rows:
        raise SystemExit(f"no ssim kernel in a *kernel_trace.csv under {root}")
    groups = {}
    for r in rows:
        name = "ssim_tile_kernel" if "ssim_tile" in r["Kernel_Name"] else "ssim_finish_kernel"
        groups.setdefault((name, int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])), []).append(r)
    frame_bytes = 2 * size * size * 3 * 4
    smallest = {n: min(g for (m, g) in groups if m == n) for n in ("ssim_tile_kernel", "ssim_finish_kernel")}
    res = {}
    for (name, wgs), rs in sorted(groups.items()):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rs]
        frames = wgs // smallest[name]
        e = dict(workgroups=wgs, frames=frames, dispatches=len(us), median_us=round(statistics.median(us), 3),
                 minmax_us=[min(us), max(us)], vgprs=int(rs[0].get("VGPR_Count", 0) or 0),
                 lds_bytes=int(rs[0].get("LDS_Block_Size", 0) or 0), scratch_bytes=int(rs[0].get("Scratch_Size", 0) or 0))
        if name == "ssim_tile_kernel":
            e["tile_bytes_per_s"] = frames * frame_bytes / (e["median_us"] * 1e-6)
        res[f"{name}/{'frame' if frames == 1 else 'stack%d' % frames}"] = e
    line = {}
    if out and os.path.exists(out):
        with open(out) as f:
            line = json.loads(f.read())
    line["kernel_trace"] = res
    text = json.dumps(line)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host_repeats", type=int, default=20)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--stack", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--profile", type=int, default=0, metavar="N", help="only launch the HIP route N times per shape (for rocprofv3)")
    ap.add_argument("--reduce_trace", type=str, default=None, metavar="DIR", help="add the kernel times of a rocprofv3 run to --out")
    args = ap.parse_args()
    if args.reduce_trace:
        return reduce_trace(args.reduce_trace, args.out, args.size)
    if min(args.repeats, args.host_repeats) < 20:
        raise SystemExit("at least 20 timed runs")
    import ctypes
    import numpy as np
    import torch
    from mirror_nerf_amd import _lib, metrics
    from tests import ssim_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py measures on the GPU only")
    dev = "cuda:0"
    H = W = args.size
    pairs = [R.pair(R.KINDS[i % 4], H, W, seed=i) for i in range(args.stack)]
    sp = torch.from_numpy(np.stack([p for p, _ in pairs])).to(dev)
    st = torch.from_numpy(np.stack([t for _, t in pairs])).to(dev)
    shapes = (("frame", sp[:1], st[:1]), (f"stack{args.stack}", sp, st))
    if args.profile:
        for _, p, t in shapes:
            for _ in range(args.profile):
                metrics.structural_similarity(p, t)
            torch.cuda.synchronize()
        return

    def timed(fn, repeats, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), [min(ts), max(ts)]

    def launch_pair_ms(p, t):
        """Events around mnrf_ssim itself: buffers, strides and taps are made once, outside."""
        L = _lib.lib()
        F, C = p.shape[0], p.shape[3]
        strides = [(ctypes.c_int64 * 4)(v.stride(2), v.stride(1), v.stride(3), v.stride(0)) for v in (p, t)]
        taps = (ctypes.c_double * 7)(*([1.0 / 7] * 7))
        part = torch.empty(L.mnrf_ssim_blocks(H, W, F, C), dtype=torch.float64, device=dev)
        out = torch.empty(F, dtype=torch.float32, device=dev)
        stream = _lib.stream()
        ts = []
        for it in range(args.warmup + args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(L.mnrf_ssim(p.data_ptr(), strides[0], t.data_ptr(), strides[1], H, W, C, F, taps, 3, 0, 49.0 / 48.0, 1e-4,
                                   9e-4, part.data_ptr(), _lib.ptr(out), None, stream), "mnrf_ssim")
            e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                ts.append(e0.elapsed_time(e1))
        assert torch.equal(out, metrics.structural_similarity(p, t))
        return statistics.median(ts)

    def host_route(p, t):
        a, b = p.cpu().numpy(), t.cpu().numpy()
        return [R.structural_similarity(a[f], b[f]) for f in range(a.shape[0])]

    line = dict(metric="structural_similarity_routes", size=[H, W, 3], win_size=7, repeats=args.repeats, warmup=args.warmup,
                host_repeats=args.host_repeats, device=torch.cuda.get_device_name(0))
    frame_bytes = 2 * H * W * 3 * 4
    for label, p, t in shapes:
        F = p.shape[0]
        hip, hip_mm = timed(lambda: metrics.structural_similarity(p, t), args.repeats, args.warmup)
        tor, tor_mm = timed(lambda: torch_route(p, t), args.repeats, args.warmup)
        host, host_mm = timed(lambda: host_route(p, t), args.host_repeats, 1)
        k = launch_pair_ms(p, t)
        got = metrics.structural_similarity(p, t).cpu().numpy().astype(np.float64)
        line[label] = dict(frames=F, hip_ms=round(hip, 4), hip_minmax_ms=hip_mm, hip_launch_pair_events_ms=round(k, 4),
                           torch_f64_ms=round(tor, 4), torch_f64_minmax_ms=tor_mm, host_copy_numpy_ms=round(host, 2),
                           host_copy_numpy_minmax_ms=host_mm, read_bytes=F * frame_bytes,
                           hip_call_bytes_per_s=F * frame_bytes / (hip * 1e-3), torch_over_hip=tor / hip, host_over_hip=host / hip,
                           abs_diff_torch=float(np.max(np.abs(got - torch_route(p, t).cpu().numpy()))),
                           abs_diff_host=float(np.max(np.abs(got - np.array(host_route(p, t))))))
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
