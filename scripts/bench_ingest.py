#!/usr/bin/env python3
"""What bringing the frames of a real capture to the training size on the device costs, per route.  The script writes a seeded
scene of 24 JPEG frames at 1920 x 1440 (PIL) into a temporary directory and times, for the whole scene to 480 x 360:

  (a) decode        the files decoded with PIL on the thread pool, nothing else: the floor of both routes
  (b) host_resize   decode + `resize(img_wh, Image.LANCZOS)` on the pool, the small frames stacked and uploaded: the route of
                    data.read_arkit followed by the RayBank constructor (read_arkit itself decodes serially; the pool is given
                    to this route too, so that the two differ in where the resize runs and in nothing else)
  (c) device_resize decode on the pool, each frame uploaded at its native size and resized by data.resample_lanczos into its
                    slot of the bank's array: the route of RayBank.from_arkit

A host clock runs around work that ends in a device synchronise; every route is warmed up first, then the routes alternate for
`--rounds` rounds and the median is reported with the spread.  The resize kernels alone (the 24 native frames already resident,
one call) are timed with device events.  (c) is compared with (b) measured in the same run, never with itself; the bytes of
both are checked to be equal.  Masks are left out: their resize is a pick per pixel on either route.  At most 16 threads.

    python scripts/bench_ingest.py --out profiles/ingest_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mirror_nerf_amd.data import resample_lanczos  # noqa: E402


def commit():
    p = os.path.join(ROOT, "mirror_nerf_amd", "BUILD_COMMIT")
    if os.path.exists(p):
        return open(p).read().strip()
    g = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True)
    return g.stdout.strip() if g.returncode == 0 else "unknown"


def write_scene(root, frames, native_wh, seed=0):
    """`frames` JPEG files: smooth gradients that differ per frame under seeded noise, so that the files have a photograph's size."""
    from PIL import Image
    w, h = native_wh
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    paths = []
    for k in range(frames):
        base = np.stack([127 + 120 * np.sin(x / (90 + 7 * k) + k), 127 + 120 * np.cos(y / (70 + 5 * k)), (x + y) / (w + h) * 255], -1)
        img = np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)
        paths.append(os.path.join(root, f"frame_{k:04d}.jpg"))
        Image.fromarray(img).save(paths[-1], quality=92)
    return paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--native_wh", type=int, nargs=2, default=(1920, 1440))
    ap.add_argument("--img_wh", type=int, nargs=2, default=(480, 360))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest.py measures on the GPU; none is visible")
    from PIL import Image
    dev = torch.device("cuda", 0)
    wh = tuple(a.img_wh)
    threads = max(1, min(16, a.threads))
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=threads) as pool:
        paths = write_scene(tmp, a.frames, tuple(a.native_wh))
        file_bytes = sum(os.path.getsize(p) for p in paths)

        def decode(p):
            return np.asarray(Image.open(p), dtype=np.uint8)

        def decode_resize(p):
            return np.asarray(Image.open(p).resize(wh, Image.LANCZOS), dtype=np.uint8)

        def route_a():
            return list(pool.map(decode, paths))

        def route_b():
            out = torch.from_numpy(np.stack(list(pool.map(decode_resize, paths)))).to(dev)
            torch.cuda.synchronize()
            return out

        def route_c():
            out = torch.empty(len(paths), wh[1], wh[0], 3, dtype=torch.uint8, device=dev)
            for f, img in enumerate(pool.map(decode, paths)):
                resample_lanczos(torch.from_numpy(img).to(dev)[None], wh, out=out[f:f + 1])
            torch.cuda.synchronize()
            return out

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3

        same = bool(torch.equal(route_b(), route_c()))          # also the warm-up of (b) and (c)
        route_a()
        t = {"decode": [], "host_resize": [], "device_resize": []}
        for _ in range(a.rounds):
            t["decode"].append(timed(route_a))
            t["host_resize"].append(timed(route_b))
            t["device_resize"].append(timed(route_c))

        # the kernels alone: the native frames resident, one call over the stack, device events
        native = torch.from_numpy(np.stack(route_a())).to(dev)
        out = torch.empty(len(paths), wh[1], wh[0], 3, dtype=torch.uint8, device=dev)
        resample_lanczos(native, wh, out=out)
        kernel_ms = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            resample_lanczos(native, wh, out=out)
            e1.record()
            e1.synchronize()
            kernel_ms.append(e0.elapsed_time(e1))
        kernels_same = bool(torch.equal(out, route_b()))

    res = dict(commit=commit(), device=torch.cuda.get_device_name(0), torch=torch.__version__, pillow=Image.__version__,
               frames=a.frames, native_wh=list(a.native_wh), img_wh=list(wh), threads=threads, rounds=a.rounds, jpeg_bytes=file_bytes,
               what="ms for the whole scene; host clock around work that ends in a device synchronise; median over alternating rounds",
               same_bytes_host_and_device_route=same and kernels_same,
               resize_kernels_ms=statistics.median(kernel_ms), resize_kernels_ms_min_max=[min(kernel_ms), max(kernel_ms)],
               resize_kernels_source_bytes=int(native.numel()))
    for k, v in t.items():
        res[k + "_ms"] = statistics.median(v)
        res[k + "_ms_min_max"] = [min(v), max(v)]
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
