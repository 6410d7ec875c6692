#!/usr/bin/env python3
"""What the output stage of a test frame costs, from "the float maps of the frame are on the device" to "every 8-bit image of
the frame is in pinned host memory", for one 800 x 800 frame of seeded maps:

  device  frames.finish_frame (the extrema launch and the finish launch), the seven uint8 images concatenated on the device
          and ONE copy into a pinned buffer
  host    what a user of `to_cpu="maps"` does today: the seven float maps copied into pinned buffers (as recursion.py stages
          them), then the reference's expressions in numpy on the host (tests/frames_ref.py, the restatement of
          eval.py:743-894)

The two routes alternate in rounds; a round times `--frames` frames with a host clock around work that ends in a device
synchronise, after a warm-up of both.  Reported: the median over the rounds and their spread, the bytes each route moves over
PCIe per frame, and that the two routes give the same bytes.  PNG encoding is host work common to both and is not part of
either figure.  Writes one JSON file; needs a GPU (no fall-back).

    python scripts/bench_frames.py --out profiles/frames_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mirror_nerf_amd import frames  # noqa: E402

KEYS = {"rgb": "rgb_fine", "mirror_mask": "mirror_mask_fine", "depth": "depth_fine", "depth_reflect": "depth_fine_reflect",
        "surface_normal": "surface_normal_fine", "surface_normal_grad": "surface_normal_grad_fine", "x_surface": "x_surface_fine"}


def commit():
    p = os.path.join(ROOT, "mirror_nerf_amd", "BUILD_COMMIT")
    if os.path.exists(p):
        return open(p).read().strip()
    g = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True)
    return g.stdout.strip() if g.returncode == 0 else "unknown"


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img_wh", nargs=2, type=int, default=[800, 800])
    ap.add_argument("--frames", type=int, default=5, help="frames per timed round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames.py measures on the GPU; none is visible")
    from tests import frames_ref as FR
    dev = torch.device("cuda", 0)
    n = a.img_wh[0] * a.img_wh[1]
    maps = FR.seeded_maps(n, seed=0, nonfinite="nan")
    results = {KEYS[k]: torch.from_numpy(v).to(dev) for k, v in maps.items()}
    table = frames.jet_table()
    table_dev = torch.from_numpy(table).to(dev)

    float_bytes = sum(v.numel() * 4 for v in results.values())
    pinned_u8 = torch.empty(7 * n * 3, dtype=torch.uint8).pin_memory()
    pinned_f = {k: torch.empty(v.shape, dtype=torch.float32).pin_memory() for k, v in results.items()}
    last = {}

    def device_route():
        images = frames.finish_frame(results, "fine", table=table_dev)
        flat = torch.cat([v.reshape(-1) for v in images.values()])
        pinned_u8[:flat.numel()].copy_(flat, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        last["device"] = (list(images), flat.numel())

    def host_route():
        for k, v in results.items():
            pinned_f[k].copy_(v, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        last["host"] = FR.frame_images({k: v.numpy() for k, v in pinned_f.items()}, table)

    for fn in (device_route, host_route):
        timed(fn, 2)
    names, total = last["device"]
    got = pinned_u8[:total].numpy().reshape(len(names), n, 3)
    same = all((got[i] == last["host"][k]).all() for i, k in enumerate(names))
    t_dev, t_host = [], []
    for _ in range(a.rounds):
        t_dev.append(timed(device_route, a.frames))
        t_host.append(timed(host_route, a.frames))
    res = dict(commit=commit(), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               what="ms per frame from 'float maps on the device' to 'all 8-bit images in pinned host memory'; host clock around "
                    "`frames` frames ending in a device synchronise; median over alternating rounds; PNG encoding excluded",
               img_wh=a.img_wh, images=names, frames_per_round=a.frames, rounds=a.rounds,
               device_route_ms=statistics.median(t_dev), device_route_ms_min_max=[min(t_dev), max(t_dev)],
               host_route_ms=statistics.median(t_host), host_route_ms_min_max=[min(t_host), max(t_host)],
               device_route_pcie_bytes=int(total), host_route_pcie_bytes=int(float_bytes),
               same_bytes_on_both_routes=bool(same))
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
