#!/usr/bin/env python3
"""The benchmark's frame (bench.py: 800x800 rays, 64 + 128 samples, one bounce, chunk 32768, maps on the device) with the models
of another synthetic scene: `--weights opaque` (synthetic.OPAQUE: no ray a mirror), `straddle` (about 40 % of the rays) or
`bench` (the benchmark's own: every ray).  Prints one JSON line: ms per frame of each timed frame, and how many level-0 fine
launches of the last frame took the blended-level launch.  `--tree DIR` imports the package from another checkout (A/B)."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--weights", choices=["bench", "opaque", "straddle"], default="opaque")
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))

import torch  # noqa: E402
import bench  # noqa: E402
import mirror_nerf_amd as M  # noqa: E402
from mirror_nerf_amd import mirror_nerf as MN, synthetic as SY  # noqa: E402

dev = torch.device("cuda", 0)
models, _sds, emb = bench.build_models(dev)
if a.weights != "bench":
    models = SY.build_models(dev, SY.OPAQUE if a.weights == "opaque" else SY.STRADDLE, seed=0)[0]
rays = SY.device_rays(800, 800, dev)
ms = []
for it in range(a.warmup + a.steps):
    MN.LAUNCH_LOG = [] if it == a.warmup + a.steps - 1 else None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    M.batched_inference(models, emb, rays, bench.N_SAMPLES, bench.N_IMPORTANCE, False, bench.CHUNK, args=bench.ARGS,
                        trace_secondary_rays=True, to_cpu=False)
    torch.cuda.synchronize()
    if it >= a.warmup:
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
fine = [f for f, _B, _e0, _e1 in MN.LAUNCH_LOG if not f & 1]
MN.LAUNCH_LOG = None
print(json.dumps({"weights": a.weights, "tree": os.path.abspath(a.tree), "ms_per_frame": ms,
                  "fine_launches": len(fine), "blended_level_launches": sum(bool(f & 0x8000) for f in fine)}))
