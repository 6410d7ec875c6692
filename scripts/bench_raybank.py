#!/usr/bin/env python3
"""What producing a training batch of 1024 rays costs: RayBank.draw (one launch over frames kept as bytes) against the route
of scripts/train_scene.py (a torch.randint, three indexed gathers over float ray / colour / mask arrays of the same frames and
three copy_ into the step's buffers), for (a) 48 frames of 100 x 100 and (b) 100 frames of 800 x 800 of seeded random bytes.

Per case the two routes alternate in rounds; a round times `--steps` batches with a host clock around work that ends in a
device synchronise (what is measured is what a training loop pays per step: launches and host work included), after a
warm-up of every shape.  Reported: the median over the rounds and their spread, the bytes resident for each route, and that the
two routes give the same batch for the same indices.  Writes one JSON file; needs a GPU (no fall-back).

    python scripts/bench_raybank.py --out profiles/raybank_bench.json
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

from mirror_nerf_amd.data import RayBank  # noqa: E402
from mirror_nerf_amd import synthetic as SY  # noqa: E402

CASES = {"a_48x100x100": (48, 100, 100), "b_100x800x800": (100, 800, 800)}


def commit():
    p = os.path.join(ROOT, "mirror_nerf_amd", "BUILD_COMMIT")
    if os.path.exists(p):
        return open(p).read().strip()
    g = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True)
    return g.stdout.strip() if g.returncode == 0 else "unknown"


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(steps):
        fn(s)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def run_case(name, F, H, W, batch, steps, rounds, dev):
    import numpy as np
    g = torch.Generator(device=dev).manual_seed(1)
    images = torch.randint(0, 256, (F, H, W, 4), dtype=torch.uint8, device=dev, generator=g)
    masks = torch.randint(0, 2, (F, H, W), device=dev, generator=g).to(torch.int8)
    rng = np.random.default_rng(0)
    poses = np.stack([SY.look_at_pose(eye=(float(rng.uniform(-3, 3)), float(rng.uniform(-4, -2)), float(rng.uniform(1, 3)))) for _ in range(F)])
    bank = RayBank(poses, images, masks, 0.5 * W / np.tan(0.5 * SY.CAMERA_ANGLE_X), SY.NEAR, SY.FAR, dev)
    # the parent route's arrays: every ray of every frame as float32 (12 floats per ray), made by the bank frame by frame
    rays_t = torch.empty(bank.n_rays, 8, device=dev)
    rgbs_t = torch.empty(bank.n_rays, 3, device=dev)
    masks_t = torch.empty(bank.n_rays, device=dev)
    hw = H * W
    for f in range(F):
        d = bank.frame(f)
        rays_t[f * hw:(f + 1) * hw], rgbs_t[f * hw:(f + 1) * hw], masks_t[f * hw:(f + 1) * hw] = d["rays"], d["rgbs"], d["mirror_mask"]
    out = (torch.zeros(batch, 8, device=dev), torch.zeros(batch, 3, device=dev), torch.zeros(batch, device=dev))
    out2 = tuple(torch.zeros_like(t) for t in out)
    gen = torch.Generator(device=dev).manual_seed(1)

    def draw(s):
        bank.draw(s, batch, 0, 0, 1, out=out)

    def parent(s):          # scripts/train_scene.py:93-97 with GraphedTrainStep.__call__'s three copies
        idx = torch.randint(0, rays_t.shape[0], (batch,), device=dev, generator=gen)
        out2[0].copy_(rays_t[idx])
        out2[1].copy_(rgbs_t[idx])
        out2[2].copy_(masks_t[idx])

    # same indices, same batch (bit for bit)
    idx = bank.draw(3, batch, 0, 0, 1, out=out, return_indices=True)[3]
    same = bool(torch.equal(out[0], rays_t[idx]) and torch.equal(out[1], rgbs_t[idx]) and torch.equal(out[2], masks_t[idx]))
    for fn in (draw, parent):
        timed(fn, 500)
    t_draw, t_parent = [], []
    for _ in range(rounds):
        t_draw.append(timed(draw, steps))
        t_parent.append(timed(parent, steps))
    res = dict(frames=F, H=H, W=W, channels=4, batch=batch, steps_per_round=steps, rounds=rounds,
               draw_ms=statistics.median(t_draw), draw_ms_min_max=[min(t_draw), max(t_draw)],
               parent_route_ms=statistics.median(t_parent), parent_route_ms_min_max=[min(t_parent), max(t_parent)],
               bank_bytes_resident=bank.bytes_resident(),
               parent_route_bytes_resident=sum(t.numel() * t.element_size() for t in (rays_t, rgbs_t, masks_t)),
               same_batch_for_same_indices=same)
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20000, help="batches per timed round (a round is 0.1-1 s)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raybank_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_raybank.py measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    res = dict(commit=commit(), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               what="ms per batch, host clock around `steps` batches ending in a device synchronise; median over alternating rounds",
               cases={n: run_case(n, *CASES[n], a.batch, a.steps, a.rounds, dev) for n in a.cases})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
