#!/usr/bin/env python3
"""What a validation costs, at 800 x 800 with 64 + 128 samples, on the analytic scene:

  (i)  validation.validate of ONE frame (eval-semantics render with reflections, TotalLoss, two PSNRs, the panel, one host
       read) beside ONE batched_inference frame of the same rays in the same process -- the existing eval route, the
       yardstick; a validation also keeps the per-sample tensors the loss terms read, so it is expected to cost more;
  (ii) the validation panel through the two launches of frames.val_panel, beside the same (24, 3, H, W) stack assembled from
       torch operations on the device (`panel_torch`, about forty small launches): the alternative to the kernels.  The two
       stacks are compared first.

Method: a host clock around work that ends in a device synchronise, the two routes of a pair alternating, the median of
`--rounds` rounds after a warm-up of both.  Also timed: training steps of 1024 rays on the static route, so that the share of
an epoch that four validations take can be stated: 4 * frames * validate / (rays per epoch / 1024 * step + the same).
Writes one JSON file; needs a GPU (no fall-back).

    python scripts/bench_validation.py --out profiles/validation_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mirror_nerf_amd as M  # noqa: E402
from mirror_nerf_amd import frames, synthetic, training, validation  # noqa: E402
from mirror_nerf_amd.data import RayBank  # noqa: E402


def commit():
    p = os.path.join(ROOT, "mirror_nerf_amd", "BUILD_COMMIT")
    if os.path.exists(p):
        return open(p).read().strip()
    g = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True)
    return g.stdout.strip() if g.returncode == 0 else "unknown"


def timed(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def panel_torch(img_wh, batch, results, table):
    """frames.val_panel from torch operations: the reference's expressions (utils/visualization.py:26-184) left on the device."""
    W, H = img_wh
    chw = lambda t: t.reshape(H, W, 3).permute(2, 0, 1)  # noqa: E731
    tab = table.to(torch.float32) / 255.0

    def depth(d):
        x = torch.nan_to_num(d.reshape(-1))
        mi, ma = x.min(), x.max()
        x = (torch.minimum(torch.maximum(x, mi), ma) - mi) / torch.clamp(ma - mi, min=1e-8)
        return chw(tab[(255 * x).to(torch.uint8).long()])

    def glob(t):
        mn, mx = t.min(), t.max()
        return torch.where(mn == mx, torch.ones_like(t), (t - mn) / (mx - mn))

    out = []
    for name, kind, t in frames.val_panel_tiles(batch, results):
        if kind == M._lib.MNRF_PANEL_COPY:
            out.append(chw(t))
        elif kind == M._lib.MNRF_PANEL_MASK:
            out.append(chw(t.reshape(-1, 1).repeat(1, 3)))
        elif kind == M._lib.MNRF_PANEL_NORMAL:
            out.append(chw((t + 1) / 2))
        elif kind == M._lib.MNRF_PANEL_GLOBAL:
            out.append(chw(glob(t)))
        else:
            out.append(depth(t))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img_wh", nargs=2, type=int, default=[800, 800])
    ap.add_argument("--N_samples", type=int, default=64)
    ap.add_argument("--N_importance", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--train_steps", type=int, default=20, help="training steps per timed round (1024 rays, static route)")
    ap.add_argument("--epoch_frames", type=int, default=100, help="training frames of the epoch the share is stated for")
    ap.add_argument("--val_frames", type=int, default=1, help="validation frames per validation in that statement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validation_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_validation.py measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    W, H = a.img_wh
    hp = training.default_hparams(N_samples=a.N_samples, N_importance=a.N_importance)
    torch.manual_seed(0)
    system = M.NeRFSystem(hp).to(dev)
    _, sds = synthetic.build_models(dev, synthetic.STRADDLE, seed=0)
    system.nerf_coarse.load_state_dict({k: torch.from_numpy(v) for k, v in sds[0].items()})
    system.nerf_fine.load_state_dict({k: torch.from_numpy(v) for k, v in sds[1].items()})
    rng = np.random.default_rng(0)
    masks = np.zeros((1, H, W), np.int8)
    masks[:, H // 4:H // 2, W // 4:W // 2] = 1
    bank = RayBank(synthetic.look_at_pose()[None], rng.integers(0, 256, (1, H, W, 4), dtype=np.uint8), masks,
                   0.5 * W / np.tan(0.5 * synthetic.CAMERA_ANGLE_X), synthetic.NEAR, synthetic.FAR, dev)
    crit = M.get_loss(SimpleNamespace(model_type="nerf"))
    rays = bank.frame(0)["rays"]
    args = dict(predict_normal=True, only_one_field=False, only_one_field_fine_epoch=2, max_recursive_level=1)
    keep = {}

    def validate():
        keep["val"] = validation.validate(system, bank, crit, 5, hp)

    def inference():
        keep["inf"] = M.batched_inference(system.models, system.embeddings, rays, a.N_samples, a.N_importance, False, hp.chunk,
                                          args=args, trace_secondary_rays=True, to_cpu=False, maps_only=True)

    for fn in (validate, inference):
        timed(fn)
    t_val, t_inf = [], []
    for _ in range(a.rounds):
        t_val.append(timed(validate))
        t_inf.append(timed(inference))

    # (ii) the panel on the maps of a validation frame
    with torch.no_grad(), validation._held(system):
        _log, batch, results = validation._step(system, bank.frame(0), crit, 5, hp)
    pb = {k: batch[k] for k in ("rgbs", "mirror_mask")}
    table = frames._table(None, dev)

    def kernels():
        keep["k"] = frames.val_panel((W, H), pb, results)[0]

    def torch_ops():
        keep["t"] = panel_torch((W, H), pb, results, table)

    for fn in (kernels, torch_ops):
        timed(fn, 2)
    diff = (keep["k"] - keep["t"]).abs()
    same = bool(torch.equal(torch.nan_to_num(keep["k"], nan=-7.0), torch.nan_to_num(keep["t"], nan=-7.0)))
    t_k, t_t = [], []
    for _ in range(a.rounds):
        t_k.append(timed(kernels, 10))
        t_t.append(timed(torch_ops, 10))

    # the training step the share is stated against
    opt = torch.optim.Adam(list(system.parameters()), lr=5e-4, fused=True)
    loss_fn = training.total_loss_fn(SimpleNamespace(model_type="nerf"), epoch=5)
    out = (torch.empty(1024, 8, device=dev), torch.empty(1024, 3, device=dev), torch.empty(1024, device=dev))
    state = {"it": 0}

    def steps():
        for _ in range(a.train_steps):
            r, c, m = bank.draw(state["it"], 1024, 0, 0, 1, out=out)
            training.train_step(system, opt, r, c, m, loss_fn, epoch=5, gt_valid=True)
            state["it"] += 1

    timed(steps)
    t_step = [timed(steps) / a.train_steps for _ in range(a.rounds)]

    med = statistics.median
    steps_per_epoch = a.epoch_frames * W * H / 1024.0
    val_ms = 4 * a.val_frames * med(t_val)
    res = dict(commit=commit(), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               what="host clock around work that ends in a device synchronise; the routes of a pair alternate; median of the rounds",
               img_wh=a.img_wh, N_samples=a.N_samples, N_importance=a.N_importance, rounds=a.rounds, precision=M.mirror_nerf.PRECISION,
               validate_one_frame_ms=med(t_val), validate_one_frame_ms_min_max=[min(t_val), max(t_val)],
               batched_inference_one_frame_ms=med(t_inf), batched_inference_one_frame_ms_min_max=[min(t_inf), max(t_inf)],
               validate_over_batched_inference=med(t_val) / med(t_inf),
               panel_tiles=int(keep["k"].shape[0]), panel_kernels_ms=med(t_k), panel_kernels_ms_min_max=[min(t_k), max(t_k)],
               panel_torch_ms=med(t_t), panel_torch_ms_min_max=[min(t_t), max(t_t)], panel_torch_over_kernels=med(t_t) / med(t_k),
               panel_same_as_torch=same, panel_largest_difference=float(torch.nan_to_num(diff, nan=0.0).max()),
               train_step_1024_rays_static_ms=med(t_step), train_step_ms_min_max=[min(t_step), max(t_step)],
               epoch=dict(train_frames=a.epoch_frames, steps=steps_per_epoch, validations=4, val_frames=a.val_frames,
                          validation_share=val_ms / (steps_per_epoch * med(t_step) + val_ms)))
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
