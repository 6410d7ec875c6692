#!/usr/bin/env python3
"""Train the MirrorNeRF pair from a Blender-format directory (datasets/blender.py's layout: transforms_train.json, the frames'
PNGs, masks/MirrorMask_*.png) ON THE GPU: the frames are read once (data.read_blender), kept on the device as decoded bytes
(data.RayBank) and every batch is ONE launch that draws from a shuffled stream visiting each ray once per epoch -- no host
ray arrays, no DataLoader, no per-step host-to-device copy.  On the graph route the draw writes straight into the captured
step's static buffers.  The weights are written as scripts/train_scene.py writes them (coarse__* / fine__* arrays).

With --dataset_name real_arkit the directory is a real capture (datasets/real_arkit.py's layout): the poses are centred with the
average pose of transforms.json and divided by --scale_factor, and the frames are resized on the device as they enter the bank
(RayBank.from_arkit).

    python scripts/train_blender.py --root_dir data/scene --img_wh 400 400 --near 2 --far 6 --steps 20000 --route graph --out weights.npz
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mirror_nerf_amd as M  # noqa: E402
from mirror_nerf_amd import dist, training  # noqa: E402
from mirror_nerf_amd.data import RayBank  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root_dir", required=True)
    ap.add_argument("--img_wh", type=int, nargs=2, default=(800, 800))
    ap.add_argument("--near", type=float, default=2.0)
    ap.add_argument("--far", type=float, default=6.0)
    ap.add_argument("--train_skip_step", type=int, default=1)
    ap.add_argument("--dataset_name", choices=("blender", "real_arkit"), default="blender")
    ap.add_argument("--scale_factor", type=float, default=1.0, help="real_arkit: translations, near and far are divided by it")
    ap.add_argument("--val_idx", type=int, default=0, help="real_arkit: accepted as the reference's option; the train split does not use it")
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--lr", type=float, default=5e-4)
    ap.add_argument("--seed", type=int, default=0, help="of the weights and of the shuffled stream")
    ap.add_argument("--route", choices=("host", "static", "graph"), default="host",
                    help="host = the reference's control flow (reads the reflected-ray count on the host); static = the count stays on the "
                         "device; graph = the whole step replayed as one hipGraph (training.GraphedTrainStep), the draw writing into its buffers")
    ap.add_argument("--loss", choices=("total", "color_mask"), default="total")
    ap.add_argument("--geometry_epochs", type=int, default=0,
                    help="epochs of the geometry stage at the start (--train_geometry_stage): no reflections, frames with a valid mask only")
    ap.add_argument("--precision", default="split")
    ap.add_argument("--out", default="blender_weights.npz", help="where the weights are written")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    M.set_precision(a.precision)
    torch.manual_seed(a.seed)
    hp = training.default_hparams(N_importance=64, train_geometry_stage_end_epoch=a.geometry_epochs)
    system = M.NeRFSystem(hp).to(dev)
    if a.dataset_name == "real_arkit":
        full = RayBank.from_arkit(a.root_dir, "train", tuple(a.img_wh), a.near, a.far, a.scale_factor, a.val_idx, a.train_skip_step,
                                  device=dev)
    else:
        full = RayBank.from_blender(a.root_dir, "train", tuple(a.img_wh), a.near, a.far, a.train_skip_step, device=dev)
    print(f"{full.n_frames} frames of {full.W}x{full.H}x{full.channels}, {len(full.frames_with_mask)} with a mirror mask; "
          f"{full.bytes_resident() / 1e6:.2f} MB resident ({full.n_rays * 48 / 1e6:.2f} MB as float rays)", flush=True)
    if a.geometry_epochs > 0 and not full.frames_with_mask:
        raise SystemExit("--geometry_epochs: no frame of this dataset has a mirror mask")

    rank, world = dist.world()
    gamma = 0.1 ** (1.0 / max(1, a.steps))
    if a.route == "graph":
        opt = training.FlatAdam(list(system.models.values()), lr=a.lr)
    else:
        opt = torch.optim.Adam(list(system.parameters()), lr=a.lr, fused=True)

    def setup(epoch):
        """The bank, the loss and the validity statement of an epoch (the stage's frames all have a valid mask)."""
        stage = epoch < a.geometry_epochs
        system.train_geometry_stage = stage
        bank = full.select("with_mask") if stage else full
        loss_fn = training.total_loss_fn(SimpleNamespace(model_type="nerf"), epoch=epoch, train_geometry_stage=stage) if a.loss == "total" \
            else training.color_mask_loss
        return bank, loss_fn, (stage or len(full.frames_with_mask) == full.n_frames)

    # the epoch is the stream's: every ray of the bank once.  The stage's bank is a subset, so its epochs are shorter; where the
    # selection changes the stream starts again at position 0 of the new bank (`first`, `epoch_first`)
    epoch, first, epoch_first = 0, 0, 0
    bank, loss_fn, gt_valid = setup(0)
    graphed = training.GraphedTrainStep(system, opt, a.batch, loss_fn, epoch=0, gt_valid=gt_valid) if a.route == "graph" else None
    if graphed is not None:
        out = (graphed.rays, graphed.target, graphed.gt)
    else:
        out = (torch.empty(a.batch, 8, device=dev), torch.empty(a.batch, 3, device=dev), torch.empty(a.batch, device=dev))
    t0 = time.time()
    loss = None
    for it in range(a.steps):
        e = epoch_first + bank.epoch_of(it - first, a.batch, world)
        if e != epoch:
            epoch, n_before = e, bank.n_rays
            bank, loss_fn, gt_valid = setup(epoch)
            if bank.n_rays != n_before:
                first, epoch_first = it, epoch
            if graphed is not None and graphed.gt_valid != gt_valid:
                graphed = training.GraphedTrainStep(system, opt, a.batch, loss_fn, epoch=epoch, gt_valid=gt_valid)
                out = (graphed.rays, graphed.target, graphed.gt)
            elif graphed is not None:
                graphed.set_epoch(epoch, loss_fn)
        rays, rgbs, mask = bank.draw(it - first, a.batch, a.seed, rank, world, out=out)
        if graphed is not None:
            loss = graphed(rays, rgbs, mask)          # the step's own buffers: its copy_ of a tensor onto itself is a no-op
        else:
            loss = training.train_step(system, opt, rays, rgbs, mask, loss_fn, epoch=epoch, gt_valid=gt_valid if a.route == "static" else None)
        opt.param_groups[0]["lr"] *= gamma
        if it % 1000 == 0 or it == a.steps - 1:
            print(f"step {it:6d}  epoch {epoch}  loss {loss.item():.4f}  [{time.time() - t0:.0f} s]", flush=True)
    arrs = {}
    for mname, mod in (("coarse", system.nerf_coarse), ("fine", system.nerf_fine)):
        for k, v in mod.state_dict().items():
            arrs[f"{mname}__{k}"] = v.detach().cpu().numpy().copy()
    arrs["meta"] = np.array(json.dumps(dict(steps=a.steps, batch=a.batch, lr=a.lr, root_dir=os.path.abspath(a.root_dir), img_wh=list(a.img_wh),
                                            frames=full.n_frames, route=a.route, loss=a.loss, seed=a.seed, epochs=epoch + 1,
                                            final_loss=None if loss is None else float(loss.item()),
                                            trained_with="mirror_nerf_amd (scripts/train_blender.py), precision " + a.precision)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **arrs)
    print("wrote", a.out, f"{os.path.getsize(a.out) / 1e6:.1f} MB; ms/step {(time.time() - t0) / max(1, a.steps) * 1e3:.2f}")


if __name__ == "__main__":
    main()
