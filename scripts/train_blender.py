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

The validation half of the reference's loop (train.py:460-564, 574) is opt-in; without these options a run is what it was:
  --val_every F    validate every F-th of an epoch (the reference's val_check_interval is 0.25) on the frames of
                   transforms_val.json / the ARKit `val` split (--val_frames picks some of them), between two steps on the same
                   stream; a captured step is kept and replayed afterwards (mirror_nerf_amd/validation.py)
  --log_dir D      val.jsonl, one line per validation with the reference's val/* names, and val_panel_{step}.png, the
                   val/GT_pred_depth panel of the first validation frame as a grid (val_panel_{step}.json names the tiles)
  --ckpt_dir D     epoch={epoch}.ckpt (Lightning's file name for the reference's filename="{epoch:d}") and last.ckpt at the end
                   of every epoch and of the run, resumable (checkpoint.save_training_state); best.json says which epoch had
                   the best val/psnr
  --resume PATH    continue such a checkpoint: weights, optimizer, learning rate, gradient-scale state, the position in the
                   shuffled stream and the generators; --steps stays the TOTAL, so K steps + a resumed run to 2K is a 2K run

The reference's optimizers and learning-rate schedules (opt.py:106-153, utils/__init__.py:47-101) are opt-in as well; without
these options the run keeps Adam and its own decay, lr *= 0.1 ** (1 / steps) after every step:
  --optimizer sgd|adam|radam   with --momentum and --weight_decay; on the graph route training.FlatSGD / FlatAdam / FlatRAdam
                   (the HIP kernels), on the other routes torch's optimizer.  `ranger` is refused (torch_optimizer's
                   Lookahead-RAdam is not part of this package)
  --lr_scheduler steplr|cosine|poly   with --decay_step, --decay_gamma, --poly_exp, --warmup_epochs, --warmup_multiplier and
                   --num_epochs (mirror_nerf_amd/schedules.py): the rate is set at every epoch boundary of the stream, as
                   Lightning steps an epoch-interval scheduler, and is constant within an epoch.  run.sh:259-280's recipe is
                   --optimizer adam --lr_scheduler steplr --decay_step 2 4 8 --decay_gamma 0.5 --num_epochs 30
  --num_epochs N   the run ends with epoch N - 1 (or with --steps, whichever comes first)
The schedule's options and position travel in the checkpoint; --resume refuses another schedule or optimizer.
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
from mirror_nerf_amd import checkpoint, dist, training  # noqa: E402
from mirror_nerf_amd.data import RayBank  # noqa: E402


def save_panel(path, stack, names):
    """The (N, 3, H, W) panel as one PNG: the tiles in a grid, row-major in the reference's order, a one-pixel gap between them
    (PIL; the 8-bit cast is the output stage's: clip to [0, 1], times 255, truncated).  The tile names go beside it as JSON."""
    from PIL import Image
    n, _, h, w = stack.shape
    cols = int(np.ceil(np.sqrt(n)))
    rows = (n + cols - 1) // cols
    tiles = (stack.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()      # a NaN tile casts to 0
    grid = np.zeros((rows * (h + 1) - 1, cols * (w + 1) - 1, 3), np.uint8)
    for i in range(n):
        r, c = divmod(i, cols)
        grid[r * (h + 1):r * (h + 1) + h, c * (w + 1):c * (w + 1) + w] = tiles[i]
    Image.fromarray(grid).save(path)
    with open(os.path.splitext(path)[0] + ".json", "w") as f:
        json.dump({"names": names, "cols": cols, "rows": rows, "tile_wh": [w, h], "gap": 1}, f)


def main(argv=None):
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
    ap.add_argument("--val_every", type=float, default=0.0, help="validate every this fraction of an epoch (the reference: 0.25); 0 = never")
    ap.add_argument("--val_frames", type=int, nargs="*", default=None, help="frames of the validation split to validate on (default: all)")
    ap.add_argument("--ckpt_dir", default=None, help="epoch={epoch}.ckpt and last.ckpt every epoch, best.json (train.py:554-564)")
    ap.add_argument("--resume", default=None, help="a checkpoint of --ckpt_dir to continue (train.py:574)")
    ap.add_argument("--trusted", action="store_true", help="--resume: unpickle the checkpoint fully (only for files you wrote)")
    ap.add_argument("--log_dir", default=None, help="val.jsonl and the validation panels")
    ap.add_argument("--optimizer", choices=("sgd", "adam", "radam", "ranger"), default="adam")
    ap.add_argument("--momentum", type=float, default=0.9, help="--optimizer sgd")
    ap.add_argument("--weight_decay", type=float, default=0.0)
    ap.add_argument("--lr_scheduler", choices=("steplr", "cosine", "poly"), default=None,
                    help="the reference's epoch schedules (default: none of them, lr *= 0.1 ** (1 / steps) after every step)")
    ap.add_argument("--decay_step", type=int, nargs="+", default=[20], help="steplr: the epochs at which the rate drops")
    ap.add_argument("--decay_gamma", type=float, default=0.1, help="steplr: by this factor")
    ap.add_argument("--poly_exp", type=float, default=0.9)
    ap.add_argument("--warmup_epochs", type=int, default=0, help="linear warm-up over this many epochs (sgd and adam only)")
    ap.add_argument("--warmup_multiplier", type=float, default=1.0, help="the rate reaches lr times this at the end of the warm-up")
    ap.add_argument("--num_epochs", type=int, default=None, help="end the run with epoch N - 1; T_max of cosine, the end of poly (default there: 16)")
    a = ap.parse_args(argv)
    if a.val_every < 0:
        raise SystemExit("--val_every must not be negative")
    if a.optimizer == "ranger":
        raise SystemExit("--optimizer ranger: torch_optimizer's Ranger (Lookahead around RAdam) is not part of this package and there is "
                         "no implementation here to hold one against; use sgd, adam or radam")
    if a.num_epochs is not None and a.num_epochs < 1:
        raise SystemExit("--num_epochs must be at least 1")
    sched = None
    if a.lr_scheduler is not None:
        from mirror_nerf_amd.schedules import lr_schedule
        try:
            sched = lr_schedule(SimpleNamespace(lr=a.lr, lr_scheduler=a.lr_scheduler, decay_step=a.decay_step, decay_gamma=a.decay_gamma,
                                                num_epochs=16 if a.num_epochs is None else a.num_epochs, poly_exp=a.poly_exp,
                                                warmup_epochs=a.warmup_epochs, warmup_multiplier=a.warmup_multiplier, optimizer=a.optimizer))
        except ValueError as e:
            raise SystemExit(str(e))
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
        if a.optimizer == "adam":
            opt = training.FlatAdam(list(system.models.values()), lr=a.lr, weight_decay=a.weight_decay)
        elif a.optimizer == "sgd":
            opt = training.FlatSGD(list(system.models.values()), lr=a.lr, momentum=a.momentum, weight_decay=a.weight_decay)
        else:
            opt = training.FlatRAdam(list(system.models.values()), lr=a.lr, weight_decay=a.weight_decay)
    elif a.optimizer == "adam":
        opt = torch.optim.Adam(list(system.parameters()), lr=a.lr, weight_decay=a.weight_decay, fused=True)
    elif a.optimizer == "sgd":
        opt = torch.optim.SGD(list(system.parameters()), lr=a.lr, momentum=a.momentum, weight_decay=a.weight_decay, fused=True)
    else:
        opt = torch.optim.RAdam(list(system.parameters()), lr=a.lr, eps=1e-8, weight_decay=a.weight_decay)

    def setup(epoch):
        """The bank, the loss and the validity statement of an epoch (the stage's frames all have a valid mask)."""
        stage = epoch < a.geometry_epochs
        system.train_geometry_stage = stage
        bank = full.select("with_mask") if stage else full
        loss_fn = training.total_loss_fn(SimpleNamespace(model_type="nerf"), epoch=epoch, train_geometry_stage=stage) if a.loss == "total" \
            else training.color_mask_loss
        return bank, loss_fn, (stage or len(full.frames_with_mask) == full.n_frames)

    val_bank = val_loss = None
    if a.val_every > 0:
        from mirror_nerf_amd import get_loss, validation
        if a.dataset_name == "real_arkit":
            val_bank = RayBank.from_arkit(a.root_dir, "val", tuple(a.img_wh), a.near, a.far, a.scale_factor, a.val_idx, device=dev)
        else:
            val_bank = RayBank.from_blender(a.root_dir, "val", tuple(a.img_wh), a.near, a.far, device=dev)
        val_loss = get_loss(SimpleNamespace(model_type="nerf"))
    for d in (a.ckpt_dir, a.log_dir):
        if d:
            os.makedirs(d, exist_ok=True)
    best = {"monitor": "val/psnr", "best_epoch": None, "best_score": None}
    last_val = [None]

    def validate_now(step):
        """train.py:460-543 between two steps; one host read.  The training state, a captured step included, is left as it was."""
        means, _logs, panel = validation.validate(system, val_bank, val_loss, epoch, hp, frames=a.val_frames,
                                                  want_panel=a.log_dir is not None)
        last_val[0] = means["val/psnr"]
        print(f"step {step:6d}  epoch {epoch}  " + "  ".join(f"{k} {v:.4f}" for k, v in means.items() if k in ("val/loss", "val/psnr")), flush=True)
        if a.log_dir and rank == 0:
            with open(os.path.join(a.log_dir, "val.jsonl"), "a") as f:
                f.write(json.dumps(dict(means, step=step, epoch=epoch)) + "\n")
            if panel is not None:
                save_panel(os.path.join(a.log_dir, f"val_panel_{step}.png"), *panel)

    def save_epoch(ep, steps_done, final=False):
        """train.py:554-564: the epoch's checkpoint and last.ckpt; the best val/psnr so far is recorded beside them."""
        stream = dict(seed=a.seed, step=steps_done, epoch=epoch, first=first, epoch_first=epoch_first, batch=a.batch,
                      stage=bool(system.train_geometry_stage), total_steps=a.steps, optimizer=a.optimizer)
        checkpoint.save_training_state(os.path.join(a.ckpt_dir, "last.ckpt"), system, opt, ep, steps_done, stream=stream,
                                       schedule=None if sched is None else sched.state_dict())
        if not final:
            import shutil
            shutil.copyfile(os.path.join(a.ckpt_dir, "last.ckpt"), os.path.join(a.ckpt_dir, f"epoch={ep}.ckpt"))
            if last_val[0] is not None and last_val[0] == last_val[0] and (best["best_score"] is None or last_val[0] > best["best_score"]):
                best.update(best_epoch=ep, best_score=last_val[0])
        with open(os.path.join(a.ckpt_dir, "best.json"), "w") as f:
            json.dump(best, f)

    # the epoch is the stream's: every ray of the bank once.  The stage's bank is a subset, so its epochs are shorter; where the
    # selection changes the stream starts again at position 0 of the new bank (`first`, `epoch_first`)
    epoch, first, epoch_first, start = 0, 0, 0, 0
    resumed = None
    if a.resume:
        # (the generators are put back below, behind the capture of the graph route: its rehearsal steps draw)
        try:
            resumed = checkpoint.load_training_state(a.resume, system, opt, trusted=a.trusted, restore_rng=False)
        except ValueError as e:
            raise SystemExit(f"--resume: {e}")
        st = resumed["stream"]
        if (resumed.get("schedule") is None) != (sched is None):
            raise SystemExit("--resume: the checkpoint was written " + ("without" if sched is not None else "with") + " --lr_scheduler; "
                             "continue it with the schedule it was written with")
        if sched is not None:
            try:
                sched.load_state_dict(resumed["schedule"])
            except ValueError as e:
                raise SystemExit(f"--resume: {e}")
        if (st["seed"], st["batch"], st["total_steps"]) != (a.seed, a.batch, a.steps):
            raise SystemExit(f"--resume: the checkpoint was written with --seed {st['seed']} --batch {st['batch']} --steps {st['total_steps']}; "
                             "continue it with the same (the stream and the learning-rate schedule depend on them)")
        epoch, first, epoch_first, start = st["epoch"], st["first"], st["epoch_first"], st["step"]
        if a.ckpt_dir and os.path.exists(os.path.join(a.ckpt_dir, "best.json")):
            with open(os.path.join(a.ckpt_dir, "best.json")) as f:
                best.update(json.load(f))
        print(f"resumed {a.resume}: step {start}, epoch {epoch}, lr {resumed['lr']:.3e}", flush=True)
    bank, loss_fn, gt_valid = setup(epoch)
    lr_by_epoch = {}
    if sched is not None:
        lr_by_epoch[epoch] = sched.apply(opt, epoch)
        print(f"epoch {epoch}  lr {lr_by_epoch[epoch]:.6e}", flush=True)
    graphed = training.GraphedTrainStep(system, opt, a.batch, loss_fn, epoch=epoch, gt_valid=gt_valid) if a.route == "graph" else None
    if resumed is not None:
        if graphed is not None:
            graphed.capture()
        checkpoint.restore_rng(a.resume, dev, trusted=a.trusted)
    if graphed is not None:
        out = (graphed.rays, graphed.target, graphed.gt)
    else:
        out = (torch.empty(a.batch, 8, device=dev), torch.empty(a.batch, 3, device=dev), torch.empty(a.batch, device=dev))
    t0 = time.time()
    loss = None
    done = start
    for it in range(start, a.steps):
        e = epoch_first + bank.epoch_of(it - first, a.batch, world)
        if a.num_epochs is not None and e >= a.num_epochs:
            break
        if e != epoch:
            if a.ckpt_dir and rank == 0:
                save_epoch(epoch, it)
            epoch, n_before = e, bank.n_rays
            bank, loss_fn, gt_valid = setup(epoch)
            if bank.n_rays != n_before:
                first, epoch_first = it, epoch
            if graphed is not None and graphed.gt_valid != gt_valid:
                graphed = training.GraphedTrainStep(system, opt, a.batch, loss_fn, epoch=epoch, gt_valid=gt_valid)
                out = (graphed.rays, graphed.target, graphed.gt)
            elif graphed is not None:
                graphed.set_epoch(epoch, loss_fn)
            if sched is not None:
                lr_by_epoch[epoch] = sched.apply(opt, epoch)
                print(f"epoch {epoch}  lr {lr_by_epoch[epoch]:.6e}", flush=True)
        rays, rgbs, mask = bank.draw(it - first, a.batch, a.seed, rank, world, out=out)
        if graphed is not None:
            loss = graphed(rays, rgbs, mask)          # the step's own buffers: its copy_ of a tensor onto itself is a no-op
        else:
            loss = training.train_step(system, opt, rays, rgbs, mask, loss_fn, epoch=epoch, gt_valid=gt_valid if a.route == "static" else None)
        done = it + 1
        if sched is None:
            opt.param_groups[0]["lr"] *= gamma
        if val_bank is not None:
            # val_check_interval (train.py:585): every int(batches per epoch * fraction) batches of the epoch
            per_epoch = max(1, bank.n_rays // (a.batch * world))
            every = max(1, int(per_epoch * a.val_every))
            if ((it - first) % per_epoch + 1) % every == 0:
                validate_now(it + 1)
        if it % 1000 == 0 or it == a.steps - 1:
            print(f"step {it:6d}  epoch {epoch}  loss {loss.item():.4f}  [{time.time() - t0:.0f} s]", flush=True)
    if a.ckpt_dir and rank == 0:
        save_epoch(epoch, done if a.num_epochs is not None else a.steps, final=True)
    arrs = {}
    for mname, mod in (("coarse", system.nerf_coarse), ("fine", system.nerf_fine)):
        for k, v in mod.state_dict().items():
            arrs[f"{mname}__{k}"] = v.detach().cpu().numpy().copy()
    arrs["meta"] = np.array(json.dumps(dict(steps=a.steps, batch=a.batch, lr=a.lr, root_dir=os.path.abspath(a.root_dir), img_wh=list(a.img_wh),
                                            frames=full.n_frames, route=a.route, loss=a.loss, seed=a.seed, epochs=epoch + 1,
                                            final_loss=None if loss is None else float(loss.item()),
                                            trained_with="mirror_nerf_amd (scripts/train_blender.py), precision " + a.precision,
                                            **({} if a.optimizer == "adam" else {"optimizer": a.optimizer}),
                                            **({} if a.num_epochs is None else {"steps_run": done}),
                                            **({} if sched is None else {"lr_scheduler": sched.state_dict()["options"],
                                                                         "lr_by_epoch": {str(k): v for k, v in lr_by_epoch.items()}}))))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **arrs)
    print("wrote", a.out, f"{os.path.getsize(a.out) / 1e6:.1f} MB; ms/step {(time.time() - t0) / max(1, a.steps) * 1e3:.2f}")


if __name__ == "__main__":
    main()
