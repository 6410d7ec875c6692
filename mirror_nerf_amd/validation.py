"""The validation half of the reference's training loop (train.py:460-543): `validation_step` renders one validation frame
with the eval semantics of the recursion (reflections kept apart: rgb_*_reflect, depth_*_reflect, secondary_rays_o,
reflect_direction), evaluates the reference's loss and PSNR on it and returns the `log` dict as device scalars; `validate`
runs it over the validation frames, takes validation_epoch_end's means and, for frame 0, builds the val/GT_pred_depth panel
on the device (frames.val_panel).

    loss = losses.get_loss(hparams)
    means, logs, panel = validate(system, val_bank, loss, epoch, hparams)       # between two training steps
    means["val/psnr"]                                                           # Python floats: the one host read

A validation leaves the training state as it found it: parameters and `.grad` (everything runs under no_grad), the modules'
`training` flags, the gradient-scale state, the precision the range guard selected, the guard words the training launches
wrote into the packed weight images, and the random generators (the reference validates with --perturb / --noise_std as it
trains, so a validation draws; the draws come from the generators' state, which is put back).  A captured GraphedTrainStep
therefore replays after a validation exactly as without one.  If the split arithmetic leaves its range on a validation frame,
that frame is rendered again on the exact fp32 kernels, as batched_inference does, and the models return to what they were:
the training route is never pinned from here."""
import torch

from . import frames as _frames
from . import metrics
from .mirror_nerf import MirrorNeRF, guard_words, precision_of
from . import mirror_nerf as _mn
from .weights import invalidate_packed

_GUARD_KEYS = ("_mnrf_precision", "_mnrf_transient", "_mnrf_range_trips", "_mnrf_guard_trips", "_mnrf_seed_reduction")


def _word(m):
    cache = m.__dict__.get("_mnrf_packed")
    return None if cache is None or cache.packed is None else cache.packed[-1:]


class _held:
    """Everything a validation could leave behind in the training state, saved on entry and put back on exit."""

    def __init__(self, system):
        self.system = system

    def __enter__(self):
        s = self.system
        self.training = [(m, m.training) for m in s.modules()]
        self.stage = s.train_geometry_stage
        self.fields = [m for m in dict.fromkeys(s.models.values()) if isinstance(m, MirrorNeRF)]
        self.flags = [{k: m.__dict__[k] for k in _GUARD_KEYS if k in m.__dict__} for m in self.fields]
        self.words = [None if _word(m) is None else _word(m).clone() for m in self.fields]
        self.cpu_rng = torch.get_rng_state()
        self.dev_rng = torch.cuda.get_rng_state(next(s.parameters()).device)
        return self

    def __exit__(self, *exc):
        s = self.system
        for m, t in self.training:
            m.training = t
        s.train_geometry_stage = self.stage
        for m, flags, word in zip(self.fields, self.flags, self.words):
            for k in _GUARD_KEYS:
                m.__dict__.pop(k, None)
            m.__dict__.update(flags)
            now = _word(m)
            if now is not None:      # (an image first packed during the validation had no training launch yet: a clean word)
                now.zero_() if word is None else now.copy_(word)
            invalidate_packed(m)     # the next step packs again, as it does behind every optimizer step
        torch.set_rng_state(self.cpu_rng)
        torch.cuda.set_rng_state(self.dev_rng, next(s.parameters()).device)
        return False


def _stage_of(system, epoch, hparams):
    """train.py:462-466: the stage flag, cleared from train_geometry_stage_end_epoch on."""
    return bool(system.train_geometry_stage) and not epoch >= getattr(hparams, "train_geometry_stage_end_epoch", 4)


def _extra_info(hparams, batch, epoch, stage):
    """train.py:491-506."""
    return {"is_eval": True, "mirror_mask": batch["mirror_mask"].reshape(-1),
            "only_one_field": getattr(hparams, "only_one_field", False),
            "only_one_field_fine_epoch": getattr(hparams, "only_one_field_fine_epoch", 2), "current_epoch": epoch,
            "train_geometry_stage": stage,
            "detach_density_outside_mirror_for_mask_loss": getattr(hparams, "detach_density_outside_mirror_for_mask_loss", False),
            "detach_density_for_mask_loss": getattr(hparams, "detach_density_for_mask_loss", False),
            "detach_density_for_normal_loss": getattr(hparams, "detach_density_for_normal_loss", False)}


def _render(system, rays, extra):
    """system(rays, extra) under the validation's own range guard: the words are cleared in front of the frame, read behind
    it, and a frame that tripped is rendered again with every field on the fp32 kernels (for this frame only)."""
    fields = [m for m in dict.fromkeys(system.models.values()) if isinstance(m, MirrorNeRF)]
    watch = _mn.GUARD and _mn.PRECISION == "split" and any(precision_of(m) == "split" for m in fields)
    if watch:
        for m in fields:
            if _word(m) is not None:
                _word(m).zero_()
        rng = torch.get_rng_state(), torch.cuda.get_rng_state(rays.device)
    results = system(rays, dict(extra, _guard=False))
    if watch and rays.shape[0] and any(guard_words(fields)):
        before = [m.__dict__.get("_mnrf_precision") for m in fields]
        try:
            torch.set_rng_state(rng[0])                      # the same frame again: the same draws
            torch.cuda.set_rng_state(rng[1], rays.device)
            for m in fields:
                m.__dict__["_mnrf_precision"] = "fp32"
            results = system(rays, dict(extra, _guard=False))
        finally:
            for m, p in zip(fields, before):
                m.__dict__.pop("_mnrf_precision", None)
                if p is not None:
                    m.__dict__["_mnrf_precision"] = p
    return results


def _step(system, batch, loss, epoch, hparams):
    stage = _stage_of(system, epoch, hparams)
    system.train_geometry_stage = stage
    rays = batch["rays"].reshape(-1, batch["rays"].shape[-1])
    gt_mask = batch["mirror_mask"].reshape(-1)
    rgbs = batch["rgbs"].reshape(-1, 3)
    if stage and not getattr(hparams, "woMaskRGBtoBlack", False):
        # train.py:480-486 on a copy, and without the host read of `(mask < 0).any()`: black inside a mask that is valid everywhere
        black = (gt_mask != 0) & ~(gt_mask < 0).any()
        rgbs = torch.where(black.view(-1, 1), torch.zeros((), dtype=rgbs.dtype, device=rgbs.device), rgbs)
    batch = dict(batch, rays=rays, rgbs=rgbs, mirror_mask=gt_mask)
    results = _render(system, rays, _extra_info(hparams, batch, epoch, stage))
    loss_sum, loss_dict = loss(results, batch, stage)
    log = {"val_loss": loss_sum}
    log.update(loss_dict)
    typ = "fine" if "rgb_fine" in results else "coarse"
    log["val_psnr"] = metrics.psnr(results[f"rgb_{typ}"], rgbs)
    log["val_psnr_coarse"] = metrics.psnr(results["rgb_coarse"], rgbs)
    return log, batch, results


def validation_step(system, batch, loss, epoch, hparams):
    """train.py:460-534 for one frame.  batch: what RayBank.frame(f) returns, on the device (never written: the geometry stage
    blackens a copy of the colours).  loss: losses.get_loss(hparams).  Returns the reference's `log` dict -- val_loss, the loss
    terms in use, val_psnr (fine, or coarse without a fine model), val_psnr_coarse -- as 0-d device tensors: no value is read
    here.  The training state is left untouched (module docstring)."""
    with torch.no_grad(), _held(system):
        return _step(system, batch, loss, epoch, hparams)[0]


def validate(system, bank, loss, epoch, hparams, frames=None, want_panel=True):
    """validation_step over frames `frames` of `bank` (default: all) and validation_epoch_end's means (train.py:536-543).
    Returns (means, logs, panel): means {"val/loss", "val/psnr", "val/psnr_coarse"} plus "val/<term>" for every loss term, as
    Python floats (the one host read of the validation); logs: the per-frame log dicts as floats; panel: (stack, names) of
    frames.val_panel for the first frame, the reference's batch_nb == 0, or None without want_panel."""
    todo = list(range(bank.n_frames)) if frames is None else [int(f) for f in frames]
    if not todo:
        raise ValueError("validate: no frame to validate")
    logs, panel = [], None
    with torch.no_grad(), _held(system):
        for i, f in enumerate(todo):
            log, batch, results = _step(system, bank.frame(f), loss, epoch, hparams)
            if i == 0 and want_panel:
                panel = _frames.val_panel((bank.W, bank.H), batch, results)
            logs.append(log)
        keys = list(logs[0])
        table = torch.stack([torch.stack([log[k].float().reshape(()) for k in keys]) for log in logs])
        host = torch.cat([table, table.mean(0, keepdim=True)]).tolist()          # the one host read
    logs = [dict(zip(keys, row)) for row in host[:-1]]
    mean = dict(zip(keys, host[-1]))
    means = {"val/loss": mean["val_loss"], "val/psnr": mean["val_psnr"], "val/psnr_coarse": mean["val_psnr_coarse"]}
    means.update({f"val/{k}": v for k, v in mean.items() if not k.startswith("val_")})
    return means, logs, panel

