"""Checkpoint interchange with the reference (utils/__init__.py:109-136; train.py:56,66;
eval.py:996-1001): a Lightning `.ckpt` (or a plain dict) whose `state_dict` keys are
`nerf_coarse.<param>` / `nerf_fine.<param>` loads into our MirrorNeRF modules unchanged, and
`save_ckpt` writes the same layout back."""
import os
import pickle

import torch


def _load_file(path, trusted=False):
    """torch.load of a checkpoint file.  Tensors-only first (`weights_only=True`, the default of this torch).  Lightning
    1.5 checkpoints of the reference also pickle `hyper_parameters` (an argparse.Namespace / AttributeDict), callbacks
    and optimizer states: those load with the known plain containers allow-listed; anything else needs `trusted=True`
    (full unpickling executes code from the file -- only for checkpoints you wrote yourself)."""
    try:
        return torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError as e:
        first = e
    import argparse
    import collections
    allow = [argparse.Namespace, collections.OrderedDict, collections.defaultdict, dict]
    try:
        with torch.serialization.safe_globals(allow):
            return torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError as e:
        if trusted:
            return torch.load(path, map_location="cpu", weights_only=False)
        raise RuntimeError(
            f"{path}: the checkpoint pickles objects outside the tensors-only allow-list ({e}); if you trust the file, "
            "pass trusted=True (load_ckpt / extract_model_state_dict) to unpickle it fully") from first


def extract_model_state_dict(ckpt, model_name="model", prefixes_to_ignore=(), trusted=False):
    """ckpt: path (str / bytes / os.PathLike) or an already loaded dict.  Returns {param name: tensor} of `model_name`."""
    checkpoint = _load_file(os.fspath(ckpt), trusted) if isinstance(ckpt, (str, bytes, os.PathLike)) else ckpt
    if "state_dict" in checkpoint:   # pytorch-lightning checkpoint
        checkpoint = checkpoint["state_dict"]
    out = {}
    for k, v in checkpoint.items():
        if not k.startswith(model_name):
            continue
        k = k[len(model_name) + 1:]
        if any(k.startswith(p) for p in prefixes_to_ignore):
            continue
        out[k] = v
    return out


def load_ckpt(model, ckpt, model_name="model", prefixes_to_ignore=(), trusted=False):
    if not ckpt:
        return
    sd = model.state_dict()
    got = extract_model_state_dict(ckpt, model_name, prefixes_to_ignore, trusted)
    assert len(got) > 0, f"the checkpoint holds no parameter named '{model_name}.*'"     # the reference asserts here too
    sd.update(got)
    model.load_state_dict(sd, strict=False)


def save_ckpt(path, system, epoch=0, global_step=0):
    """Writes {"state_dict": {"nerf_coarse.*", "nerf_fine.*"}, "epoch", "global_step"} like Lightning's
    ModelCheckpoint does for train.NeRFSystem."""
    sd = {}
    for name in ("nerf_coarse", "nerf_fine"):
        m = getattr(system, name, None)
        if m is not None:
            for k, v in m.state_dict().items():
                sd[f"{name}.{k}"] = v.detach().cpu()
    torch.save({"state_dict": sd, "epoch": epoch, "global_step": global_step}, path)


_FIELDS = ("nerf_coarse", "nerf_fine")


def _to_cpu(o):
    """An optimizer state dict with every tensor as a CPU copy; dicts, lists and tuples keep their type."""
    if isinstance(o, torch.Tensor):
        return o.detach().cpu().clone()
    if isinstance(o, dict):
        return {k: _to_cpu(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return type(o)(_to_cpu(v) for v in o)
    return o


def save_training_state(path, system, optimizer, epoch, global_step, stream=None, schedule=None):
    """A checkpoint a run can be resumed from (train.py:554-564, 574).  The file is Lightning-shaped: the `state_dict`, `epoch`
    and `global_step` of save_ckpt, so load_ckpt, scripts/eval_scene.py --ckpt_path and the reference's load_ckpt read it as any
    checkpoint, plus
      optimizer_states  [optimizer.state_dict()] (training.FlatAdam's, FlatSGD's, FlatRAdam's or a torch optimizer's), Lightning's key;
      mnrf_training     lr (the first group's current value), grad_scale {field: the gradient-scale reductions of the split
                        backward}, stream (the caller's position in the bank's shuffled stream: seed, step, epoch, stage ...,
                        plain numbers), rng {cpu, cuda: the generators' states}, schedule (schedules.LRSchedule.state_dict(): the
                        options and the epoch of a learning-rate schedule, or None), optimizer (the class name).
    Only tensors and plain containers are written: load_training_state reads it with the tensors-only unpickler."""
    sd = {}
    for name in _FIELDS:
        m = getattr(system, name, None)
        if m is not None:
            for k, v in m.state_dict().items():
                sd[f"{name}.{k}"] = v.detach().cpu().clone()
    opt = optimizer.state_dict()
    dev = next(system.parameters()).device
    rng = {"cpu": torch.get_rng_state()}
    if dev.type == "cuda":
        rng["cuda"] = torch.cuda.get_rng_state(dev)
    extra = {"lr": float(optimizer.param_groups[0]["lr"]),
             "grad_scale": {name: int(getattr(system, name).__dict__.get("_mnrf_seed_reduction", 0))
                            for name in _FIELDS if getattr(system, name, None) is not None},
             "stream": {k: (v if isinstance(v, (bool, int, float, str)) or v is None else int(v)) for k, v in dict(stream or {}).items()},
             "rng": rng, "schedule": schedule, "optimizer": type(optimizer).__name__}
    torch.save({"state_dict": sd, "epoch": int(epoch), "global_step": int(global_step), "optimizer_states": [_to_cpu(opt)],
                "lr_schedulers": [], "mnrf_training": extra}, path)


def _set_rng(rng, device):
    torch.set_rng_state(rng["cpu"])
    if device.type == "cuda" and "cuda" in rng:
        torch.cuda.set_rng_state(rng["cuda"], device)


def restore_rng(path, device, trusted=False):
    """The generators as save_training_state found them, for a caller that draws between loading a state and continuing
    (load_training_state(..., restore_rng=False) first: capturing a training.GraphedTrainStep rehearses steps, which draw)."""
    _set_rng(_load_file(os.fspath(path), trusted)["mnrf_training"]["rng"], torch.device(device))


def load_training_state(path, system, optimizer=None, trusted=False, restore_rng=True):
    """Put a save_training_state file back: the fields' parameters (in place: training.FlatAdam's views stay views), the
    optimizer state and learning rate, the gradient-scale state and -- restore_rng -- the generators.  Load BEFORE a
    GraphedTrainStep is built on the optimizer.  Unpickling follows _load_file (tensors and plain containers unless `trusted`).
    A state written by another optimizer class than `optimizer`'s is refused (ValueError; files from before the class was recorded
    are taken as they are).  Returns {"epoch", "global_step", "lr", "stream"}, and "schedule" where the file carries one."""
    ckpt = _load_file(os.fspath(path), trusted)
    if "mnrf_training" not in ckpt:
        raise RuntimeError(f"{path}: a checkpoint without training state (written by save_ckpt or by the reference): it can "
                           "initialise the weights (load_ckpt) but a run cannot be resumed from it")
    extra = ckpt["mnrf_training"]
    written_by = extra.get("optimizer")
    if optimizer is not None and written_by is not None and written_by != type(optimizer).__name__:      # (before anything is changed)
        raise ValueError(f"{path}: the optimizer state was written by {written_by}, not by {type(optimizer).__name__}: a run "
                         "continues with the optimizer it was started with")
    with torch.no_grad():
        for name in _FIELDS:
            m = getattr(system, name, None)
            if m is None:
                continue
            got = extract_model_state_dict(ckpt, name)
            own = m.state_dict()
            if sorted(got) != sorted(own):
                raise RuntimeError(f"{path}: the parameters of {name} differ from the model's: {sorted(set(got) ^ set(own))}")
            for k, v in own.items():
                v.copy_(got[k])
            m.__dict__.pop("_mnrf_seed_reduction", None)
            if int(extra["grad_scale"].get(name, 0)):
                m.__dict__["_mnrf_seed_reduction"] = int(extra["grad_scale"][name])
            from .weights import invalidate_packed
            invalidate_packed(m)
    if optimizer is not None:
        optimizer.load_state_dict(ckpt["optimizer_states"][0])      # (training.FlatAdam: its device-resident step count included)
        for g in optimizer.param_groups:
            g["lr"] = float(extra["lr"])
    if restore_rng:
        _set_rng(extra["rng"], next(system.parameters()).device)
    out = {"epoch": int(ckpt["epoch"]), "global_step": int(ckpt["global_step"]), "lr": float(extra["lr"]),
           "stream": dict(extra["stream"])}
    if extra.get("schedule") is not None:
        out["schedule"] = extra["schedule"]
    return out
