"""The reference's learning-rate schedules (utils/__init__.py:77-101 get_scheduler, utils/warmup_scheduler.py, opt.py:118-153) as
closed forms of the epoch: Lightning steps them once per epoch (train.py:364-366 returns the scheduler with the default
interval), so the rate is a function of the epoch alone and stays constant within one.

    sched = lr_schedule(hparams)          # hparams: lr, lr_scheduler, decay_step, decay_gamma, num_epochs, poly_exp,
    sched.apply(optimizer, epoch)         #          warmup_epochs, warmup_multiplier, optimizer -- the reference's options
    sched.lr_at(epoch)

  steplr  torch's MultiStepLR(milestones=decay_step, gamma=decay_gamma): lr * gamma ** (milestones <= epoch)
  cosine  torch's CosineAnnealingLR(T_max=num_epochs, eta_min=1e-8): eta_min + (lr - eta_min) (1 + cos(pi epoch / T_max)) / 2
  poly    lr * (1 - epoch / num_epochs) ** poly_exp.  The reference's own `poly` cannot run: utils/__init__.py:86 builds a
          LambdaLR that the file never imports, a NameError; this is the schedule its lambda describes.  It ends with
          num_epochs (the base of the power is negative afterwards): lr_at refuses a later epoch.

Warm-up (warmup_epochs W > 0, optimizer sgd or adam only, as utils/__init__.py:93): the linear ramp
lr ((warmup_multiplier - 1) epoch / W + 1) for epoch <= W, the value of epoch W once more at W + 1, then the schedule above from
lr * warmup_multiplier at ITS epoch `epoch - W - 1`.  That is what the reference's GradualWarmupScheduler does in front of steplr
and poly (tests/golden/schedules/lr_sequences.json).  In front of cosine it is refused: the class calls `get_lr()` of the
after-scheduler, which for CosineAnnealingLR is torch's recursive form and reads the optimizer's current rate, not its own base;
what comes out depends on the torch version and is not a cosine from lr * multiplier (5.087e-4 at epoch 4 from a base of 5e-4,
with W = 3 over 12 epochs under torch 2.10)."""
import math

SCHEDULERS = ("steplr", "cosine", "poly")
COSINE_ETA_MIN = 1e-8
_DEFAULTS = dict(lr=5e-4, lr_scheduler="steplr", decay_step=(20,), decay_gamma=0.1, num_epochs=16, poly_exp=0.9, warmup_epochs=0,
                 warmup_multiplier=1.0, optimizer="adam")


class LRSchedule:
    def __init__(self, options):
        self.options = dict(options)
        self.epoch = None                  # the epoch of the last apply(): the position a checkpoint carries

    def _after(self, base, e):
        o = self.options
        if o["lr_scheduler"] == "steplr":
            return base * o["decay_gamma"] ** sum(1 for m in o["decay_step"] if m <= e)
        if o["lr_scheduler"] == "cosine":
            return COSINE_ETA_MIN + (base - COSINE_ETA_MIN) * (1.0 + math.cos(math.pi * e / o["num_epochs"])) / 2.0
        if e > o["num_epochs"]:
            raise ValueError(f"lr_schedule: poly ends with num_epochs = {o['num_epochs']}; epoch {e} is past it")
        return base * (1.0 - e / o["num_epochs"]) ** o["poly_exp"]

    def lr_at(self, epoch):
        """The learning rate of `epoch` (0-based: the rate the steps of that epoch run with)."""
        e, o = int(epoch), self.options
        if e < 0:
            raise ValueError("lr_schedule: epoch >= 0")
        W, mult = o["warmup_epochs"], o["warmup_multiplier"]
        if W <= 0:
            return self._after(o["lr"], e)
        if e <= W + 1:
            return o["lr"] * ((mult - 1.0) * min(e, W) / W + 1.0)
        return self._after(o["lr"] * mult, e - W - 1)

    def apply(self, optimizer, epoch):
        """Write the epoch's rate into every param group (FlatAdam and its siblings read theirs at every step)."""
        lr = self.lr_at(epoch)
        for g in optimizer.param_groups:
            g["lr"] = lr
        self.epoch = int(epoch)
        return lr

    def state_dict(self):
        """Plain numbers, strings and lists: the options and the position."""
        return {"options": {k: (list(v) if isinstance(v, (list, tuple)) else v) for k, v in self.options.items()}, "epoch": self.epoch}

    def load_state_dict(self, sd):
        """Continue at the saved position; a state written for other options is refused (the rates would not be the run's)."""
        mine, saved = self.state_dict()["options"], dict(sd["options"])
        if saved != mine:
            diff = sorted(k for k in set(mine) | set(saved) if mine.get(k) != saved.get(k))
            raise ValueError("lr_schedule: the saved schedule differs from this one in " +
                             ", ".join(f"{k} ({saved.get(k)!r} saved, {mine.get(k)!r} here)" for k in diff))
        self.epoch = sd["epoch"]


def lr_schedule(hparams):
    """The schedule the reference's get_scheduler builds from `hparams` (an argparse namespace or anything with the options as
    attributes; a missing option takes opt.py's default), as an LRSchedule."""
    o = {k: getattr(hparams, k, d) for k, d in _DEFAULTS.items()}
    o.update(lr=float(o["lr"]), decay_step=[int(m) for m in o["decay_step"]], decay_gamma=float(o["decay_gamma"]),
             num_epochs=int(o["num_epochs"]), poly_exp=float(o["poly_exp"]), warmup_epochs=int(o["warmup_epochs"]),
             warmup_multiplier=float(o["warmup_multiplier"]))
    if o["lr_scheduler"] not in SCHEDULERS:
        raise ValueError(f"lr_schedule: scheduler not recognized: {o['lr_scheduler']!r} (one of {', '.join(SCHEDULERS)})")
    if o["num_epochs"] < 1 and o["lr_scheduler"] != "steplr":
        raise ValueError("lr_schedule: num_epochs >= 1")
    if o["warmup_epochs"] > 0 and o["optimizer"] in ("radam", "ranger"):
        o["warmup_epochs"] = 0             # utils/__init__.py:93: no warm-up in front of the rectified optimizers
    if o["warmup_epochs"] > 0:
        if o["warmup_multiplier"] < 1.0:
            raise ValueError("lr_schedule: warmup_multiplier should be greater than or equal to 1")      # warmup_scheduler.py:17-18
        if o["lr_scheduler"] == "cosine":
            raise ValueError("lr_schedule: warm-up in front of cosine is not supported: the reference's warm-up class steps "
                             "CosineAnnealingLR through torch's recursive get_lr(), which does not start from lr * "
                             "warmup_multiplier and whose sequence depends on the torch version; use steplr or poly, or no warm-up")
    else:
        o["warmup_epochs"], o["warmup_multiplier"] = 0, 1.0      # (without warm-up the multiplier is never read)
    del o["optimizer"]
    return LRSchedule(o)
