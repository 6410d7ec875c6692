#!/usr/bin/env python3
"""Golden learning-rate sequences (tests/golden/schedules/lr_sequences.json): 40 epochs of torch's own schedulers, composed the
way the reference's get_scheduler composes them (utils/__init__.py:77-101: MultiStepLR(decay_step, decay_gamma) |
CosineAnnealingLR(T_max=num_epochs, eta_min=1e-8) | LambdaLR of (1 - epoch / num_epochs) ** poly_exp, behind the REFERENCE's
GradualWarmupScheduler where warmup_epochs > 0), stepped once per epoch as Lightning steps an epoch-interval scheduler: entry e is
the rate the steps of epoch e run with.  utils/warmup_scheduler.py is imported by path (utils/__init__.py itself imports
torch_optimizer, which this container lacks); LambdaLR is imported here because the reference forgets to (its `poly` raises
NameError).

  steplr_run_sh     --decay_step 2 4 8 --decay_gamma 0.5 (run.sh:259-280)        steplr_default   opt.py's: [20], 0.1
  cosine            T_max = 30 (so the 40 epochs pass the minimum)                 poly             num_epochs 40, poly_exp 0.9
  steplr_driver     --decay_step 1 2 --num_epochs 3: the three-epoch run of the driver's GPU test (tests/test_hip_optim_steps.py)
  steplr / poly with warm-up: W = 3, multiplier 1 and 2
  cosine_warmup_w3_12: the combination the package refuses, recorded for the doc string's figure (W = 3, 12 epochs)

Build-container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_schedules.py
"""
import importlib.util
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import _ref_import as R  # noqa: E402
import torch  # noqa: E402
from torch.optim.lr_scheduler import CosineAnnealingLR, LambdaLR, MultiStepLR  # noqa: E402

EPOCHS = 40
BASE = 5e-4
CASES = {
    "steplr_run_sh": dict(lr_scheduler="steplr", decay_step=[2, 4, 8], decay_gamma=0.5, num_epochs=30),
    "steplr_driver": dict(lr_scheduler="steplr", decay_step=[1, 2], decay_gamma=0.1, num_epochs=3),
    "steplr_default": dict(lr_scheduler="steplr", decay_step=[20], decay_gamma=0.1, num_epochs=16),
    "cosine": dict(lr_scheduler="cosine", num_epochs=30),
    "poly": dict(lr_scheduler="poly", num_epochs=40, poly_exp=0.9),
    "steplr_warmup_m1": dict(lr_scheduler="steplr", decay_step=[2, 4, 8], decay_gamma=0.5, num_epochs=30, warmup_epochs=3, warmup_multiplier=1.0),
    "steplr_warmup_m2": dict(lr_scheduler="steplr", decay_step=[2, 4, 8], decay_gamma=0.5, num_epochs=30, warmup_epochs=3, warmup_multiplier=2.0),
    "poly_warmup_m1": dict(lr_scheduler="poly", num_epochs=40, poly_exp=0.9, warmup_epochs=3, warmup_multiplier=1.0),
    "poly_warmup_m2": dict(lr_scheduler="poly", num_epochs=40, poly_exp=0.9, warmup_epochs=3, warmup_multiplier=2.0),
}
REFUSED = {"cosine_warmup_w3_12": (dict(lr_scheduler="cosine", num_epochs=12, warmup_epochs=3, warmup_multiplier=1.0), 12)}


def warmup_class():
    if not R.available():
        raise RuntimeError("reference tree not present at " + R.REF_ROOT)
    spec = importlib.util.spec_from_file_location("ref_warmup_scheduler", os.path.join(R.REF_ROOT, "utils", "warmup_scheduler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.GradualWarmupScheduler


def sequence(o, epochs):
    p = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=BASE)
    after = {"steplr": lambda: MultiStepLR(opt, milestones=o.get("decay_step"), gamma=o.get("decay_gamma")),
             "cosine": lambda: CosineAnnealingLR(opt, T_max=o["num_epochs"], eta_min=1e-8),
             "poly": lambda: LambdaLR(opt, lambda epoch: (1 - epoch / o["num_epochs"]) ** o["poly_exp"])}[o["lr_scheduler"]]()
    sched = after
    if o.get("warmup_epochs", 0) > 0:
        sched = warmup_class()(opt, multiplier=o["warmup_multiplier"], total_epoch=o["warmup_epochs"], after_scheduler=after)
    out = []
    for _ in range(epochs):
        out.append(float(opt.param_groups[0]["lr"]))
        p.grad = torch.zeros_like(p)
        opt.step()
        sched.step()
    return out


def main():
    d = os.path.join(os.environ.get("MNRF_GOLDEN_OUT", HERE), "schedules")
    os.makedirs(d, exist_ok=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (the warm-up class passes an epoch to step(): deprecated, still honoured)
        doc = {"meta": {"torch": torch.__version__, "epochs": EPOCHS, "lr": BASE, "optimizer": "adam",
                        "source": "torch.optim.lr_scheduler + the reference's utils/warmup_scheduler.py, stepped once per epoch"},
               "cases": {k: {"options": o, "lr": sequence(o, EPOCHS)} for k, o in CASES.items()},
               "refused": {k: {"options": o, "lr": sequence(o, n)} for k, (o, n) in REFUSED.items()}}
    path = os.path.join(d, "lr_sequences.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    for k, c in doc["cases"].items():
        print(k, " ".join(f"{v:.4g}" for v in c["lr"][:12]), "...")
    print("refused:", doc["refused"])
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
