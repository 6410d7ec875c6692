#!/usr/bin/env python3
"""Golden vectors of the validation loop (tests/golden/validation/): the REFERENCE's

(a) utils/visualization.py `visualize_val_image(img_wh, batch, results, add_text=False)` on a 6x8 frame whose `results` carry
    every key it reads (tests/val_panel_ref.seeded_case): val_panel_6x8.npz.  The module is imported by path with two
    stand-ins for libraries this container lacks: `cv2.applyColorMap(x, cmap)` is a look-up in mirror_nerf_amd.frames.jet_table()
    and torchvision's `ToTensor()` is its published definition for an 8-bit image (HWC -> CHW, float32, / 255).  Everything
    else -- the order and presence rules, the transposes, visualize_depth's normalisation, visualize_rgb_map_global -- is the
    reference's code.  THE COLOUR TABLE IS THE PROJECT'S RESTATEMENT AND IS NOT PINNED (meta.table).
(b) train.py `NeRFSystem.validation_step(batch, batch_nb=1)` (no panel drawn) on an 8x6 frame of the analytic scene (the
    STRADDLE weights of the G6/G7 fixtures), perturb = noise_std = 0, once in the geometry stage (ground truth blackened inside
    the mirror mask, nothing traced) and once outside it with reflections traced: val_step_stage.npz, val_step_traced.npz hold
    the `log` dict.

Build-container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_validation.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

import _ref_import as R  # noqa: E402

R.install()
import torch  # noqa: E402

import weights as W  # noqa: E402
from make_golden import ref_models  # noqa: E402
from oracle import mirror_nerf_oracle as O  # noqa: E402
from tests import val_panel_ref as VR  # noqa: E402

torch.set_num_threads(8)
SUB = "validation"


def _out(name):
    d = os.path.join(os.environ.get("MNRF_GOLDEN_OUT", HERE), SUB)
    os.makedirs(d, exist_ok=True)
    return os.path.join(d, name + ".npz")


def ref_visualization():
    """utils/visualization.py by path, with the two stand-ins of the module docstring installed first."""
    from mirror_nerf_amd.frames import jet_table     # (numpy only: nothing touches a GPU)
    table = jet_table()
    sys.modules["cv2"].applyColorMap = lambda x, cmap: table[np.asarray(x)]

    class ToTensor:
        def __call__(self, img):
            a = np.asarray(img)
            assert a.dtype == np.uint8 and a.ndim == 3
            return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(torch.float32).div(255)

    sys.modules["torchvision.transforms"].ToTensor = ToTensor
    spec = importlib.util.spec_from_file_location("ref_visualization", os.path.join(R.REF_ROOT, "utils", "visualization.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, table


def panel_case(name="val_panel_6x8", H=6, W_=8, seed=11):
    V, table = ref_visualization()
    batch, results = VR.seeded_case(H, W_, seed, "all")
    tb = {k: torch.from_numpy(v.copy()) for k, v in batch.items()}
    tr = {k: torch.from_numpy(v.copy()) for k, v in results.items()}
    stack = V.visualize_val_image((W_, H), tb, tr, add_text=False).numpy()
    mine, names = VR.val_panel((W_, H), batch, results, table)
    assert stack.shape == mine.shape == (len(names), 3, H, W_), (stack.shape, mine.shape)
    assert np.array_equal(stack, mine, equal_nan=True), "tests/val_panel_ref.py does not reproduce the reference's panel"
    for k in results:        # the reference leaves its inputs alone
        assert np.array_equal(tr[k].numpy(), results[k], equal_nan=True), k
    arrs = {"batch__" + k: v for k, v in batch.items()}
    arrs.update({"in__" + k: v for k, v in results.items()})
    arrs["out__stack"] = stack
    arrs["meta"] = np.array(json.dumps(dict(
        H=H, W=W_, seed=seed, variant="all", names=names,
        table="mirror_nerf_amd.frames.jet_table(): the project's restatement of COLORMAP_JET in cv2's BGR order, NOT pinned "
              "against cv2 (absent from the build container); ToTensor is its published definition")))
    np.savez_compressed(_out(name), **arrs)
    print(f"  wrote {SUB}/{name}.npz  {os.path.getsize(_out(name)) / 1024:.0f} KiB  ({len(names)} tiles)")


HP = dict(predict_normal=True, predict_mirror_mask=True, trace_secondary_rays=True, N_samples=64, N_importance=64, perturb=0,
          noise_std=0, chunk=32768)


def step_case(name, stage, epoch, H=6, W_=8, seed=21):
    import train as ref_train

    hp = R.get_hparams(train_geometry_stage=stage, **HP)
    torch.manual_seed(0)
    system = ref_train.NeRFSystem(hp)
    _, sds = ref_models(0, 2, W.STRADDLE)
    system.nerf_coarse.load_state_dict({k: torch.from_numpy(v) for k, v in sds[0].items()})
    system.nerf_fine.load_state_dict({k: torch.from_numpy(v) for k, v in sds[1].items()})
    system.current_epoch = epoch
    system.train_dataset = types.SimpleNamespace(white_back=False, train_geometry_stage=stage)
    system.val_dataset = types.SimpleNamespace(white_back=False, train_geometry_stage=stage)
    n = H * W_
    rays = O.synthetic_rays(H, W_)
    rs = np.random.RandomState(seed)
    rgbs = rs.uniform(size=(n, 3)).astype(np.float32)
    gt = np.zeros((H, W_), np.float32)
    gt[1:5, 2:6] = 1.0                                   # a valid mask with a mirror block
    gt = gt.reshape(n)
    batch = {"rays": torch.from_numpy(rays.copy())[None], "rgbs": torch.from_numpy(rgbs.copy())[None],
             "mirror_mask": torch.from_numpy(gt.copy())[None]}
    with torch.no_grad():                                # Lightning's validation loop
        log = system.validation_step(batch, 1)
    assert system.train_geometry_stage == stage
    blackened = bool((batch["rgbs"][0].numpy() != rgbs).any())
    assert blackened == stage
    outs = {k: np.float32(float(v)) for k, v in log.items()}
    print(f"  {name}: " + "  ".join(f"{k} {float(v):.6f}" for k, v in outs.items()))
    arrs = {"in__rays": rays, "in__rgbs": rgbs, "in__gt_mask": gt}
    arrs.update({"out__" + k: v for k, v in outs.items()})
    hp_o = dict(HP, train_geometry_stage=stage, only_one_field=False, max_recursive_level=hp.max_recursive_level,
                only_trace_rays_in_mirrors=hp.only_trace_rays_in_mirrors, for_vis=hp.for_vis, use_disp=False,
                train_geometry_stage_end_epoch=hp.train_geometry_stage_end_epoch)
    arrs["meta"] = np.array(json.dumps(dict(seed=0, n_models=2, tweaks=W.STRADDLE, checksum=[W.checksum(s) for s in sds], hp=hp_o,
                                            epoch=epoch, H=H, W=W_, batch_nb=1, blackened=blackened, keys=list(outs))))
    np.savez_compressed(_out(name), **arrs)
    print(f"  wrote {SUB}/{name}.npz  {os.path.getsize(_out(name)) / 1024:.0f} KiB")


def main():
    panel_case()
    step_case("val_step_stage", True, 0)
    step_case("val_step_traced", False, 5)


if __name__ == "__main__":
    main()
