"""`RayBank.from_arkit` on the GPU against the reference's RealDatasetARKit (fixture G25) on the scene of
tests/arkit_scene.py, written here as PNGs: colours and masks with tolerance zero, rays within 1e-6 (a float64 pose that differs
in its last bits may round to the neighbouring float32), near and far exact; the bank's bytes are read_arkit's.  For the path
splits, synthetic.generate_rays on read_arkit's poses meets the reference's rays (fixture G24) within 1e-6."""
import numpy as np
import pytest
import torch

from tests import arkit_scene as SC
from tests.golden.fixtures import Fixture

pytestmark = pytest.mark.gpu
ARGS = (SC.IMG_WH, SC.NEAR, SC.FAR, SC.SCALE_FACTOR)


@pytest.fixture(scope="module")
def g25():
    return Fixture("g25_arkit_train")


@pytest.fixture(scope="module")
def scene(tmp_path_factory, g25):
    root = str(tmp_path_factory.mktemp("arkit") / "lounge")
    SC.write_scene(root, g25.inputs["poses"], g25.inputs["key_poses"])
    return root


@pytest.fixture(scope="module")
def bank(scene):
    from mirror_nerf_amd.data import RayBank
    return RayBank.from_arkit(scene, "train", *ARGS, val_idx=SC.VAL_IDX, workers=3)


def test_bank_bytes_are_read_arkit_s(scene, bank):
    from mirror_nerf_amd.data import read_arkit
    d = read_arkit(scene, "train", *ARGS, val_idx=SC.VAL_IDX)
    assert (bank.H, bank.W, bank.channels, bank.n_frames) == (6, 8, 4, 6)
    assert np.array_equal(bank.images.cpu().numpy(), d["images"])
    assert np.array_equal(bank.masks.cpu().numpy(), d["masks"])
    assert np.array_equal(bank.poses.cpu().numpy(), d["poses"])
    assert (bank.focal, bank.near, bank.far) == (d["focal"], d["near"], d["far"]) and np.array_equal(bank.pose_avg, d["pose_avg"])
    assert bank.file_paths == d["file_paths"]


def test_gather_meets_the_reference(bank, g25):
    o = g25.outputs
    n = bank.n_rays
    assert n == len(o["rays"]) == 6 * 48
    idx = torch.arange(n - 1, -1, -1, dtype=torch.int64, device="cuda")           # every ray, in another order than stored
    rays, rgbs, mask = (t.cpu().numpy()[::-1] for t in bank.gather(idx))
    assert np.array_equal(rgbs, o["rgbs"])
    assert np.array_equal(mask, o["mirror_mask"])
    err = float(np.abs(rays[:, :6] - o["rays"][:, :6]).max())
    print(f"rays: max abs difference {err:.3e}")
    assert err <= 1e-6
    assert np.array_equal(rays[:, 6:], o["rays"][:, 6:])                          # near and far
    f = SC.RGBA_FRAME
    assert np.array_equal(bank.frame(f)["valid_mask"].cpu().numpy(), o["valid_mask_rgba_frame"])
    assert bank.select("with_mask").frame_ids == o["frames_with_mask"].tolist()


def test_other_splits_and_a_three_channel_bank(scene, bank):
    from mirror_nerf_amd.data import RayBank, read_arkit
    v = RayBank.from_arkit(scene, "val", *ARGS, val_idx=SC.VAL_IDX)
    d = read_arkit(scene, "val", *ARGS, val_idx=SC.VAL_IDX)
    assert v.channels == 3 and v.n_frames == 1 and np.array_equal(v.images.cpu().numpy(), d["images"])
    assert np.array_equal(v.masks.cpu().numpy(), d["masks"]) and v.focal == d["focal"]
    s = RayBank.from_arkit(scene, "train", *ARGS, val_idx=SC.VAL_IDX, train_skip_step=2)
    assert s.channels == 3 and np.array_equal(s.images.cpu().numpy(), bank.images[::2, ..., :3].cpu().numpy())
    with pytest.raises(ValueError, match="poses only"):
        RayBank.from_arkit(scene, "test_rotate", *ARGS)


@pytest.mark.parametrize("split", ["test_rotate", "test_interpolation"])
def test_path_split_rays(scene, split):
    from mirror_nerf_amd import synthetic
    from mirror_nerf_amd.data import read_arkit
    fx = Fixture("g24_arkit_paths")
    d = read_arkit(scene, split, *ARGS, val_idx=SC.VAL_IDX)
    w, h = SC.IMG_WH
    for i in fx.meta["rays_of"]:
        got = synthetic.generate_rays(h, w, d["focal"], d["poses"][i], d["near"], d["far"], "cuda").cpu().numpy()
        want = fx.outputs[f"{split}__rays_{i}"]
        err = float(np.abs(got[:, :6] - want[:, :6]).max())
        print(f"{split} frame {i}: max abs difference {err:.3e}")
        assert err <= 1e-6 and np.array_equal(got[:, 6:], want[:, 6:])


def test_eval_scene_renders_the_interpolated_path(scene, tmp_path, capsys):
    """scripts/eval_scene.py --dataset_name real_arkit --split test_interpolation on the fixture scene: 64 frames under the
    reference's names and the GIF of 64 frames; no ground truth, so no PSNR line.  Frame 5 decodes to what the same rays give
    by hand."""
    import importlib.util
    import os
    from types import SimpleNamespace
    from PIL import Image
    import mirror_nerf_amd as M
    from mirror_nerf_amd import checkpoint, synthetic
    from mirror_nerf_amd.data import read_arkit
    models = synthetic.build_models("cuda:0", synthetic.STRADDLE, seed=0)[0]
    ckpt = tmp_path / "last.ckpt"
    checkpoint.save_ckpt(str(ckpt), SimpleNamespace(nerf_coarse=models["coarse"], nerf_fine=models["fine"]))
    out = tmp_path / "results" / "lounge_exp"
    argv = ["--root_dir", scene, "--dataset_name", "real_arkit", "--split", "test_interpolation", "--img_wh", "8", "6",
            "--scale_factor", str(SC.SCALE_FACTOR), "--val_idx", str(SC.VAL_IDX), "--near", str(SC.NEAR), "--far", str(SC.FAR),
            "--ckpt_path", str(ckpt), "--N_samples", "64", "--N_importance", "64", "--chunk", "32768", "--trace_secondary_rays",
            "--out_dir", str(out)]
    spec = importlib.util.spec_from_file_location("eval_scene", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                             "scripts", "eval_scene.py"))
    ES = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ES)
    assert ES.main(argv) == 0
    assert "PSNR" not in capsys.readouterr().out
    for i in range(64):
        assert (out / f"rgb_fine_{i:03d}.png").is_file() and (out / "depth" / f"depth_fine_{i:03d}.png").is_file(), i
    assert not (out / "rgb_fine_064.png").exists()
    gif = Image.open(out / "lounge_exp_rgb_fine.gif")
    assert gif.n_frames == 64 and gif.size == (8, 6) and gif.info["duration"] in (60, 70)
    args = ES.get_opts(argv)
    d = read_arkit(scene, "test_interpolation", *ARGS, val_idx=SC.VAL_IDX)
    rays = synthetic.generate_rays(6, 8, d["focal"], d["poses"][5], d["near"], d["far"], torch.device("cuda:0"))
    images = M.finish_frame(ES.render(ES.load_system(args, torch.device("cuda:0")), rays, args), "fine")
    png = np.asarray(Image.open(out / "rgb_fine_005.png"))
    assert png.shape == (6, 8, 3) and (png.reshape(48, 3) == images["rgb_fine"].cpu().numpy()).all()
