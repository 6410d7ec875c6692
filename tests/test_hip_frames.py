"""The output stage of eval.py on the device (csrc/mnrf_frames.hip, mirror_nerf_amd/frames.py) against tests/frames_ref.py, the
numpy restatement of eval.py:743-978.  EQUALITY IS EXACT: every uint8 image and every extremum must be numpy's, bit for bit,
over every pixel.  The tolerance of zero is derived, not measured: every step of every image is one IEEE fp32 elementwise
operation (the kernels are compiled without contraction and with correctly rounded division), the casts are truncations of
values inside [0, 256), and min / max do not depend on the order of reduction.

Shapes: 1 x 1; 23 x 37 (odd: 3-byte rows never align to a dword; fewer pixels than one block of 256 threads x 4 pixels; not a
multiple of a wave); 67 x 130 (several blocks and a tail).  Those fit every grid uncapped (26 blocks at the most).  Past the caps:
n = 1 400 003 (3 n / 1024 = 4102 blocks wanted: frame_finish_kernel's cap of 4096 and frame_extrema_kernel's of 1024 are both
reached, so the flat three-channel loops and the reduction stride, with n and 3 n no multiples of 4 and a storage offset of 1;
a second frame of that size has its extremes only where a thread's second or later value lies); n = 4 200 003 (n / 1024 = 4102:
the per-pixel loops of frame_finish_kernel -- mirror mask, depth_image, store_pixels -- and of depth_colormap_kernel sweep
twice, the latter over a stack of two frames of different ranges, whose own extremes come from a capped extrema launch with
one stats block per frame).  Each of these tests asserts that reach from its n."""
import importlib.util
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import frames_ref as FR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"rgb": "rgb_fine", "mirror_mask": "mirror_mask_fine", "depth": "depth_fine", "depth_reflect": "depth_fine_reflect",
        "surface_normal": "surface_normal_fine", "surface_normal_grad": "surface_normal_grad_fine", "x_surface": "x_surface_fine"}


def _table(seed=5):
    return np.random.default_rng(seed).integers(0, 256, size=(256, 3), dtype=np.uint8)


def _results(maps):
    return {KEYS[k]: v for k, v in maps.items()}


def _to_device(maps, offset=0):
    """Device tensors of the maps; with `offset`, views that start `offset` elements into a larger allocation (a non-zero
    storage offset: 4-byte but not 16-byte aligned)."""
    out = {}
    for k, v in maps.items():
        t = torch.from_numpy(v)
        if offset:
            big = torch.full((v.size + offset + 5,), -7.0, dtype=torch.float32, device=DEV)
            view = big[offset:offset + v.size].view(v.shape)
            view.copy_(t)
            assert view.storage_offset() == offset
            out[k] = view
        else:
            out[k] = t.to(DEV)
    return out


def _extrema(dev_maps, running=None):
    """The six extremes of the stats block after one extrema launch, as float32 numpy (x_surface may be absent: a null map)."""
    from mirror_nerf_amd import _lib
    L = _lib.lib()
    stats = torch.zeros(L.mnrf_frame_stats_floats(), dtype=torch.float32, device=DEV)
    n = dev_maps["depth"].shape[0]
    _lib.check(L.mnrf_frame_extrema(dev_maps["depth"].data_ptr(), dev_maps["depth_reflect"].data_ptr(),
                                    dev_maps["x_surface"].data_ptr() if "x_surface" in dev_maps else None, n, stats.data_ptr(),
                                    None if running is None else running.data_ptr(), _lib.stream()), "mnrf_frame_extrema")
    s = stats.cpu().numpy()
    assert not s[8:].view(np.uint32).any()       # the reduction's state is left zero for the next launch
    return s[:6]


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _want_extrema(maps):
    return np.array([*FR.depth_extrema(maps["depth"]), *FR.depth_extrema(maps["depth_reflect"]),
                     *FR.x_surface_extrema(maps["x_surface"])], np.float32)


def _check_frame(maps, table, offset=0):
    from mirror_nerf_amd import frames
    dev = _to_device(maps, offset)
    before = {k: v.clone() for k, v in dev.items()}
    got = frames.finish_frame(_results(dev), "fine", table=table)
    want = FR.frame_images(_results(maps), table)
    assert set(got) == set(want) and len(got) == 7
    for k in want:
        g = got[k].cpu().numpy()
        assert g.dtype == np.uint8 and g.shape == want[k].shape
        bad = np.flatnonzero((g != want[k]).any(axis=1))
        assert bad.size == 0, (k, bad[:5], g[bad[:5]], want[k][bad[:5]])
    assert (_bits(_extrema(dev)) == _bits(_want_extrema(maps))).all()
    for k in dev:                                 # the maps are read in place and left as they were
        assert torch.equal(dev[k].view(-1).view(torch.int32), before[k].view(-1).view(torch.int32)), k
    return got


CASES = [  # (H, W, storage offset, seeded_maps keywords)
    (1, 1, 0, {}),
    (23, 37, 1, dict(nonfinite="nan")),
    (23, 37, 0, dict(nonfinite="all")),
    (23, 37, 3, dict(constant_depth=True, constant_xs=True)),
    (67, 130, 0, dict(nonfinite="nan")),
    (67, 130, 2, dict(nonfinite="inf")),
    (67, 130, 0, dict(nonfinite="none")),
]


@pytest.mark.parametrize("H,W,offset,kw", CASES)
def test_images_and_extrema_equal_numpy(H, W, offset, kw):
    maps = FR.seeded_maps(H * W, seed=H * 1000 + W + offset, **kw)
    _check_frame(maps, _table(), offset)


# ----------------------------------------------------------------------------- past the caps of the grids
# blocks_for(items, 4 per thread, cap) of csrc/mnrf_frames.hip: a block covers 256 * 4 = 1024 items of a loop's first sweep.
FINISH_CAP, EXTREMA_CAP = 4096, 1024
N_FLAT = 1_400_003           # 3 n floats: the flat loops of frame_finish_kernel sweep twice
N_PIXEL = 4_200_003          # n pixels: its per-pixel loops, and depth_colormap_kernel's, sweep twice


def _blocks(items):
    return -(-items // 1024)


def test_flat_loops_past_the_grid_caps():
    """rgb, the normals and x_surface on the second sweep of a grid capped at 4096 blocks, the extrema launch at its cap of
    1024; n is no multiple of 4 and the maps start 4 bytes past a 16-byte boundary, so the tails and the scalar loads run."""
    n = N_FLAT
    assert _blocks(3 * n) > FINISH_CAP and _blocks(3 * n) > EXTREMA_CAP and n % 4 != 0 and (3 * n) % 4 != 0
    _check_frame(FR.seeded_maps(n, seed=41, nonfinite="all"), _table(), 1)


def test_extremes_that_only_the_later_sweeps_see():
    """The extrema launch has 1024 * 256 threads and each takes one value per sweep: the minimum and the maximum of both
    depths and of x_surface are put at flat positions from 1024 * 256 on, where only a thread's second or later value finds
    them -- one of them in the last three elements of its map."""
    n = N_FLAT
    first_sweep = EXTREMA_CAP * 256
    assert _blocks(n) > EXTREMA_CAP and _blocks(3 * n) > FINISH_CAP
    maps = FR.seeded_maps(n, seed=42, nonfinite="none")
    places = {"depth": (n - 2, first_sweep + 37_856), "depth_reflect": (first_sweep, n - 1),
              "x_surface": (3 * n - 1, first_sweep + 3 * 4096 * 256 + 5)}          # (minimum, maximum), flat
    for k, (lo, hi) in places.items():
        flat = maps[k].reshape(-1)
        assert np.shares_memory(flat, maps[k])                                       # a view: the edit lands in the map
        flat[lo], flat[hi] = flat.min() - np.float32(1.5), flat.max() + np.float32(2.5)
    for k, (lo, hi) in places.items():
        flat = maps[k].reshape(-1)
        assert min(lo, hi) >= first_sweep and max(lo, hi) < flat.size
        assert int(np.argmin(flat)) == lo and int(np.argmax(flat)) == hi
        assert (flat == flat[lo]).sum() == 1 and (flat == flat[hi]).sum() == 1
    assert any(p >= maps[k].size - 3 for k, pair in places.items() for p in pair)
    assert (_want_extrema(maps) == [maps[k].reshape(-1)[p] for k in places for p in places[k]]).all()
    _check_frame(maps, _table())


@pytest.fixture(scope="module")
def pixel_frames():
    """Two frames of N_PIXEL pixels with the maps the per-pixel images need (and rgb, without which nothing is emitted): the
    second is the first reversed, its depth squared and its reflected depth shifted, so the frames' ranges differ.  NaN only:
    with an infinity the range overflows and every pixel gets the same colour."""
    n = N_PIXEL
    assert _blocks(n) > FINISH_CAP and n % 4 != 0
    first = {k: v for k, v in FR.seeded_maps(n, seed=43, nonfinite="nan").items() if k in ("rgb", "mirror_mask", "depth", "depth_reflect")}
    second = {k: np.ascontiguousarray(v[::-1]) for k, v in first.items() if k != "rgb"}
    second["depth"] = (second["depth"] * second["depth"] * np.float32(0.125)).astype(np.float32)      # not a rescaling: another image
    second["depth_reflect"] = (second["depth_reflect"] + np.float32(1.5)).astype(np.float32)
    return first, second


def test_per_pixel_loops_past_the_grid_cap(pixel_frames):
    """mirror_mask, depth and depth_reflect of frame_finish_kernel on their second sweep (4 pixels per thread, 4096 blocks)."""
    from mirror_nerf_amd import frames
    maps, _ = pixel_frames
    n, T = N_PIXEL, _table(6)
    assert _blocks(n) > FINISH_CAP
    dev = _to_device(maps)
    stems = ["mirror_mask", "depth", "depth_reflect"]
    got = frames.finish_frame(_results(dev), "fine", table=T, want=stems)
    want = FR.frame_images(_results(maps), T)
    assert set(got) == {"mirror_mask_fine", "depth_fine", "depth_reflect_fine"} and set(got) | {"rgb_fine"} == set(want)
    for k in got:
        g = got[k].cpu().numpy()
        assert g.dtype == np.uint8 and g.shape == want[k].shape == (n, 3)
        bad = np.flatnonzero((g != want[k]).any(axis=1))
        assert bad.size == 0, (k, bad.size, bad[:5], g[bad[:5]], want[k][bad[:5]])
        assert len(np.unique(g[:, 0])) > 16                    # an image, not one colour
    ex = _extrema(dev)                                         # without x_surface; asserts the reduction's state is zero again
    want_ex = np.array([*FR.depth_extrema(maps["depth"]), *FR.depth_extrema(maps["depth_reflect"])], np.float32)
    assert (_bits(ex[:4]) == _bits(want_ex)).all() and np.isnan(ex[4:6]).all()
    for k in dev:
        assert dev[k].cpu().numpy().tobytes() == maps[k].tobytes(), k


@pytest.mark.parametrize("masked", [False, True], ids=["depth", "depth_reflect"])
@pytest.mark.parametrize("own", [False, True], ids=["given_extremes", "own_extremes"])
def test_depth_stack_past_the_grid_cap(pixel_frames, own, masked):
    """depth_colormap_kernel on its second sweep over a stack of two frames of different ranges: with the frames' own
    extremes (the extrema launch at its cap, one stats block per frame) and with a given pair that clips both frames."""
    from mirror_nerf_amd import frames
    n, T = N_PIXEL, _table(7)
    assert _blocks(n) > FINISH_CAP and _blocks(n) > EXTREMA_CAP
    key = "depth_reflect" if masked else "depth"
    stack = torch.from_numpy(np.stack([m[key] for m in pixel_frames])).to(DEV)
    masks = torch.from_numpy(np.stack([m["mirror_mask"] for m in pixel_frames])).to(DEV) if masked else None
    pair = (None, None) if own else ((1.0, 7.5) if masked else (2.5, 5.0))
    if own:
        ranges = [FR.depth_extrema(m[key]) for m in pixel_frames]
        assert ranges[0][0] != ranges[1][0] or ranges[0][1] != ranges[1][1]
    ex = None if own else torch.tensor(pair, dtype=torch.float32, device=DEV)
    got = frames.colormap_depth(stack, ex, masks, table=T)
    assert tuple(got.shape) == (2, n, 3) and got.dtype == torch.uint8
    got = got.cpu().numpy()
    for f, m in enumerate(pixel_frames):
        want = FR.depth_reflect_image(m[key], m["mirror_mask"], T, *pair) if masked else FR.depth_image(m[key], T, *pair)
        bad = np.flatnonzero((got[f] != want).any(axis=1))
        assert bad.size == 0, (f, bad.size, bad[:5], got[f][bad[:5]], want[bad[:5]])
    assert (got[0] != got[1][::-1]).any()


def test_default_table_is_jet():
    from mirror_nerf_amd import frames
    maps = FR.seeded_maps(23 * 37, seed=11, nonfinite="nan")
    got = _check_frame(maps, frames.jet_table())
    dflt = frames.finish_frame(_results(_to_device(maps)), "fine")
    for k in got:
        assert torch.equal(got[k], dflt[k]), k


def test_nan_in_x_surface_propagates():
    """torch.min / torch.max of a map with a NaN are NaN: min == max is false, every value becomes NaN and every byte 0."""
    from mirror_nerf_amd import frames
    maps = FR.seeded_maps(300, seed=3, nonfinite="none")
    maps["x_surface"][17, 1] = np.nan
    dev = _to_device(maps)
    assert np.isnan(_extrema(dev)[4:6]).all() and np.isnan(_want_extrema(maps)[4:6]).all()
    got = frames.finish_frame(_results(dev), "fine", table=_table(), want=["x_surface"])
    assert list(got) == ["x_surface_fine"]
    assert (got["x_surface_fine"].cpu().numpy() == FR.x_surface_image(maps["x_surface"])).all()


def test_presence_rules_and_want():
    from mirror_nerf_amd import frames
    maps = FR.seeded_maps(50, seed=4, nonfinite="none")
    dev = _results(_to_device(maps))
    T = _table()
    no_mask = {k: v for k, v in dev.items() if k != "mirror_mask_fine"}
    assert set(frames.finish_frame(no_mask, "fine", table=T)) == {"rgb_fine", "depth_fine", "surface_normal_fine",
                                                                 "surface_normal_grad_fine", "x_surface_fine"}
    assert frames.finish_frame({k: v for k, v in dev.items() if k != "rgb_fine"}, "fine", table=T) == {}
    few = frames.finish_frame({"rgb_fine": dev["rgb_fine"], "depth_fine": dev["depth_fine"]}, "fine", table=T)
    assert set(few) == {"rgb_fine", "depth_fine"}
    assert (few["depth_fine"].cpu().numpy() == FR.depth_image(maps["depth"], T)).all()
    coarse = frames.finish_frame({"rgb_coarse": dev["rgb_fine"]}, "coarse")
    assert list(coarse) == ["rgb_coarse"] and (coarse["rgb_coarse"].cpu().numpy() == FR.rgb_image(maps["rgb"])).all()
    with pytest.raises(ValueError):
        frames.finish_frame(dev, "fine", want=["colour"])
    with pytest.raises(ValueError):
        frames.finish_frame(dict(dev, depth_fine=dev["depth_fine"][:-1]), "fine")


def test_three_frame_split():
    """The running block after frames 0, 1 and 2 (frame 1 holds NaN in both depths and must change nothing), the unified
    pass with it, the per-frame pass with extrema=None, and the masked variant."""
    from mirror_nerf_amd import frames
    n, T = 23 * 37, _table(9)
    split = [FR.seeded_maps(n, seed=20, nonfinite="none"), FR.seeded_maps(n, seed=21, nonfinite="nan"),
             FR.seeded_maps(n, seed=22, nonfinite="none")]
    split[0]["depth"] = (split[0]["depth"] + np.float32(1.5)).astype(np.float32)        # frames of different ranges
    split[2]["depth"] = (split[2]["depth"] * np.float32(0.5)).astype(np.float32)
    dev = [_to_device(m) for m in split]
    ex = frames.SplitExtrema(DEV)
    rd, rr = FR.RunningExtrema(), FR.RunningExtrema()
    assert ex.values() == dict(depth_min=np.inf, depth_max=-np.inf, depth_reflect_min=np.inf, depth_reflect_max=-np.inf)
    for m, d in zip(split, dev):
        frames.finish_frame(_results(d), "fine", table=T, split_extrema=ex)
        rd.update(m["depth"])
        rr.update(m["depth_reflect"])
        v = ex.values()
        got = [v["depth_min"], v["depth_max"], v["depth_reflect_min"], v["depth_reflect_max"]]
        assert (_bits(got) == _bits([rd.min, rd.max, rr.min, rr.max])).all(), (got, rd.min, rd.max, rr.min, rr.max)
    assert np.isfinite([rd.min, rd.max, rr.min, rr.max]).all()
    only0 = FR.RunningExtrema().update(split[0]["depth"]).update(split[2]["depth"])
    assert (rd.min, rd.max) == (only0.min, only0.max)      # the frame with the NaN changed nothing

    depth = torch.stack([d["depth"] for d in dev])
    refl = torch.stack([d["depth_reflect"] for d in dev])
    mask = torch.stack([d["mirror_mask"] for d in dev])
    uni = frames.colormap_depth(depth, ex.depth, table=T).cpu().numpy()
    uni_r = frames.colormap_depth(refl, ex.depth_reflect, mask, table=T).cpu().numpy()
    own = frames.colormap_depth(depth, table=T).cpu().numpy()
    own_r = frames.colormap_depth(refl, None, mask, table=T).cpu().numpy()
    assert uni.shape == (3, n, 3) and uni.dtype == np.uint8
    for f, m in enumerate(split):
        assert (uni[f] == FR.depth_image(m["depth"], T, rd.min, rd.max)).all(), f
        assert (uni_r[f] == FR.depth_reflect_image(m["depth_reflect"], m["mirror_mask"], T, rr.min, rr.max)).all(), f
        assert (own[f] == FR.depth_image(m["depth"], T)).all(), f
        assert (own_r[f] == FR.depth_reflect_image(m["depth_reflect"], m["mirror_mask"], T)).all(), f
    assert (uni != own).any()                              # the two normalisations are different images
    one = frames.colormap_depth(dev[1]["depth"], table=T)
    assert one.shape == (n, 3) and (one.cpu().numpy() == own[1]).all()
    # an infinity counts; reset() starts over
    inf_maps = FR.seeded_maps(n, seed=23, nonfinite="inf")
    frames.finish_frame(_results(_to_device(inf_maps)), "fine", table=T, split_extrema=ex.reset())
    want = FR.RunningExtrema().update(inf_maps["depth"])
    assert ex.values()["depth_max"] == np.inf == want.max and ex.values()["depth_min"] == want.min


def test_two_runs_are_identical():
    from mirror_nerf_amd import frames
    maps = FR.seeded_maps(67 * 130, seed=31, nonfinite="all")
    dev = _to_device(maps)
    T = _table()
    runs = []
    for _ in range(2):
        ex = frames.SplitExtrema(DEV)
        imgs = frames.finish_frame(_results(dev), "fine", table=T, split_extrema=ex)
        runs.append(({k: v.clone() for k, v in imgs.items()}, _extrema(dev).copy(), ex.block.clone()))
    for k in runs[0][0]:
        assert torch.equal(runs[0][0][k], runs[1][0][k]), k
    assert (_bits(runs[0][1]) == _bits(runs[1][1])).all()
    assert torch.equal(runs[0][2].view(torch.int32), runs[1][2].view(torch.int32))


def _models():
    from mirror_nerf_amd import synthetic as SY
    return SY.build_models(DEV, SY.STRADDLE, seed=0)[0]


def test_finish_frame_on_a_rendered_frame():
    """batched_inference(to_cpu=False, maps_only=True) at 8 x 8 rays with the seeded weights of the other GPU tests: the
    images of the dict it returns equal the restatement applied to the same dict copied to the host, and the keys follow the
    presence rules."""
    import mirror_nerf_amd as M
    from mirror_nerf_amd import synthetic as SY
    rays = SY.device_rays(8, 8, DEV)
    args = dict(predict_normal=True, only_one_field=False, only_one_field_fine_epoch=2, max_recursive_level=1)
    emb = {"xyz": M.Embedding(10), "dir": M.Embedding(4)}
    res = M.batched_inference(_models(), emb, rays, 64, 64, False, 32768, args=args, trace_secondary_rays=True, to_cpu=False,
                              maps_only=True)
    assert res["rgb_fine"].is_cuda and res["rgb_fine"].shape == (64, 3)
    host = {k: v.cpu().numpy() for k, v in res.items()}
    T = _table(2)
    got = M.finish_frame(res, "fine", table=T)
    want = FR.frame_images(host, T)
    assert set(got) == set(want)
    assert {"rgb_fine", "depth_fine", "mirror_mask_fine", "depth_reflect_fine", "x_surface_fine"} <= set(got)
    for k in want:
        assert (got[k].cpu().numpy() == want[k]).all(), k
    for k, v in res.items():
        assert v.cpu().numpy().tobytes() == host[k].tobytes(), k          # the maps are left as they were


def _load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_eval_scene_writes_the_reference_layout(tmp_path, capsys):
    """scripts/eval_scene.py end to end on a Blender-layout directory of 2 frames of 8 x 8: the reference's file names exist
    and rgb_fine_000.png decodes to the bytes finish_frame gives for that frame."""
    from PIL import Image
    import mirror_nerf_amd as M
    from mirror_nerf_amd import checkpoint
    from mirror_nerf_amd import synthetic as SY
    from mirror_nerf_amd.data import RayBank
    root = tmp_path / "scene"
    (root / "test").mkdir(parents=True)
    rng = np.random.default_rng(0)
    frames_meta = []
    for i, eye in enumerate(((0.0, -4.0, 1.5), (1.0, -3.5, 2.0))):
        Image.fromarray(rng.integers(0, 256, size=(8, 8, 3), dtype=np.uint8)).save(root / "test" / f"r_{i}.png")
        pose = np.eye(4)
        pose[:3, :4] = SY.look_at_pose(eye=eye)
        frames_meta.append({"file_path": f"./test/r_{i}", "transform_matrix": pose.tolist()})
    with open(root / "transforms_test.json", "w") as f:
        json.dump({"camera_angle_x": SY.CAMERA_ANGLE_X, "frames": frames_meta}, f)
    models = _models()
    ckpt = tmp_path / "last.ckpt"
    checkpoint.save_ckpt(str(ckpt), SimpleNamespace(nerf_coarse=models["coarse"], nerf_fine=models["fine"]))
    out = tmp_path / "results"
    argv = ["--root_dir", str(root), "--split", "test", "--img_wh", "8", "8", "--ckpt_path", str(ckpt), "--N_samples", "64",
            "--N_importance", "64", "--chunk", "32768", "--trace_secondary_rays", "--depth_format", "png_pfm_bytes",
            "--near", str(SY.NEAR), "--far", str(SY.FAR), "--out_dir", str(out)]
    ES = _load_script("eval_scene")
    assert ES.main(argv) == 0
    assert "Mean PSNR (fine):" in capsys.readouterr().out
    for i in range(2):
        for rel in (f"rgb_fine_{i:03d}.png", f"depth/depth_fine_{i:03d}.png", f"depth/depth_fine_{i:03d}.pfm",
                    f"depth/depth_fine_{i:03d}", f"mirror_mask/mirror_mask_fine_{i:03d}.png",
                    f"depth_reflect/depth_reflect_fine_{i:03d}.png", f"normal/surface_normal_fine_{i:03d}.png",
                    f"x_surface/x_surface_fine_{i:03d}.png", f"depth_unified_normalization/depth_fine_{i:03d}.png",
                    f"depth_reflect_unified_normalization/depth_reflect_fine_{i:03d}.png"):
            assert (out / rel).is_file(), rel
    assert os.path.getsize(out / "depth" / "depth_fine_000") == 64 * 4
    # the same frame again, by hand
    args = ES.get_opts(argv)
    system = ES.load_system(args, torch.device(DEV))
    bank = RayBank.from_blender(str(root), "test", (8, 8), SY.NEAR, SY.FAR, device=torch.device(DEV))
    images = M.finish_frame(ES.render(system, bank.frame(0)["rays"], args), "fine")
    png = np.asarray(Image.open(out / "rgb_fine_000.png"))
    assert png.shape == (8, 8, 3) and (png.reshape(64, 3) == images["rgb_fine"].cpu().numpy()).all()
    png = np.asarray(Image.open(out / "depth" / "depth_fine_000.png"))
    assert (png.reshape(64, 3) == images["depth_fine"].cpu().numpy()).all()
