"""The ray bank on the device (csrc/mnrf_bank.hip through mirror_nerf_amd.data.RayBank).

Everything is compared exactly: gathered rays against mnrf_generate_rays of the same pose (one shared device function, bit for
bit), colours and masks against the same float32 expressions in torch on the CPU (IEEE division, multiply, subtract, add; no
contraction on either side), drawn indices against the integer restatement tests/raybank_ref.py.  The one tolerance is fixture
G12's own 1e-6 on rays captured from the reference.  Shapes: odd, non-square frames (37 x 53, 5 x 7), N not a power of two,
batches that divide neither N nor the 256-thread block."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import raybank_ref as R
from tests.golden import fixtures as FX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR, FAR = 0.05, 8.0


def _poses(n, seed=0):
    from mirror_nerf_amd import synthetic as SY
    rng = np.random.default_rng(seed)
    return np.stack([SY.look_at_pose(eye=tuple(rng.uniform(-3, 3, 2)) + (rng.uniform(1, 3),)) for _ in range(n)])


def _arrays(F, H, W, C, seed=0):
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 256, (F, H, W, C), dtype=np.uint8)
    images[:, 0, :5, C - 1] = (0, 255, 1, 254, 128)          # alpha (or blue): both ends and values between
    masks = rng.integers(0, 2, (F, H, W)).astype(np.int8)
    masks[F - 1] = -1                                        # the last frame has no ground-truth mask
    return _poses(F, seed), images, masks


def _bank(F=3, H=37, W=53, C=4, seed=0):
    from mirror_nerf_amd.data import RayBank
    poses, images, masks = _arrays(F, H, W, C, seed)
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    return RayBank(poses, images, masks, focal, NEAR, FAR, DEV), (poses, images, masks, focal)


@pytest.fixture(scope="module")
def bank():
    return _bank()


def _frame_rays(H, W, focal, pose):
    from mirror_nerf_amd import _lib
    rays = torch.empty(H * W, 8, device=DEV)
    c2w = (ctypes.c_float * 12)(*np.asarray(pose, np.float32).reshape(-1).tolist())
    _lib.check(_lib.lib().mnrf_generate_rays(H, W, float(focal), c2w, NEAR, FAR, _lib.ptr(rays), _lib.stream()), "mnrf_generate_rays")
    return rays


def _expected_colour(images, masks):
    """The reference's expressions in float32 torch on the CPU (blender.py:128-133, 129, 153-156), flattened over the frames."""
    img = torch.from_numpy(images).reshape(-1, images.shape[-1]).float().div(255)          # ToTensor
    valid = img[:, -1] > 0
    if images.shape[-1] == 4:
        img = img[:, :3] * img[:, -1:] + (1 - img[:, -1:])
    return img, torch.from_numpy(masks).reshape(-1).float(), valid


def test_rays_equal_the_frame_kernel(bank):
    b, (poses, _, _, focal) = bank
    hw = b.H * b.W
    assert (b.n_frames, b.n_rays) == (3, 3 * hw)
    rays, _, _ = b.gather(torch.arange(b.n_rays, device=DEV))
    for f in range(3):
        want = _frame_rays(b.H, b.W, focal, poses[f])
        assert torch.equal(rays[f * hw:(f + 1) * hw], want), f
        assert torch.equal(b.frame(f)["rays"], want), f


def test_rays_against_fixture_g12():
    from mirror_nerf_amd.data import RayBank
    fx = FX.Fixture("g12_rays_37x53")
    m = fx.meta
    H, W = m["H"], m["W"]
    focal = 0.5 * W / np.tan(0.5 * (2 * np.arctan(0.5 * W / m["focal"])))          # as test_generate_rays_golden derives it
    b = RayBank(np.asarray(fx.inputs["pose"], np.float32)[None, :3, :4], np.zeros((1, H, W, 3), np.uint8), None, focal,
                m["near"], m["far"], DEV)
    rays = b.frame(0)["rays"].cpu().numpy()
    want = fx.outputs["rays"]
    assert rays.shape == want.shape
    err = float(np.max(np.abs(rays[:, :6] - want[:, :6])))
    print("g12_rays_37x53 through the bank: max abs difference", err)
    assert err <= 1e-6
    assert np.array_equal(rays[:, 6:], want[:, 6:])


@pytest.mark.parametrize("C", [4, 3])
def test_colour_and_masks_equal_the_reference_expressions(C):
    b, (_, images, masks, _) = _bank(C=C, seed=C)
    want_rgb, want_mask, want_valid = _expected_colour(images, masks)
    hw = b.H * b.W
    _, rgbs, mask = b.gather(torch.arange(b.n_rays, device=DEV))
    assert torch.equal(rgbs.cpu(), want_rgb) and torch.equal(mask.cpu(), want_mask)
    assert set(mask.unique().tolist()) == {-1.0, 0.0, 1.0}
    for f in range(3):
        d = b.frame(f)
        assert d["valid_mask"].dtype == torch.bool and d["valid_mask"].shape == (hw,)
        assert torch.equal(d["valid_mask"].cpu(), want_valid[f * hw:(f + 1) * hw])
        assert torch.equal(d["rgbs"].cpu(), want_rgb[f * hw:(f + 1) * hw]) and torch.equal(d["mirror_mask"].cpu(), want_mask[f * hw:(f + 1) * hw])
    assert not want_valid.all() and want_valid.any()


def test_gather_takes_any_order_and_marks_bad_indices(bank):
    b, _ = bank
    full = b.gather(torch.arange(b.n_rays, device=DEV))
    idx = torch.tensor([b.n_rays - 1, 0, 1234, 1234, 5], device=DEV)
    for got, ref in zip(b.gather(idx), full):
        assert torch.equal(got, ref[idx])
    rays, rgbs, mask = b.gather(torch.tensor([-1, b.n_rays, 7], device=DEV))
    assert rays[:2].isnan().all() and rgbs[:2].isnan().all() and mask[:2].isnan().all()
    assert torch.equal(rays[2], full[0][7]) and torch.equal(rgbs[2], full[1][7])
    empty = b.gather(torch.empty(0, dtype=torch.int64, device=DEV))
    assert [tuple(t.shape) for t in empty] == [(0, 8), (0, 3), (0,)]


@pytest.mark.parametrize("F,H,W,B,steps", [(3, 5, 7, 16, 20), (3, 37, 53, 1000, 8)])
def test_drawn_indices_equal_the_restatement(F, H, W, B, steps):
    b, _ = _bank(F, H, W)
    n = F * H * W
    assert steps * B > n and n % B != 0          # an epoch ends inside a batch
    for seed in (0, 2 ** 40 + 12345):
        for s in range(steps):
            idx = b.draw(s, B, seed, rank=0, world=1, return_indices=True)[3]
            assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), R.draw_indices(n, s, B, seed)), (seed, s)


def test_stream_covers_every_ray_once_per_epoch():
    b, _ = _bank(3, 5, 7)
    n, B = b.n_rays, 16
    got = torch.cat([b.draw(s, B, 5, rank=0, world=1, return_indices=True)[3] for s in range(14)]).cpu().numpy()[:2 * n]
    assert got.size == 2 * n == 210
    assert np.array_equal(np.sort(got[:n]), np.arange(n)) and np.array_equal(np.sort(got[n:]), np.arange(n))
    assert not np.array_equal(got[:n], got[n:])
    assert [b.epoch_of(s, 15, 1) for s in (0, 6, 7, 13, 14)] == [0, 0, 1, 1, 2] and b.epoch_of(3, 15, 2) == 0 and b.epoch_of(4, 15, 2) == 1


def test_draw_equals_gather_of_the_drawn_indices(bank):
    b, _ = bank
    B = 1000
    out = (torch.zeros(B, 8, device=DEV), torch.zeros(B, 3, device=DEV), torch.zeros(B, device=DEV))
    res = b.draw(5, B, 9, rank=0, world=1, out=out, return_indices=True)          # step 5 of 1000 crosses the end of epoch 0 (N = 5883)
    assert all(r is o for r, o in zip(res[:3], out))
    for got, want in zip(out, b.gather(res[3])):
        assert torch.equal(got, want)
    assert not out[0].isnan().any()


def test_ranks_split_the_stream(bank):
    b, _ = bank
    B = 300
    for s in (0, 9, 10):          # N = 5883: the batch of 600 at step 9 crosses into epoch 1
        whole = b.draw(s, 2 * B, 4, rank=0, world=1, return_indices=True)
        parts = [b.draw(s, B, 4, rank=r, world=2, return_indices=True) for r in range(2)]
        for k in range(4):
            assert torch.equal(torch.cat([parts[0][k], parts[1][k]]), whole[k]), (s, k)


def test_frame_selection():
    b, _ = _bank(4, 5, 7)
    hw, B = 35, 16
    assert b.frames_with_mask == [0, 1, 2] and b.select("with_mask").frame_ids == [0, 1, 2]
    sel = b.select([2, 0])
    assert (sel.n_frames, sel.n_rays, b.n_frames) == (2, 2 * hw, 4)
    full = b.gather(torch.arange(b.n_rays, device=DEV))
    idx = torch.cat([sel.draw(s, B, 1, rank=0, world=1, return_indices=True)[3] for s in range(5)])[:2 * hw]      # one epoch
    assert np.array_equal(np.sort(idx.cpu().numpy()), np.arange(2 * hw))
    # slot 0 is frame 2, slot 1 is frame 0: the epoch covers exactly their pixels
    pixels = torch.where(idx < hw, 2 * hw + idx, idx - hw)
    assert np.array_equal(np.sort(pixels.cpu().numpy()), np.concatenate([np.arange(hw), np.arange(2 * hw, 3 * hw)]))
    for got, ref in zip(sel.gather(idx), full):
        assert torch.equal(got, ref[pixels])
    assert torch.equal(sel.frame(0)["rays"], b.frame(2)["rays"]) and torch.equal(sel.frame(1)["rgbs"], b.frame(0)["rgbs"])
    assert b.select(None).n_rays == b.n_rays
    for bad in ([], [4], [-1], "all"):
        with pytest.raises(ValueError):
            b.select(bad)


def test_captured_draw_advances_with_a_device_step_word(bank):
    b, _ = bank
    B, seed = 1000, 11
    want = [[t.clone() for t in b.draw(s, B, seed, rank=0, world=1, return_indices=True)] for s in range(3)]
    out = (torch.zeros(B, 8, device=DEV), torch.zeros(B, 3, device=DEV), torch.zeros(B, device=DEV))
    word = torch.zeros(1, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # one warm-up off the capture
        b.draw(0, B, seed, rank=0, world=1, out=out, step_dev=word)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):          # a single stream: the draw, then the word's increment
        b.draw(0, B, seed, rank=0, world=1, out=out, step_dev=word)
        word.add_(1)
    for s in range(3):
        graph.replay()
        for got, ref in zip(out, want[s]):
            assert torch.equal(got, ref), s
    assert int(word) == 3
    # the host step and the word add up
    word.fill_(1)
    got = b.draw(1, B, seed, rank=0, world=1, step_dev=word, return_indices=True)
    assert torch.equal(got[3], want[2][3])


def test_draw_writes_into_the_training_steps_buffers(bank):
    """`GraphedTrainStep` allocates rays (B, 8), target (B, 3) and gt (B,) with torch.zeros(..., device=dev): such tensors are
    accepted as they are."""
    b, _ = bank
    B = 64
    rays, target, gt = torch.zeros(B, 8, device=DEV), torch.zeros(B, 3, device=DEV), torch.zeros(B, device=DEV)
    b.draw(0, B, 0, out=(rays, target, gt))          # rank and world from dist.world(): 0 of 1 here
    want = b.draw(0, B, 0, rank=0, world=1)
    assert torch.equal(rays, want[0]) and torch.equal(target, want[1]) and torch.equal(gt, want[2])


def test_refusals(bank):
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd.data import RayBank, _Bank
    b, (poses, images, masks, focal) = bank
    B = 16
    ok = lambda: [torch.zeros(B, 8, device=DEV), torch.zeros(B, 3, device=DEV), torch.zeros(B, device=DEV)]      # noqa: E731
    with pytest.raises(RuntimeError, match="GPU only"):
        b.gather(torch.arange(4))
    with pytest.raises(ValueError, match="int64"):
        b.gather(torch.arange(4, device=DEV, dtype=torch.int32))
    with pytest.raises(ValueError, match="1-D"):
        b.gather(torch.zeros(2, 2, dtype=torch.int64, device=DEV))
    for k, bad in ((0, torch.zeros(B, 8)), (1, torch.zeros(B, 3))):
        out = ok()
        out[k] = bad
        with pytest.raises(RuntimeError, match="GPU only"):
            b.draw(0, B, 0, out=out)
    for k, bad in ((0, torch.zeros(B, 8, dtype=torch.float64, device=DEV)), (0, torch.zeros(B, 6, device=DEV)),
                   (1, torch.zeros(B + 1, 3, device=DEV)), (2, torch.zeros(B, 1, device=DEV)), (0, torch.zeros(8, B, device=DEV).t())):
        out = ok()
        out[k] = bad
        with pytest.raises(ValueError, match="shape"):
            b.draw(0, B, 0, out=out)
    with pytest.raises(ValueError, match="shape"):
        b.draw(0, B + 1, 0, out=ok())          # out of another batch size
    with pytest.raises(ValueError, match="triple"):
        b.draw(0, B, 0, out=ok()[:2])
    with pytest.raises(ValueError, match="rank"):
        b.draw(0, B, 0, rank=1, world=1)
    with pytest.raises(ValueError, match="rank"):
        b.draw(0, B, 0, rank=2, world=2)
    with pytest.raises(ValueError):
        b.draw(-1, B, 0)
    with pytest.raises(RuntimeError):
        b.draw(0, B, 0, step_dev=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="int64"):
        b.draw(0, B, 0, step_dev=torch.zeros(1, dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError, match="uint8"):
        RayBank(poses, images.astype(np.float32), masks, focal, NEAR, FAR, DEV)
    with pytest.raises(ValueError, match="poses"):
        RayBank(poses[:2], images, masks, focal, NEAR, FAR, DEV)
    with pytest.raises(ValueError, match="masks"):
        RayBank(poses, images, masks[:, :-1], focal, NEAR, FAR, DEV)
    with pytest.raises(ValueError, match="3 or 4"):
        RayBank(poses, images[..., :2], masks, focal, NEAR, FAR, DEV)
    # N >= 2^32 through the C entry with null buffers: refused with a message, nothing allocated, nothing launched
    L = _lib.lib()
    big = _Bank(None, None, None, None, 65536, 256, 256, 4, 65536, 1.0, NEAR, FAR)
    assert L.mnrf_bank_draw(ctypes.byref(big), 0, 0, None, 0, 1, B, None, None, None, None, None, None) < 0
    assert b"2^32" in L.mnrf_last_error()
    # ... and the bank still works after the refusals
    assert not b.draw(0, B, 0)[0].isnan().any()


def test_train_blender_driver(tmp_path):
    """scripts/train_blender.py on a three-frame 8 x 8 dataset, two steps on the static route, as a fresh child process."""
    from tests.test_raybank_cpu import make_dataset
    root = tmp_path / "scene"
    root.mkdir()
    make_dataset(str(root), w=8, h=8, mixed=False)
    out = tmp_path / "weights.npz"
    r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, os.path.join(ROOT, "scripts", "train_blender.py"), "--root_dir", str(root),
                        "--img_wh", "8", "8", "--near", "0.05", "--far", "8", "--route", "static", "--steps", "2", "--batch", "64",
                        "--out", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    z = np.load(str(out))
    assert "coarse__sigma.weight" in z.files and "fine__sigma.weight" in z.files and "meta" in z.files
