"""The ray bank on the device (csrc/mnrf_bank.hip through mirror_nerf_amd.data.RayBank).

Everything is compared exactly: gathered rays against mnrf_generate_rays of the same pose (one shared device function, bit for
bit), colours and masks against the same float32 expressions in torch on the CPU (IEEE division, multiply, subtract, add; no
contraction on either side), drawn indices against the integer restatement tests/raybank_ref.py.  The one tolerance is fixture
G12's own 1e-6 on rays captured from the reference.  Shapes: odd, non-square frames (37 x 53, 5 x 7), N not a power of two,
batches that divide neither N nor the 256-thread block.  Those banks have 105 and 5883 rays (half = 4 and 7).  The 32-bit range of
the stream is reached with banks that select the two frames of a small base bank tens of thousands of times: N = 2^32 - 1 (the
largest accepted; half = 16, slots and `start` above 2^31), N = 2^31 (the domain is 2 N and `x >= N` a uint32 comparison with
0x80000000), N = 2^31 + 65536 (bit 31 set on both sides of it), and with plain banks of N = 65536 (N is the domain: no walk),
65537 (half = 9, the longest walks) and 1, 2, 3 (the bit count raised to 2).  Each asserts its N and its half."""
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


# ----------------------------------------------------------------------------- the 32-bit range of the shuffled stream
# Banks whose n_rays sits at the edges of the permutation's domain, made by selecting the frames of a small base bank again and
# again (a slot costs 4 bytes).  (id, base (F, H, W, C), selection, N, half):
EDGE_BANKS = [
    ("N=2^32-1", (2, 255, 257, 4), [0, 1] * 32768 + [1], 2 ** 32 - 1, 16),   # the largest N accepted: the domain 2^32 holds one value more
    ("N=2^31", (2, 256, 256, 4), [0, 1] * 16384, 2 ** 31, 16),               # N - 1 has 31 bits, the domain is 2^32 = 2 N: every other value
    #                                                                          walks, and the walk ends on a uint32 comparison with 0x80000000
    ("N=2^31+65536", (2, 256, 256, 4), [0, 1] * 16384 + [0], 2 ** 31 + 65536, 16),      # x >= N with bit 31 set on both sides
    ("N=65536", (1, 256, 256, 3), None, 65536, 8),                           # N is the Feistel domain: never walks
    ("N=65537", (1, 1, 65537, 3), None, 65537, 9),                           # one past it: the domain is 4 N - 4, long walks
    ("N=1", (1, 1, 1, 3), None, 1, 1),                                       # bits < 2 is raised to 2; every draw is ray 0
    ("N=2", (1, 1, 2, 3), None, 2, 1),
    ("N=3", (1, 1, 3, 3), None, 3, 1),
]
EDGE_B = 1000


def _edge_base(F, H, W, C, seed):
    from mirror_nerf_amd.data import RayBank
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 256, (F, H, W, C), dtype=np.uint8)
    masks = rng.integers(-1, 2, (F, H, W)).astype(np.int8)
    return RayBank(_poses(F, seed), images, masks, 0.5 * W / np.tan(0.5 * 0.6911112), NEAR, FAR, DEV)


@pytest.fixture(scope="module", params=EDGE_BANKS, ids=[e[0] for e in EDGE_BANKS])
def edge_bank(request):
    """(bank, base bank, every row of the base bank, N, whether the bank is a selection)"""
    _, shape, selection, N, half = request.param
    base = _edge_base(*shape, seed=len(selection or []) + shape[1])
    b = base if selection is None else base.select(selection)
    assert b.n_rays == N and R.half_bits(N) == half and N < 2 ** 32          # the reach of the case
    return b, base, base.gather(torch.arange(base.n_rays, device=DEV)), N, selection is not None


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.reshape(-1).view(torch.int32), b.reshape(-1).view(torch.int32))


def test_stream_at_the_edges_of_its_32_bit_range(edge_bank):
    """The drawn indices are the restatement's at step 0, at the step that straddles the end of epoch 0, several epochs on at a
    position above 2^32 (also reached through the device step word), at one above 2^34 and for rank 2 of 3; the drawn rows are the gather of those
    indices and, through the frame list, the base bank's pixels."""
    b, base, base_rows, N, selected = edge_bank
    B, hw = EDGE_B, b.H * b.W
    straddle, far, deep = N // B, (3 * N + 2 ** 32) // B + 7, 2 ** 34 // B + 1
    assert N % B != 0 and (straddle * B) // N == 0 and (straddle * B + B - 1) // N >= 1      # the batch crosses into epoch 1
    assert far * B > 2 ** 32 and (far * B) // N >= 3 and ((far * 3 + 2) * B) // N >= 3
    assert (deep * B) // N >= 4 and (N > 3 or (deep * B) // N >= 2 ** 32)       # small banks: the epoch has a high word
    word = torch.tensor([far - 5], dtype=torch.int64, device=DEV)
    ids = torch.tensor(b.frame_ids, dtype=torch.int64, device=DEV)
    for seed in (0, 2 ** 40 + 12345):
        draws = [(s, 0, 1, None) for s in (0, straddle, far, deep)] + [(5, 0, 1, word), (0, 2, 3, None), (far, 2, 3, None)]
        for step, rank, world, step_dev in draws:
            tag = (seed, step, rank, world, step_dev is not None)
            rays, rgbs, mask, idx = b.draw(step, B, seed, rank=rank, world=world, step_dev=step_dev, return_indices=True)
            want = R.draw_indices(N, far if step_dev is not None else step, B, seed, rank, world)
            assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), want), tag
            assert int(idx.min()) >= 0 and int(idx.max()) < N
            rows = (rays, rgbs, mask)
            assert not any(t.isnan().any() for t in rows), tag
            for got, ref in zip(rows, b.gather(idx)):
                assert _same_bits(got, ref), tag
            pixels = ids[idx // hw] * hw + idx % hw                          # slots past 2^31 are pixels of the base frames
            assert selected or torch.equal(pixels, idx)
            for got, ref in zip(rows, base_rows):
                assert _same_bits(got, ref[pixels]), tag
        if N == 2 ** 32 - 1:
            assert int(idx.max()) >= 2 ** 31                                 # half of the bank lies there: bit 31 is in use
    if N == 1:
        assert not idx.any()
    if selected:
        assert set(b.frame_ids) == {0, 1} and len(set((ids[idx // hw]).tolist())) == 2      # both base frames were drawn from


def test_last_slot_of_an_edge_bank_is_its_base_frame(edge_bank):
    """frame(last slot): the rows start + 0 ... start + hw - 1 with start = (slots - 1) hw, above 2^31 in the large banks."""
    b, base, _, N, _ = edge_bank
    last = b.n_frames - 1
    if N > 2 ** 31:
        assert last * b.H * b.W >= 2 ** 31
    got, want = b.frame(last), base.frame(b.frame_ids[last])
    assert set(got) == {"rays", "rgbs", "mirror_mask", "valid_mask"} and got["valid_mask"].dtype == torch.bool
    for k in got:
        assert (torch.equal(got[k], want[k]) if k == "valid_mask" else _same_bits(got[k], want[k])), k


def test_gather_addresses_the_whole_64_bit_index():
    """Explicit indices around 2^31 and 2^32 on the bank of 2^32 - 1 rays: the rows inside are the base bank's, N, 2^32 and -1
    give NaN.  One slot more makes N >= 2^32: a draw is refused, a gather above 2^32 still finds its pixel."""
    _, shape, selection, N, _ = EDGE_BANKS[0]
    base = _edge_base(*shape, seed=3)
    rows = base.gather(torch.arange(base.n_rays, device=DEV))
    hw = base.H * base.W

    def check(bank, indices, inside):
        got = bank.gather(torch.tensor(indices, dtype=torch.int64, device=DEV))
        for k, (g, ok) in enumerate(zip(indices, inside)):
            for t, ref in zip(got, rows):
                if ok:
                    assert _same_bits(t[k], ref[bank.frame_ids[g // hw] * hw + g % hw]), g
                else:
                    assert t[k].isnan().all(), g

    b = base.select(selection)
    assert b.n_rays == N == 2 ** 32 - 1
    check(b, [0, 2 ** 31 - 1, 2 ** 31, N - 1, N, 2 ** 32, -1], [True, True, True, True, False, False, False])
    more = base.select(selection + [0])
    assert more.n_rays == 65538 * hw >= 2 ** 32
    with pytest.raises(RuntimeError, match=r"below 2\^32"):
        more.draw(0, EDGE_B, 0, rank=0, world=1)
    check(more, [2 ** 32, 2 ** 32 + 12345, more.n_rays - 1, more.n_rays], [True, True, True, False])


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
