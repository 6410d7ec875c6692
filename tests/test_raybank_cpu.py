"""The ray bank without a GPU: the permutation of tests/raybank_ref.py (the integer restatement of csrc/mnrf_bank.hip's
contract) is a bijection, differs between epochs and seeds and lands uniformly, and equals a scalar implementation in plain Python integers
at the N where 32-bit arithmetic could slip (1, 2, 3, 65536, 65537, 2^31, 2^31 + 65536, 2^32 - 1: the banks
tests/test_hip_raybank.py holds the kernel to), at epoch boundaries and at positions above 2^32; `read_blender` reads a small Blender-format
directory built here with PIL; the C entry points refuse bad arguments before any launch."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import raybank_ref as R


@pytest.mark.parametrize("n", [1, 2, 3, 5, 105, 4097, 5883, 65537])
def test_perm_is_a_bijection(n):
    for epoch in range(3):
        g, walks = R.perm(np.arange(n), n, 7, epoch, return_walks=True)
        assert np.array_equal(np.sort(g), np.arange(n)), (n, epoch)
        assert walks <= 64          # expected below 4; 41 at the worst seen with these constants


def test_half_bits():
    assert [R.half_bits(n) for n in (1, 2, 3, 4, 5, 16, 17, 105, 65536, 65537, 2 ** 32 - 1)] == [1, 1, 1, 1, 2, 2, 3, 4, 8, 9, 16]
    for n in (1, 2, 3, 5, 105, 4097, 2 ** 31 + 1):
        assert n <= 4 ** R.half_bits(n) <= max(4, 4 * n - 1)      # the domain holds N and is under 4 N


def test_epochs_and_seeds_give_different_orders():
    n = 5883
    i = np.arange(n)
    a, b, c = R.perm(i, n, 7, 0), R.perm(i, n, 7, 1), R.perm(i, n, 8, 0)
    # two independent permutations agree at one position on average
    assert (a == b).sum() < 12 and (a == c).sum() < 12 and (b == c).sum() < 12
    hi = R.perm(i, n, 7, 2 ** 32)           # the high word of the epoch is part of the key
    assert (a == hi).sum() < 12
    assert (R.perm(i, n, 7 + 2 ** 32, 0) == a).sum() < 12


def test_stream_crosses_epochs_inside_a_batch():
    n, B = 105, 16
    got = np.concatenate([R.draw_indices(n, s, B, 3) for s in range(14)])       # 224 positions: two epochs and a bit
    for e in range(2):
        assert np.array_equal(np.sort(got[e * n:(e + 1) * n]), np.arange(n))
    assert np.array_equal(got[:n], R.perm(np.arange(n), n, 3, 0)) and np.array_equal(got[n:2 * n], R.perm(np.arange(n), n, 3, 1))
    # ranks interleave: the batches of ranks 0 and 1 at step s are the two halves of the world-1 batch of 2B
    for s in range(5):
        both = np.concatenate([R.draw_indices(n, s, B, 3, rank=r, world=2) for r in range(2)])
        assert np.array_equal(both, R.draw_indices(n, s, 2 * B, 3))


def test_landing_counts_are_uniform():
    """N = 105, stream positions 0-15, 4000 epochs: chi^2 / dof of the landing counts over the 105 bins below 1.5 (104 degrees of
    freedom: standard deviation 0.14, so 1.5 is 3.6 sigma).  Seen: 0.82 with the contract's 6 rounds, 0.88 with 4, 58 with 2."""
    n, epochs = 105, 4000
    i, e = np.meshgrid(np.arange(16), np.arange(epochs))

    def chi2(rounds):
        counts = np.bincount(R.perm(i, n, 7, e, rounds=rounds).reshape(-1), minlength=n)
        expect = 16 * epochs / n
        return float(((counts - expect) ** 2 / expect).sum() / (n - 1))

    assert chi2(R.ROUNDS) < 1.5
    assert chi2(2) > 10          # the check sees a weak network


# --------------------------------------------------------------------------- the restatement against plain Python integers
def _mix32(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def _scalar_stream(p, n, seed):
    """One stream position in Python integers, from the contract in the header comment of csrc/mnrf_bank.hip: nothing is shared
    with tests/raybank_ref.py and nothing depends on how numpy's uint64 wraps, shifts or divides."""
    epoch, i = divmod(p, n)
    half = (max(2, (n - 1).bit_length()) + 1) // 2
    mask = (1 << half) - 1
    keys = []
    for r in range(6):
        k = _mix32(((seed & 0xFFFFFFFF) + 0x9E3779B9 * (r + 1)) & 0xFFFFFFFF)
        k = _mix32(k ^ ((seed >> 32) & 0xFFFFFFFF))
        keys.append(_mix32(_mix32(k ^ (epoch & 0xFFFFFFFF)) ^ ((epoch >> 32) & 0xFFFFFFFF)))
    x, passes = i, 0
    while True:
        L, R_ = x >> half, x & mask
        for k in keys:
            L, R_ = R_, L ^ (_mix32(R_ ^ k) & mask)
        x, passes = (L << half) | R_, passes + 1
        assert x < 4 ** half and passes <= 64
        if x < n:
            return x


@pytest.mark.parametrize("n", [1, 2, 3, 65536, 65537, 2 ** 31, 2 ** 31 + 65536, 2 ** 32 - 1])
def test_stream_equals_plain_python_integers_at_the_edges_of_its_range(n):
    """The N of tests/test_hip_raybank.py's edge banks: 40 positions at each of the start, the end of epoch 0 (both sides), an
    epoch boundary above 2^32, a position whose epoch has a high word (small n) and the top of a 60-bit step count."""
    over = -(-(2 ** 32 + 12345) // n) * n                         # the first epoch boundary above 2^32 + 12345
    starts = [0, max(n - 20, 0), over - 20, 7 * over + n // 3, (2 ** 60 // n) * n - 20]
    p = sorted({s + k for s in starts for k in range(40)})
    assert len(p) >= 100 and any(a // n != b // n for a, b in zip(p, p[1:])) and p[-1] > 2 ** 32 and p[-1] < 2 ** 64
    assert any(a > 2 ** 32 and a // n != (a + 1) // n for a in p[:-1])      # an epoch boundary above 2^32
    for seed in (0, 2 ** 40 + 12345, 2 ** 64 - 1):
        got = R.stream(np.array(p, np.uint64), n, seed)
        want = [_scalar_stream(q, n, seed) for q in p]
        assert got.dtype == np.int64 and got.tolist() == want, (n, seed)
        assert 0 <= min(want) and max(want) < n
    if n >= 2 ** 31:
        assert max(want) >= 2 ** 30


# --------------------------------------------------------------------------- the loader
def make_dataset(root, w=8, h=6, n=3, mixed=True, seed=0):
    """A Blender-format directory of n frames: frame 0 RGBA with an 8-bit mask, frame 1 RGB (RGBA when not `mixed`) with a 16-bit
    mask, frame 2 RGBA without a mask file.  Returns what read_blender has to give back."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "train"))
    os.makedirs(os.path.join(root, "masks"))
    frames, images, masks, poses = [], [], [], []
    for k in range(n):
        rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        rgba[0, :4, 3] = (0, 255, 1, 254)
        opaque = mixed and k == 1
        Image.fromarray(rgba[..., :3] if opaque else rgba).save(os.path.join(root, "train", f"Image_{k:04d}.png"))
        if opaque:
            rgba[..., 3] = 255
        images.append(rgba)
        if k % 3 == 0:
            m8 = rng.integers(0, 256, (h, w), dtype=np.uint8)
            m8[0, :4] = (0, 127, 128, 255)
            Image.fromarray(m8).save(os.path.join(root, "masks", f"MirrorMask_{k:04d}.png"))
            masks.append((m8 >= 128).astype(np.int8))
        elif k % 3 == 1:
            m16 = (rng.integers(0, 2, (h, w)) * rng.integers(1, 65536, (h, w))).astype(np.uint16)
            m16[0, :3] = (0, 1, 65535)
            Image.fromarray(m16).save(os.path.join(root, "masks", f"MirrorMask_{k:04d}.png"))
            masks.append((m16 > 0).astype(np.int8))
        else:
            masks.append(np.full((h, w), -1, np.int8))
        pose = np.eye(4)
        pose[:3, :4] = rng.normal(size=(3, 4))
        poses.append(pose)
        frames.append({"file_path": f"./train/Image_{k:04d}", "transform_matrix": pose.tolist()})
    for split in ("train", "test"):
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": 0.6911112, "frames": frames}, f)
    return dict(images=np.stack(images), masks=np.stack(masks), poses=np.stack(poses)[:, :3, :4].astype(np.float32))


def test_read_blender(tmp_path):
    from mirror_nerf_amd.data import read_blender
    want = make_dataset(str(tmp_path))
    d = read_blender(str(tmp_path), "train", (8, 6), 0.05, 8.0)
    assert d["images"].dtype == np.uint8 and d["images"].shape == (3, 6, 8, 4)
    assert np.array_equal(d["images"], want["images"])          # same size: LANCZOS is the identity; the RGB frame got alpha 255
    assert d["masks"].dtype == np.int8 and np.array_equal(d["masks"], want["masks"])
    assert (d["masks"][2] == -1).all() and set(np.unique(d["masks"][:2])) == {0, 1}
    assert d["poses"].dtype == np.float32 and np.array_equal(d["poses"], want["poses"])
    assert d["focal"] == 0.5 * 800 / np.tan(0.5 * 0.6911112) * (8 / 800)
    assert (d["near"], d["far"]) == (0.05, 8.0)
    # every second frame of the train split; every frame of another split
    d2 = read_blender(str(tmp_path), "train", (8, 6), 0.05, 8.0, train_skip_step=2)
    assert np.array_equal(d2["images"], want["images"][[0, 2]]) and np.array_equal(d2["poses"], want["poses"][[0, 2]])
    assert read_blender(str(tmp_path), "test", (8, 6), 0.05, 8.0, train_skip_step=2)["images"].shape[0] == 3
    # resizing: LANCZOS for the image (PIL's own), cv2's nearest rule floor(x * src / dst) for the mask
    from PIL import Image
    d3 = read_blender(str(tmp_path), "train", (4, 3), 0.05, 8.0)
    assert d3["images"].shape == (3, 3, 4, 4) and d3["focal"] == 0.5 * 800 / np.tan(0.5 * 0.6911112) * (4 / 800)
    assert np.array_equal(d3["images"][0], np.asarray(Image.fromarray(want["images"][0]).resize((4, 3), Image.LANCZOS)))
    assert np.array_equal(d3["masks"], want["masks"][:, ::2, ::2])


def test_read_blender_keeps_three_channels(tmp_path):
    from mirror_nerf_amd.data import read_blender
    from PIL import Image
    make_dataset(str(tmp_path))
    for k in range(3):
        p = os.path.join(str(tmp_path), "train", f"Image_{k:04d}.png")
        Image.open(p).convert("RGB").save(p)
    assert read_blender(str(tmp_path), "train", (8, 6), 0.05, 8.0)["images"].shape == (3, 6, 8, 3)


def test_with_mask_selection(tmp_path):
    """What select("with_mask") selects: the frames without a -1 (blender.py:91-95)."""
    from mirror_nerf_amd.data import frames_with_mask, read_blender
    make_dataset(str(tmp_path), n=5)
    d = read_blender(str(tmp_path), "train", (8, 6), 0.05, 8.0)
    assert frames_with_mask(d["masks"]) == [0, 1, 3, 4]
    m = d["masks"].copy()
    m[3, 5, 7] = -1                      # one invalid pixel takes the frame out
    assert frames_with_mask(m) == [0, 1, 4]


def test_bank_needs_a_gpu_device():
    from mirror_nerf_amd.data import RayBank
    with pytest.raises(RuntimeError, match="GPU only"):
        RayBank(np.zeros((1, 3, 4), np.float32), np.zeros((1, 2, 2, 3), np.uint8), None, 1.0, 0.1, 1.0, "cpu")


# --------------------------------------------------------------------------- the C entry points, no launch
def _bank(n_frames=3, H=5, W=7, C=4, slots=None, fake=0):
    from mirror_nerf_amd.data import _Bank
    p = ctypes.c_void_p(fake) if fake else None
    return _Bank(p, p, p, None, n_frames, H, W, C, n_frames if slots is None else slots, 1.0, 0.1, 1.0)


def test_entry_points_validate_before_any_launch():
    from mirror_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    null = None
    draw = lambda b, step=0, rank=0, world=1, batch=16: L.mnrf_bank_draw(                                     # noqa: E731
        ctypes.byref(b) if b is not None else None, 1, step, null, rank, world, batch, null, null, null, null, null, null)
    gather = lambda b, start=0, n=16: L.mnrf_bank_gather(ctypes.byref(b) if b is not None else None, null, start, n,   # noqa: E731
                                                           null, null, null, null, null)
    assert draw(None) < 0 and b"null bank" in L.mnrf_last_error()
    assert gather(None) < 0 and b"null bank" in L.mnrf_last_error()
    for bad in (_bank(C=2), _bank(C=5), _bank(H=0), _bank(W=-1), _bank(n_frames=0), _bank(slots=2)):
        assert draw(bad) < 0 and b"shape" in L.mnrf_last_error()
        assert gather(bad) < 0 and b"shape" in L.mnrf_last_error()
    # N >= 2^32 is refused by the draw: null buffers, nothing allocated
    assert draw(_bank(n_frames=65536, H=256, W=256)) < 0 and b"2^32" in L.mnrf_last_error()
    assert draw(_bank(n_frames=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1)) < 0
    ok = _bank(n_frames=65535, H=256, W=256, fake=256)          # N = 2^32 - 2^16: accepted as a size
    assert draw(ok, batch=0) == 0                              # zero rows: a no-op
    assert draw(ok, rank=1, world=1) < 0 and b"rank" in L.mnrf_last_error()
    assert draw(ok, rank=-1, world=2) < 0 and draw(ok, world=0) < 0
    assert draw(ok, step=-1) < 0 and b"step" in L.mnrf_last_error()
    assert draw(ok, batch=-1) < 0
    assert draw(_bank(), batch=16) < 0 and b"null bank array" in L.mnrf_last_error()
    # gather: zero rows are a no-op, a range outside the bank is refused
    assert gather(_bank(), n=0) == 0
    assert gather(_bank(), start=3 * 35 - 15, n=16) < 0 and b"leaves the bank" in L.mnrf_last_error()
    assert gather(_bank(), start=-1, n=1) < 0 and gather(_bank(), n=-1) < 0
    assert gather(_bank(), n=16) < 0 and b"null bank array" in L.mnrf_last_error()
