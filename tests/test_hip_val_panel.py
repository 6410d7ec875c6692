"""frames.val_panel (csrc/mnrf_frames.hip: panel_extrema_kernel, panel_write_kernel) against tests/val_panel_ref.py, the
numpy restatement of visualize_val_image(..., add_text=False) that tests/test_validation_cpu.py holds to the reference's own
capture.  Tolerance ZERO: every tile is the reference's chain of single fp32 operations.  Shapes: 6x8 (less than a wave of
4-pixel threads), 5x13 (65 pixels: one past 64, and no multiple of 4, so the tail and the unaligned rows run), 37x29 (1073
pixels: past one 256-thread workgroup of 4-pixel threads, a multiple of nothing).  Those need 4 blocks at the most.  Past the
grid caps: 283x311 (3 n / 1024 = 258 blocks wanted, panel_extrema_kernel has 256: it strides, and the last ticket is taken
under a capped grid) and 1031x1019 (n / 1024 = 1026 blocks wanted, panel_write_kernel has 1024: it strides; n = 1 mod 4).  Both
tests assert that reach from H and W."""
import json
import os

import numpy as np
import pytest
import torch

from tests import val_panel_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(6, 8), (5, 13), (37, 29)]
VAL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "validation")


def _dev(d):
    return {k: torch.from_numpy(v.copy()).to(DEV) for k, v in d.items()}


def _run(H, W, batch, res):
    import mirror_nerf_amd as M
    tb, tr = _dev(batch), _dev(res)
    stack, names = M.val_panel((W, H), tb, tr)
    torch.cuda.synchronize()
    for src, dst in ((batch, tb), (res, tr)):              # the maps are read in place and left bit for bit as they were
        for k, v in src.items():
            assert np.array_equal(dst[k].cpu().numpy().view(np.uint32), v.view(np.uint32)), k
    return stack, names


EXTREMA_CAP, WRITE_CAP = 256, 1024          # the grid caps of panel_extrema_kernel and panel_write_kernel


def _blocks(items):
    """Blocks of 256 threads x 4 items that a loop's first sweep would need."""
    return -(-items // 1024)


@pytest.mark.parametrize("variant", VR.VARIANTS)
@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_val_panel_is_the_restatement_exactly(H, W, variant):
    _check_panel(H, W, variant, *VR.seeded_case(H, W, 100 + H, variant))


@pytest.mark.parametrize("variant", ["all", "nan_global", "depth_extremes_last"])
def test_val_panel_past_the_extrema_cap(variant):
    """283 x 311: the launch is sized for 3 n values at 4 per thread and wants 258 blocks; panel_extrema_kernel has 256 and
    strides.  Its 65536 threads take one value per sweep, so a global tile is swept five times and a depth tile (n = 88013
    values) twice, and the last-ticket reduction runs under the capped grid.  The NaN of nan_global sits in the last pixel and
    the extremes of depth_extremes_last in the last element: both are seen in the last sweep only."""
    H, W = 283, 311
    assert _blocks(3 * H * W) > EXTREMA_CAP and H * W - 1 >= EXTREMA_CAP * 256
    _check_panel(H, W, variant, *VR.seeded_case(H, W, 100 + H, variant))


def test_val_panel_past_the_write_cap():
    """1031 x 1019: n / 1024 = 1026 blocks wanted, panel_write_kernel has 1024 and strides (and n = 1 mod 4: the tail runs
    there).  A reduced set of maps, still with a tile of each kind."""
    from mirror_nerf_amd import _lib, frames
    H, W = 1031, 1019
    assert _blocks(H * W) > WRITE_CAP and (H * W) % 4 != 0
    batch, res = VR.seeded_case(H, W, 100 + H, "all")
    res = {k: res[k] for k in ("rgb_fine", "depth_fine", "depth_coarse_reflect", "surface_normal_fine", "x_surface_fine")}
    kinds = [kind for _, kind, _ in frames.val_panel_tiles(batch, res)]
    assert set(kinds) == {_lib.MNRF_PANEL_COPY, _lib.MNRF_PANEL_MASK, _lib.MNRF_PANEL_NORMAL, _lib.MNRF_PANEL_GLOBAL,
                          _lib.MNRF_PANEL_DEPTH} and len(kinds) == 7
    _check_panel(H, W, "all", batch, res)


def _check_panel(H, W, variant, batch, res):
    from mirror_nerf_amd.frames import jet_table
    want, want_names = VR.val_panel((W, H), batch, res, jet_table())
    stack, names = _run(H, W, batch, res)
    assert names == want_names
    assert stack.dtype == torch.float32 and tuple(stack.shape) == want.shape and stack.is_contiguous()
    got = stack.cpu().numpy()
    for i, name in enumerate(names):
        assert np.array_equal(got[i], want[i], equal_nan=True), \
            (name, variant, float(np.nanmax(np.abs(got[i].astype(np.float64) - want[i]))), int((got[i] != want[i]).sum()))
    if variant == "nan_global":
        assert np.isnan(got[names.index("secondary_rays_o_vis")]).all() and np.isnan(got[names.index("x_surface_fine")]).all()
        assert not np.isnan(got[names.index("x_surface_coarse")]).any()
    if variant == "const_global":
        assert (got[names.index("reflect_direction_vis")] == 1).all() and (got[names.index("x_surface_coarse")] == 1).all()
    if variant == "nan_depth":
        assert not np.isnan(got[names.index("depth_fine")]).any()


def test_val_panel_reproduces_the_reference_capture():
    z = np.load(os.path.join(VAL, "val_panel_6x8.npz"))
    meta = json.loads(str(z["meta"]))
    batch = {k[7:]: z[k] for k in z.files if k.startswith("batch__")}
    res = {k[4:]: z[k] for k in z.files if k.startswith("in__")}
    stack, names = _run(meta["H"], meta["W"], batch, res)
    assert names == meta["names"]
    assert np.array_equal(stack.cpu().numpy(), z["out__stack"], equal_nan=True)


def test_val_panel_takes_the_shapes_a_frame_arrives_in():
    """The reference squeezes the masks and views the rest: (1, n, 3) colours, an (n, 1) mask, a non-contiguous map and a
    map at an address that is no multiple of 16 give the same panel; without the ground-truth mask its tile is absent."""
    from mirror_nerf_amd.frames import jet_table
    import mirror_nerf_amd as M
    H, W = 5, 13
    batch, res = VR.seeded_case(H, W, 9)
    want, names = VR.val_panel((W, H), batch, res, jet_table())
    tb, tr = _dev(batch), _dev(res)
    tb["rgbs"], tb["mirror_mask"] = tb["rgbs"][None], tb["mirror_mask"][:, None]
    tr["rgb_fine"] = torch.cat([tr["rgb_fine"], tr["rgb_fine"]], 1)[:, :3]              # row stride 6
    odd = torch.empty(H * W + 1, device=DEV)
    odd[1:] = tr["depth_coarse"]
    tr["depth_coarse"] = odd[1:]                                                        # 4 bytes past an aligned address
    odd3 = torch.empty(3 * H * W + 1, device=DEV)
    odd3[1:] = tr["x_surface_fine"].reshape(-1)
    tr["x_surface_fine"] = odd3[1:].view(H * W, 3)
    stack, got_names = M.val_panel((W, H), tb, tr)
    assert got_names == names and np.array_equal(stack.cpu().numpy(), want, equal_nan=True)
    del tb["mirror_mask"]
    stack, got_names = M.val_panel((W, H), tb, tr)
    keep = [i for i, n in enumerate(names) if n != "gt_mirror_mask"]
    assert got_names == [names[i] for i in keep] and np.array_equal(stack.cpu().numpy(), want[keep], equal_nan=True)
    with pytest.raises(ValueError, match="shape"):
        M.val_panel((W + 1, H), tb, tr)
