"""frames.val_panel (csrc/mnrf_frames.hip: panel_extrema_kernel, panel_write_kernel) against tests/val_panel_ref.py, the
numpy restatement of visualize_val_image(..., add_text=False) that tests/test_validation_cpu.py holds to the reference's own
capture.  Tolerance ZERO: every tile is the reference's chain of single fp32 operations.  Shapes: 6x8 (less than a wave of
4-pixel threads), 5x13 (65 pixels: one past 64, and no multiple of 4, so the tail and the unaligned rows run), 37x29 (1073
pixels: past one 256-thread workgroup of 4-pixel threads, a multiple of nothing)."""
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


@pytest.mark.parametrize("variant", VR.VARIANTS)
@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_val_panel_is_the_restatement_exactly(H, W, variant):
    from mirror_nerf_amd.frames import jet_table
    batch, res = VR.seeded_case(H, W, 100 + H, variant)
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
