"""The last reflection level of a frame renders colour and depth only (mnrf_field_composite_fused MNRF_FUSED_RGB_DEPTH): its
caller reads nothing else of it (eval.py:676-697), so the ray-fused fine pass stops its weight stream in front of the mirror head
(the folded stream puts it last, csrc/mnrf_layout.h) and composites rgb / depth / opacity alone.  Every map the caller reads must
stay what the full launch gives, bit for bit, and so must the whole frame."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARGS = dict(predict_normal=True, only_one_field=False, only_one_field_fine_epoch=2)


@pytest.fixture(autouse=True)
def split():
    from mirror_nerf_amd import mirror_nerf as MN
    old = MN.PRECISION
    MN.set_precision("split")
    yield
    MN.set_precision(old)


def _models(tweaks):
    from mirror_nerf_amd import synthetic as SY
    return SY.build_models(DEV, tweaks, seed=0)[0]


def _emb():
    import mirror_nerf_amd as M
    return {"xyz": M.Embedding(10), "dir": M.Embedding(4)}


def _rays(n, step=3):
    from oracle import mirror_nerf_oracle as O
    return torch.from_numpy(O.synthetic_rays(64, 64)[::step][:n].copy()).to(DEV)


def test_rgb_depth_variant_matches_the_full_fused_launch():
    """The two launches on the same rays and depths: rgb, depth, opacity, weights and x_surface equal bit for bit; ragged ray
    counts with more rays than CUs (the dynamic tile queue), one ray, and the refused map requests."""
    import mirror_nerf_amd as M
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd import synthetic as SY
    from mirror_nerf_amd.weights import folded_of
    L, p = _lib.lib(), _lib.ptr
    model = _models(SY.STRADDLE)["fine"]
    spr = L.mnrf_fused_samples_per_ray()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for n in (2 * cus + 7, 1):
        rays = _rays(n, 1)
        torch.manual_seed(n)
        z = torch.sort(2.0 + 4.0 * torch.rand(n, spr, device=DEV), dim=1).values.contiguous()
        de = M.Embedding(4)(rays[:, 3:6].contiguous()).contiguous()
        for white in (0, 1):
            outs = []
            for flags in (0, _lib.MNRF_FUSED_RGB_DEPTH):
                o = {"weights": torch.full((n, spr), -1.0, device=DEV), "opacity": torch.full((n,), -1.0, device=DEV),
                     "rgb": torch.full((n, 3), -1.0, device=DEV), "depth": torch.full((n,), -1.0, device=DEV),
                     "x_surface": torch.full((n, 3), -1.0, device=DEV)}
                full = flags == 0
                mask = torch.empty(n, device=DEV) if full else None
                sn = torch.empty(n, 3, device=DEV) if full else None
                _lib.check(L.mnrf_field_composite_fused(p(folded_of(model)), n, p(rays), p(z), p(de), 27, white | flags,
                                                        p(o["weights"]), p(o["opacity"]), p(o["rgb"]), p(o["depth"]), p(mask),
                                                        p(sn), p(o["x_surface"]), _lib.stream()), "mnrf_field_composite_fused")
                outs.append(o)
            torch.cuda.synchronize()
            for k in outs[0]:
                assert torch.equal(outs[0][k], outs[1][k]), (n, white, k)
            assert bool((outs[1]["opacity"] >= 0).all())
    # the variant evaluates neither the mirror head nor the normal map: asking for them is an error, not a silent zero
    buf = torch.empty(4, 3, device=DEV)
    for mask, sn in ((p(buf), None), (None, p(buf))):
        rc = L.mnrf_field_composite_fused(p(folded_of(model)), 1, p(rays), p(z), p(de), 27, _lib.MNRF_FUSED_RGB_DEPTH, None, None,
                                          p(buf), p(buf), mask, sn, None, _lib.stream())
        assert rc < 0 and b"MNRF_FUSED_RGB_DEPTH" in L.mnrf_last_error()
    assert L.mnrf_field_composite_fused(p(folded_of(model)), 1, p(rays), p(z), p(de), 27, 4, None, None, p(buf), p(buf), None, None,
                                        None, _lib.stream()) < 0


def _before(monkeypatch, maps_only):
    """The recursion as it was before the variant: the last level rendered with the caller's `_maps_only` and all four heads --
    the reference the routed frame is compared with."""
    from mirror_nerf_amd import recursion as R
    orig = R.render_rays

    def render(*a, **kw):
        if kw.pop("_rgb_depth_only", False):
            kw["_maps_only"] = maps_only
        return orig(*a, **kw)
    monkeypatch.setattr(R, "render_rays", render)


@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("maps_only", [False, True])
def test_frame_is_unchanged_by_the_rgb_depth_last_level(levels, maps_only, monkeypatch):
    """batched_inference, one and two bounces: the level-0 dict equal key for key (rgb_fine / depth_fine and the _reflect maps
    included) with and without the variant at the last level, whose fine launches are the variant's."""
    import mirror_nerf_amd as M
    from mirror_nerf_amd import mirror_nerf as MN
    from mirror_nerf_amd import synthetic as SY
    models = _models(SY.STRADDLE)
    rays = _rays(700)
    args = dict(ARGS, max_recursive_level=levels)

    def frame():
        return M.batched_inference(models, _emb(), rays, 64, 128, False, 300, args=args, trace_secondary_rays=True, to_cpu=False,
                                   maps_only=maps_only)
    MN.LAUNCH_LOG = []
    try:
        got = frame()
        torch.cuda.synchronize()
        fine = [flags for flags, _B, _e0, _e1 in MN.LAUNCH_LOG if not flags & 1]
    finally:
        MN.LAUNCH_LOG = None
    assert any(f & 0x4000 for f in fine), "no rgb / depth launch at the last level"
    assert not all(f & 0x4000 for f in fine), "the levels above the last one keep their launch"
    with monkeypatch.context() as mp:
        _before(mp, maps_only)
        want = frame()
    torch.cuda.synchronize()
    assert int((want["mirror_mask_fine"] != 0).sum()) > 0
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
