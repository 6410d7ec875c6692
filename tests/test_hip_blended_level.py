"""A level that traces has its colour blended with the thresholded mirror mask, m * reflected + (1 - m) * colour, m = 1 where the
composited mirror value is not below 0.5.  The blended-level launch (mnrf_field_composite_fused MNRF_FUSED_BLENDED_LEVEL) leaves
out the colour branch of such a ray and writes 0 to its rgb row.  Every other map, the rgb rows of the rays below 0.5 and the
whole frame must stay what they were, bit for bit."""
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


MAPS = ("weights", "opacity", "depth", "mirror_mask", "surf_normal", "x_surface")


def _launch(model, rays, z, de, flags, pn=True, old_entry=False):
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd.weights import folded_of
    L, p = _lib.lib(), _lib.ptr
    n, spr = z.shape
    o = {"weights": torch.full((n, spr), -1.0, device=DEV), "opacity": torch.full((n,), -1.0, device=DEV),
         "rgb": torch.full((n, 3), -1.0, device=DEV), "depth": torch.full((n,), -1.0, device=DEV),
         "mirror_mask": torch.full((n,), -1.0, device=DEV), "surf_normal": torch.full((n, 3), -1.0, device=DEV),
         "x_surface": torch.full((n, 3), -1.0, device=DEV)}
    if pn:
        o["pred_normal"] = torch.full((n, spr, 3), -1.0, device=DEV)
    head = (p(folded_of(model)), n, p(rays), p(z), p(de), 27, flags, p(o["weights"]), p(o["opacity"]), p(o["rgb"]), p(o["depth"]),
            p(o["mirror_mask"]), p(o["surf_normal"]), p(o["x_surface"]))
    if old_entry:
        _lib.check(L.mnrf_field_composite_fused(*head, _lib.stream()), "mnrf_field_composite_fused")
    else:
        _lib.check(L.mnrf_field_composite_fused_pn(*head, p(o.get("pred_normal")), _lib.stream()), "mnrf_field_composite_fused_pn")
    return o


def test_blended_launch_skips_exactly_the_rays_the_blend_discards():
    """The launch with and without the flag on the same rays and depths: ragged ray counts with more rays than CUs (the dynamic
    tile queue) and one ray, both backgrounds.  The launch of the old entry point (the full ray-fused kernel) and the per-sample
    normals of the two-kernel path are the references of the unflagged launch."""
    import mirror_nerf_amd as M
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd import mirror_nerf as MN
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
        two = MN.field_forward(model, n * spr, rays=rays, z_vals=z, spr=spr, dir_emb=de, dir_stride=27)
        for white in (0, 1):
            full = _launch(model, rays, z, de, white, pn=False, old_entry=True)
            plain = _launch(model, rays, z, de, white)
            got = _launch(model, rays, z, de, white | _lib.MNRF_FUSED_BLENDED_LEVEL)
            old = _launch(model, rays, z, de, white | _lib.MNRF_FUSED_BLENDED_LEVEL, pn=False, old_entry=True)
            torch.cuda.synchronize()
            for k in MAPS + ("rgb",):      # the flag through the entry point without the pred_normal argument
                assert torch.equal(old[k], got[k]), (n, white, k)
            for k in MAPS + ("rgb",):
                assert torch.equal(plain[k], full[k]), (n, white, k)
            assert torch.equal(plain["pred_normal"].view(-1, 3), two["pred_normal"].view(-1, 3)), (n, white)
            for k in MAPS + ("pred_normal",):
                assert torch.equal(got[k], plain[k]), (n, white, k)
            below = plain["mirror_mask"] < 0.5
            assert torch.equal(got["rgb"][below], plain["rgb"][below]), (n, white)
            assert bool((got["rgb"][~below] == 0).all()), (n, white)
            assert float((plain["mirror_mask"] - 0.5).abs().min()) > 1e-4      # (no ray on the fence: the rows above are the claim)
            if n > 1:
                assert 0 < int(below.sum()) < n, "both kinds of ray in one launch"
                assert bool((plain["rgb"][~below] != 0).any())
    # the flag decides from the mirror head: refused with the variant that has none, and without the mask the caller blends with
    buf = torch.empty(4, 3, device=DEV)
    both = _lib.MNRF_FUSED_BLENDED_LEVEL | _lib.MNRF_FUSED_RGB_DEPTH
    for fn, tail in ((L.mnrf_field_composite_fused, ()), (L.mnrf_field_composite_fused_pn, (None,))):
        rc = fn(p(folded_of(model)), 1, p(rays), p(z), p(de), 27, both, None, None, p(buf), p(buf), None, None, None, *tail,
                _lib.stream())
        assert rc < 0 and b"MNRF_FUSED_BLENDED_LEVEL" in L.mnrf_last_error()
        rc = fn(p(folded_of(model)), 1, p(rays), p(z), p(de), 27, _lib.MNRF_FUSED_BLENDED_LEVEL, None, None, p(buf), p(buf), None,
                p(buf), None, *tail, _lib.stream())
        assert rc < 0 and b"MNRF_FUSED_BLENDED_LEVEL" in L.mnrf_last_error()
    rc = L.mnrf_field_composite_fused_pn(p(folded_of(model)), 1, p(rays), p(z), p(de), 27, _lib.MNRF_FUSED_RGB_DEPTH, None, None,
                                         p(buf), p(buf), None, None, None, p(buf), _lib.stream())
    assert rc < 0 and b"MNRF_FUSED_RGB_DEPTH" in L.mnrf_last_error()


def _before(monkeypatch):
    """The recursion as it was before the blended-level launch: every level rendered without `_blended_level`."""
    from mirror_nerf_amd import recursion as R
    orig = R.render_rays

    def render(*a, **kw):
        kw.pop("_blended_level", None)
        return orig(*a, **kw)
    monkeypatch.setattr(R, "render_rays", render)


def _frame(models, rays, chunk, maps_only, args=None, blended_level=True, **kw):
    """(blended_level=True: the launch is forced wherever it may be used -- what is compared is the result; the choice per chunk
    has its own test)"""
    import mirror_nerf_amd as M
    return M.batched_inference(models, _emb(), rays, 64, 128, False, chunk, args=args or dict(ARGS, max_recursive_level=1),
                               trace_secondary_rays=True, to_cpu=False, maps_only=maps_only, blended_level=blended_level, **kw)


def _fine_launches(run):
    from mirror_nerf_amd import mirror_nerf as MN
    MN.LAUNCH_LOG = []
    try:
        out = run()
        torch.cuda.synchronize()
        return out, [flags for flags, _B, _e0, _e1 in MN.LAUNCH_LOG if not flags & 1]
    finally:
        MN.LAUNCH_LOG = None


@pytest.mark.parametrize("maps_only", [False, True])
@pytest.mark.parametrize("which", ["straddle", "all_mirror"])
def test_frame_is_unchanged_by_the_blended_level_launch(which, maps_only, monkeypatch):
    """batched_inference, one bounce, a ragged last chunk: the result dict equal key for key (rgb_fine, rgb_fine_reflect,
    weights_fine and pred_normal_fine included) with the routing of before; level 0 takes the new launch, the last level not."""
    from mirror_nerf_amd import synthetic as SY
    models = _models(SY.STRADDLE if which == "straddle" else SY.ALL_MIRROR)
    rays, chunk = (_rays(4096, 1), 1500) if which == "straddle" else (_rays(300), 300)
    got, fine = _fine_launches(lambda: _frame(models, rays, chunk, maps_only))
    n_chunks = -(-rays.shape[0] // chunk)
    assert sum(bool(f & 0x8000) for f in fine) == n_chunks, "level 0 takes the blended-level launch"
    assert not any(f & 0x8000 and f & 0x4000 for f in fine) and any(f & 0x4000 for f in fine), "the last level keeps its launch"
    with monkeypatch.context() as mp:
        _before(mp)
        want, fine0 = _fine_launches(lambda: _frame(models, rays, chunk, maps_only))
    assert not any(f & 0x8000 for f in fine0)
    assert int((want["mirror_mask_fine"] != 0).sum()) > 0
    if not maps_only:
        assert "weights_fine" in want and "pred_normal_fine" in want
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_two_bounces_take_the_launch_at_both_tracing_levels(monkeypatch):
    """max_recursive_level = 2: level 0 and level 1 (compacted reflected rays) both trace and blend, level 2 is the rgb / depth
    launch; the frame is equal key for key with the routing of before."""
    from mirror_nerf_amd import synthetic as SY
    models = _models(SY.STRADDLE)
    rays = _rays(700)
    args = dict(ARGS, max_recursive_level=2)
    got, fine = _fine_launches(lambda: _frame(models, rays, 300, False, args=args))
    assert sum(bool(f & 0x8000) for f in fine) > 3, "three chunks at level 0 and their reflections at level 1"
    assert any(f & 0x4000 for f in fine)
    with monkeypatch.context() as mp:
        _before(mp)
        want, fine0 = _fine_launches(lambda: _frame(models, rays, 300, False, args=args))
    assert not any(f & 0x8000 for f in fine0)
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_route_is_chosen_per_chunk_from_the_share_of_mirror_rays_last_counted():
    """blended_level="auto" (the default): no evidence for a model -> the launches of before; every ray a mirror -> the chunks
    behind the first counted one take the new launch, and so does the whole next frame; no ray a mirror -> never."""
    import mirror_nerf_amd as M
    from mirror_nerf_amd import recursion as R
    from mirror_nerf_amd import synthetic as SY
    rays = _rays(900, 1)
    for tweaks, expect in ((SY.ALL_MIRROR, True), (SY.OPAQUE, False)):
        models = _models(tweaks)
        assert models["fine"] not in R._MIRROR_FRACTION
        frames = []
        for _ in range(2):
            _out, fine = _fine_launches(lambda: M.batched_inference(models, _emb(), rays, 64, 128, False, 300,
                                                                    args=dict(ARGS, max_recursive_level=1),
                                                                    trace_secondary_rays=True, to_cpu=False))
            frames.append([bool(f & 0x8000) for f in fine if not f & 0x4000])      # the level-0 fine launches, in order
        assert len(frames[0]) == 3 and not frames[0][0], "nothing counted yet: the first chunk keeps its launch"
        share = R._MIRROR_FRACTION[models["fine"]][0]
        if expect:
            assert share == 1.0 and frames[0][2] and all(frames[1]), frames
        else:
            assert share == 0.0 and not any(frames[0] + frames[1]), frames


def test_blended_level_launch_is_not_used_where_more_of_the_level_is_read():
    """A placed mirror edits the mask behind the threshold and roughness jitters add further renders: those frames keep the
    launches of before."""
    from mirror_nerf_amd import synthetic as SY
    models = _models(SY.STRADDLE)
    rays = _rays(200)
    base = dict(ARGS, max_recursive_level=1)
    plane = dict(axis="x", position=0.3, normal=(1.0, 0.0, 0.0), rect=(-0.2, 0.2, -0.2, 0.2))
    for args, kw in ((dict(base, app_place_new_mirror=True, near=2.0), dict(new_mirror=plane)),
                     (dict(base, app_control_mirror_roughness=True, trace_ray_times=1), dict(normal_noise_std=0.01))):
        from types import SimpleNamespace
        _out, fine = _fine_launches(lambda: _frame(models, rays, 200, False, args=SimpleNamespace(**args), **kw))
        assert fine and not any(f & 0x8000 for f in fine), args
    _out, fine = _fine_launches(lambda: _frame(models, rays, 200, False, blended_level=False))      # the caller's opt-out
    assert fine and not any(f & 0x8000 for f in fine)
    _out, fine = _fine_launches(lambda: _frame(models, rays, 200, False))
    assert any(f & 0x8000 for f in fine)


# positions of the parts in the folded stream as they were before the mirror head's copy (in 2 KiB pairs), and where each part
# that is not folded comes from in the split stream: restated here, not read from the code under test
FOLD_PARTS = {"trunk": (0, 960, 0), "view": (1032, 8, 1296), "rgb": (1040, 4, 1304), "is_mirror_net.0": (1044, 64, 1036),
              "is_mirror_net.2": (1108, 4, 1100)}
F32_FLOATS = 2640 * 256 + 3072 + 1920 * 256 + 704 * 256
SPLIT_FWD, FOLD_FWD = F32_FLOATS, F32_FLOATS + (1312 + 960 + 352) * 512
MIRB, FOLD_BIAS = 1160, 1120 + 32


def test_fold_packer_keeps_every_part_in_place_and_adds_the_mirror_copy():
    """After mnrf_fold_weights_n every part of the folded stream holds, at the position it had before, the tiles it had before
    (the copied parts: those of the split stream); the bias block behind the stream's tail is intact; the copy of the mirror
    head for the blended-level launch follows it on a chunk boundary: is_mirror_net.0, is_mirror_net.2, four pairs of zeros."""
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd import synthetic as SY
    from mirror_nerf_amd.weights import folded_of
    model = _models(SY.STRADDLE)["fine"]
    img = folded_of(model)
    torch.cuda.synchronize()
    assert img.numel() == _lib.lib().mnrf_packed_floats() == F32_FLOATS + (1312 + 960 + 352 + 1328) * 512 + 16384
    words = img.view(torch.int32)
    pairs = lambda off, first, n: words[off + first * 512: off + (first + n) * 512]  # noqa: E731
    for name, (pos, n, src) in FOLD_PARTS.items():
        assert torch.equal(pairs(FOLD_FWD, pos, n), pairs(SPLIT_FWD, src, n)), name
        assert int((pairs(FOLD_FWD, pos, n) != 0).sum()) > 0, name
    # sigma row of the sigma | normal block: rows 16 nb + (lane & 15), row 0 = lanes 0, 16, 32, 48 of each tile
    sig_new = pairs(FOLD_FWD, 960, 8).view(16, 64, 4)[:, ::16]
    assert torch.equal(sig_new, pairs(SPLIT_FWD, 960, 8).view(16, 64, 4)[:, ::16])
    assert int((pairs(FOLD_FWD, 968, 64) != 0).sum()) > 0      # dir_encoding (folded) where it was
    assert torch.equal(pairs(FOLD_FWD, MIRB, 68), pairs(FOLD_FWD, 1044, 68))
    assert int((pairs(FOLD_FWD, MIRB + 68, 4) != 0).sum()) == 0
    bias_new = words[FOLD_FWD + FOLD_BIAS * 512: FOLD_FWD + FOLD_BIAS * 512 + 3072]
    bias_old = words[F32_FLOATS - (1920 + 704) * 256 - 3072: F32_FLOATS - (1920 + 704) * 256]
    keep = torch.ones(3072, dtype=torch.bool, device=DEV)
    keep[2049:2052] = False          # folded normal bias
    keep[2320:2448] = False          # folded dir_encoding bias
    assert torch.equal(bias_new[keep], bias_old[keep])
