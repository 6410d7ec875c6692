"""Mirror roughness (app_control_mirror_roughness) on chunks in which only some rays are mirror rays: THE RULE of include/mnrf.h
"Mirror roughness" through batched_inference, on both routes of the driver (the jitter fan and the one-by-one loop).

The weights and rays of fixture g7_eval_l1 (STRADDLE, 39 of its 96 rays are mirror rays; in chunks of 32: 5, 25 and 9) with
injected draws, std 0.01, one bounce and trace_ray_times = 3.  Before the rule the driver raised on every one of these chunks
(the reference adds (M,3) colours to an (N,3) render), and on a chunk with ONE mirror ray it silently spread that ray's
jitter colours over all rows of the reflection image.

Every comparison that the rule makes exact is torch.equal.  Against render_eval_rough at fixtures.tolerance (1e-4; depth and
x_surface 8e-4), measured on an MI355X with both arithmetics and both chunk sizes: rgb_fine and rgb_fine_reflect 3.0e-7 at
most, reflect_direction 7.7e-7, depth_fine_reflect 1.2e-7, the mirror mask 0."""
import numpy as np
import pytest
import torch

from oracle import mirror_nerf_oracle as O
from tests import rough_ref as RR
from tests.golden import fixtures as FX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EMB_O = {"xyz": 10, "dir": 4}
TIMES, STD = 3, 0.01


@pytest.fixture(autouse=True, params=["split", "fp32"])
def precision(request):
    """Both arithmetics of the field kernel, as the parity tests."""
    from mirror_nerf_amd import mirror_nerf as MN
    old = MN.PRECISION
    MN.set_precision(request.param)
    yield request.param
    MN.set_precision(old)


def _M():
    import mirror_nerf_amd as M
    return M


def _module(sd):
    M = _M()
    m = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV)


def _emb():
    M = _M()
    return {"xyz": M.Embedding(10), "dir": M.Embedding(4)}


_G7 = {}


def _g7():
    """Fixture g7_eval_l1 once: rays, numpy weights, the roughness arguments."""
    if not _G7:
        fx = FX.Fixture("g7_eval_l1")
        sds = fx.state_dicts()
        _G7.update(fx=fx, sds=sds, rays=fx.inputs["rays"],
                   args=dict(fx.meta["args"], app_control_mirror_roughness=True, trace_ray_times=TIMES, normal_noise_std=STD))
    return _G7


def _draws(n_rays, chunk, per_chunk, seed=5):
    """per_chunk (n,3) standard-normal draws for every chunk of the frame, in the order the driver consumes them."""
    rs = np.random.RandomState(seed)
    out = []
    for s in range(0, n_rays, chunk):
        n = min(chunk, n_rays - s)
        out += [rs.normal(size=(n, 3)).astype(np.float32) for _ in range(per_chunk)]
    return out


def _run(models, rays, chunk, args, draws=None, n_s=64, n_i=64, **kw):
    noise = None if draws is None else iter([torch.from_numpy(d) for d in draws])
    return _M().batched_inference(models, _emb(), rays, n_s, n_i, False, chunk, args=args, trace_secondary_rays=True,
                                  normal_noise_std=args.get("normal_noise_std", 0), _normal_noise=noise, to_cpu=False, **kw)


_WANT = {}


def _want(chunk):
    """render_eval_rough on the g7 frame, once per chunk size (shared, never modified)."""
    if chunk not in _WANT:
        g = _g7()
        m = g["fx"].meta
        _WANT[chunk] = RR.render_eval_rough({"coarse": g["sds"][0], "fine": g["sds"][1]}, EMB_O, g["rays"], m["N_samples"],
                                            m["N_importance"], False, chunk, g["args"],
                                            normal_noise=iter(_draws(96, chunk, TIMES + 1)), finish_mode=RR.DEVICE_FINISH)
    return _WANT[chunk]


@pytest.mark.parametrize("chunk,counts", [(96, [39]), (32, [5, 25, 9])])
def test_partly_mirrored_chunks_on_both_routes(chunk, counts):
    g = _g7()
    models = {"coarse": _module(g["sds"][0]), "fine": _module(g["sds"][1])}
    rays = torch.from_numpy(g["rays"]).to(DEV)
    draws = _draws(96, chunk, TIMES + 1)
    fan = _run(models, rays, chunk, g["args"], draws, batch_jitter=True)
    one = _run(models, rays, chunk, g["args"], draws, batch_jitter=False)
    mask = fan["mirror_mask_fine"] != 0
    assert [int(mask[s:s + chunk].sum()) for s in range(0, 96, chunk)] == counts
    assert set(fan) == set(one)
    for k in fan:
        assert torch.equal(fan[k], one[k]), k
    want = _want(chunk)
    for k in g["fx"].outputs:                                            # the keys the fixture pins for this frame
        if k in FX.PER_SAMPLE_FINE:
            continue
        w = want[k]
        got = fan[k].cpu().numpy()
        tol = FX.tolerance(k, g["fx"].meta)
        err = float(np.max(np.abs(got.astype(np.float64) - w)))
        print(f"chunk {chunk} {k}: max-abs {err:.3e} (tolerance {tol:.1e})")
        assert got.shape == w.shape and err <= tol, (k, err, tol)


def test_mirror_rows_are_the_all_mirror_arithmetic_and_the_others_keep_their_sample():
    g = _g7()
    models = {"coarse": _module(g["sds"][0]), "fine": _module(g["sds"][1])}
    rays = torch.from_numpy(g["rays"]).to(DEV)
    draws = _draws(96, 96, TIMES + 1)
    got = _run(models, rays, 96, g["args"], draws)
    mask = got["mirror_mask_fine"] != 0
    mb = mask.cpu().numpy()
    assert int(mask.sum()) == 39
    # the mirror rays alone, with their rows of the draws: a chunk in which every ray is a mirror ray, the arithmetic G8 pins
    alone = _run(models, rays[mask].contiguous(), 96, g["args"], [d[mb] for d in draws])
    assert bool((alone["mirror_mask_fine"] != 0).all())
    assert torch.equal(got["rgb_fine"][mask], alone["rgb_fine"])
    assert torch.equal(got["rgb_fine_reflect"][mask], alone["rgb_fine_reflect"])
    # the other rays: the frame without roughness, and the one reflection sample of draw 0
    off = _run(models, rays, 96, dict(g["args"], app_control_mirror_roughness=False))
    single = _run(models, rays, 96, dict(g["args"], trace_ray_times=0), draws[:1])
    assert torch.equal(got["rgb_fine"][~mask], off["rgb_fine"][~mask])
    assert torch.equal(got["rgb_fine_reflect"][~mask], single["rgb_fine_reflect"][~mask])
    assert not torch.equal(got["rgb_fine_reflect"][mask], single["rgb_fine_reflect"][mask])
    assert torch.equal(got["depth_fine_reflect"], single["depth_fine_reflect"])
    assert torch.equal(got["reflect_direction"], single["reflect_direction"])


def test_one_mirror_ray_in_the_chunk_does_not_reach_the_other_rows():
    """STRADDLE, seed 0, synthetic_rays(64, 64)[::3][:200], 64 + 128 samples: the frame in which the reference's addition
    broadcasts.  No ray of STRADDLE lies within 2e-4 of the threshold, so the device mask has the oracle's few mirror rays."""
    from mirror_nerf_amd import synthetic as SY
    models = SY.build_models(DEV, SY.STRADDLE, seed=0)[0]
    rays = torch.from_numpy(O.synthetic_rays(64, 64)[::3][:200].copy()).to(DEV)
    args = dict(predict_normal=True, only_one_field=False, only_one_field_fine_epoch=2, max_recursive_level=1,
                app_control_mirror_roughness=True, trace_ray_times=TIMES, normal_noise_std=STD)
    draws = _draws(200, 200, TIMES + 1, seed=6)
    single = _run(models, rays, 200, dict(args, trace_ray_times=0), draws[:1], n_i=128)
    for batch in (True, False):
        got = _run(models, rays, 200, args, draws, n_i=128, batch_jitter=batch)
        mask = got["mirror_mask_fine"] != 0
        assert 1 <= int(mask.sum()) <= 199
        assert torch.equal(got["rgb_fine_reflect"][~mask], single["rgb_fine_reflect"][~mask])
        assert not torch.equal(got["rgb_fine_reflect"][mask], single["rgb_fine_reflect"][mask])


def test_one_jitter_without_noise_is_the_frame_without_roughness():
    """trace_ray_times = 1, std 0: (R + R) finished by 2 is R, on every row."""
    g = _g7()
    models = {"coarse": _module(g["sds"][0]), "fine": _module(g["sds"][1])}
    rays = torch.from_numpy(g["rays"]).to(DEV)
    off = _run(models, rays, 96, dict(g["args"], app_control_mirror_roughness=False))
    for batch in (True, False):
        got = _run(models, rays, 96, dict(g["args"], trace_ray_times=1, normal_noise_std=0), _draws(96, 96, 2), batch_jitter=batch)
        assert torch.equal(got["rgb_fine"], off["rgb_fine"])


def test_two_bounces_with_random_draws():
    g = _g7()
    models = {"coarse": _module(g["sds"][0]), "fine": _module(g["sds"][1])}
    rays = torch.from_numpy(g["rays"]).to(DEV)
    args = dict(g["args"], max_recursive_level=2)
    off = _run(models, rays, 96, dict(args, app_control_mirror_roughness=False))
    torch.manual_seed(0)
    got = _run(models, rays, 96, args)                                   # the fan route, torch.randn draws
    mask = got["mirror_mask_fine"] != 0
    assert 1 <= int(mask.sum()) <= 95
    for k in ("rgb_fine", "rgb_fine_reflect", "depth_fine_reflect"):
        assert bool(torch.isfinite(got[k]).all()), k
    assert torch.equal(got["rgb_fine"][~mask], off["rgb_fine"][~mask])
    assert not torch.equal(got["rgb_fine"][mask], off["rgb_fine"][mask])


def test_maps_only_gives_the_full_frames_maps():
    g = _g7()
    models = {"coarse": _module(g["sds"][0]), "fine": _module(g["sds"][1])}
    rays = torch.from_numpy(g["rays"]).to(DEV)
    draws = _draws(96, 32, TIMES + 1)
    full = _run(models, rays, 32, g["args"], draws)
    for kw in (dict(maps_only=True), dict(maps_only=True, batch_jitter=True)):
        maps = _run(models, rays, 32, g["args"], draws, **kw)
        assert {"rgb_fine", "rgb_fine_reflect", "depth_fine", "depth_fine_reflect", "mirror_mask_fine"} <= set(maps)
        for k, v in maps.items():
            assert torch.equal(v, full[k]), k
    host = _M().batched_inference(models, _emb(), rays, 64, 64, False, 32, args=g["args"], trace_secondary_rays=True,
                                  normal_noise_std=STD, _normal_noise=iter([torch.from_numpy(d) for d in draws]), to_cpu="maps")
    for k, v in host.items():
        assert torch.equal(v, full[k].cpu()), k


def test_one_compaction_per_chunk_and_level_whatever_the_number_of_jitters(monkeypatch):
    """The fan route compacts the mask -- and reads the count on the host -- once per chunk of level 0, for 3 jitters as for 9;
    the one-by-one route keeps one compaction per jitter beside it."""
    from mirror_nerf_amd import recursion as R
    g = _g7()
    models = {"coarse": _module(g["sds"][0]), "fine": _module(g["sds"][1])}
    rays = torch.from_numpy(g["rays"]).to(DEV)
    calls = []
    reflect = R._reflect

    def counting(rays_, x, n, mask, compact, *a, **k):
        calls.append(bool(compact))
        return reflect(rays_, x, n, mask, compact, *a, **k)

    monkeypatch.setattr(R, "_reflect", counting)
    for times, batch, want in ((3, True, 3), (9, True, 3), (3, False, 3 * (1 + 3))):
        calls.clear()
        _run(models, rays, 32, dict(g["args"], trace_ray_times=times), _draws(96, 32, times + 1), batch_jitter=batch)
        assert sum(calls) == want and len(calls) - sum(calls) == 3, (times, batch, calls)


def test_all_mirror_fixture_through_the_fan():
    """g8_rough_allmirror (M == N: the reference's own arithmetic) through the jitter fan and the mean kernel."""
    fx = FX.Fixture("g8_rough_allmirror")
    m = fx.meta
    sds = fx.state_dicts()
    models = {"coarse": _module(sds[0]), "fine": _module(sds[1])}
    draws = [fx.inputs[f"normal_noise_{i}"] for i in range(3)]
    rays = torch.from_numpy(fx.inputs["rays"]).to(DEV)
    for batch in (True, False):
        got = _run(models, rays, m["chunk"], m["args"], draws, n_s=m["N_samples"], n_i=m["N_importance"], batch_jitter=batch)
        for k, want in fx.outputs.items():
            if k in FX.PER_SAMPLE_FINE:
                continue
            err = float(np.max(np.abs(got[k].cpu().numpy().astype(np.float64) - want)))
            assert err <= FX.tolerance(k, m), (k, err)
