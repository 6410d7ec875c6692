"""Structural similarity on the device (csrc/mnrf_metrics.hip through mirror_nerf_amd.metrics) against the float64 numpy
restatement of tests/ssim_ref.py.

Tolerance: S and its mean lie in [-1, 1] and the kernel evaluates the moments and S in float64, so the device differs from
the restatement by the final float32 rounding (<= 6e-8) plus float64 noise; 1e-6 absolute, on the mean and on every pixel of
the map, leaves an order of magnitude.  The plain float32 E[x^2] - E[x]^2 misses it by 40x in the mean and reaches 1e-3 per
pixel (the variances cancel against C2 = 9e-4).  Layouts, batching and repeated runs are compared bit for bit."""
import numpy as np
import pytest
import torch

from tests import ssim_ref as R
from tests.golden import fixtures as FX

pytestmark = pytest.mark.gpu

TOL = 1e-6
SHAPES = [(64, 64), (37, 53), (800, 800)]
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _chw(a):
    """(H, W, 3) -> (1, 3, H, W), contiguous."""
    return np.ascontiguousarray(a.transpose(2, 0, 1))[None]


def _fixture_pairs():
    """The trained pair of fixtures G11: its rendered 48x48 frame against the ground truth it was trained on
    (g11_trained_psnr), and two maps of g11_trained_render_test over the same 128 rays, reshaped to 8x16x3."""
    z = FX.Fixture("g11_trained_psnr")
    res = z.meta["res"]
    yield "g11_frame_vs_gt", z.outputs["rgb_fine"].reshape(res, res, 3), z.inputs["gt_rgb"].reshape(res, res, 3)
    y = FX.Fixture("g11_trained_render_test").outputs
    yield "g11_render_test_maps", y["rgb_fine"].reshape(8, 16, 3), (0.5 * y["surface_normal_fine"] + 0.5).reshape(8, 16, 3)


def _check_pair(name, p, t):
    from mirror_nerf_amd import metrics
    p, t = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(t, np.float32)
    got = metrics.structural_similarity(_dev(p), _dev(t))
    assert got.dtype == torch.float32 and got.dim() == 0 and got.is_cuda
    want = R.structural_similarity(p, t)
    print(f"{name}: structural_similarity device {float(got):.9f} restatement {want:.9f} diff {abs(float(got) - want):.3e}")
    assert abs(float(got) - want) <= TOL

    want_map = R.ssim_map(_chw(p), _chw(t))
    got_mean = metrics.ssim(_dev(_chw(p)), _dev(_chw(t)))
    got_map = metrics.ssim(_dev(_chw(p)), _dev(_chw(t)), reduction="none")
    assert got_mean.dtype == torch.float32 and got_mean.dim() == 0
    assert got_map.shape == (1, 3) + p.shape[:2] and got_map.dtype == torch.float32
    d_mean = abs(float(got_mean) - float(want_map.mean()))
    d_map = float(np.max(np.abs(got_map.cpu().numpy().astype(np.float64) - want_map)))
    print(f"{name}: ssim device {float(got_mean):.9f} restatement {want_map.mean():.9f} diff {d_mean:.3e}  map max diff {d_map:.3e}")
    assert d_mean <= TOL
    assert d_map <= TOL


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", R.KINDS)
def test_synthetic_pairs_match_the_restatement(kind, shape):
    p, t = R.pair(kind, *shape)
    _check_pair(f"{kind} {shape[0]}x{shape[1]}", p, t)


@pytest.mark.parametrize("which", [0, 1], ids=["g11_frame_vs_gt", "g11_render_test_maps"])
def test_rendered_fixture_frames_match_the_restatement(which):
    name, p, t = list(_fixture_pairs())[which]
    _check_pair(name, p, t)


@pytest.mark.parametrize("win_size", [3, 5, 9, 11])
def test_other_window_sizes(win_size):
    from mirror_nerf_amd import metrics
    p, t = R.pair("smooth_noise", 37, 53)
    got = float(metrics.structural_similarity(_dev(p), _dev(t), win_size=win_size))
    assert abs(got - R.structural_similarity(p, t, win_size)) <= TOL
    p2, t2 = p[:win_size, :win_size + 1], t[:win_size, :win_size + 1]      # one window tall: the smallest image that is accepted
    assert abs(float(metrics.structural_similarity(_dev(p2), _dev(t2), win_size=win_size)) -
               R.structural_similarity(p2, t2, win_size)) <= TOL


def test_data_range_scales_the_constants():
    from mirror_nerf_amd import metrics
    p, t = R.pair("quantised", 37, 53)
    p255, t255 = np.round(p * 255.0), np.round(t * 255.0)
    got = float(metrics.structural_similarity(_dev(p255), _dev(t255), data_range=255.0))
    assert abs(got - R.structural_similarity(p255, t255, data_range=255.0)) <= TOL


@pytest.mark.parametrize("kind", R.KINDS)
def test_identical_images_give_exactly_one(kind):
    from mirror_nerf_amd import metrics
    p, _ = R.pair(kind, 37, 53)
    assert float(metrics.structural_similarity(_dev(p), _dev(p))) == 1.0
    q = _dev(_chw(p))
    assert float(metrics.ssim(q, q)) == 1.0
    assert bool((metrics.ssim(q, q, reduction="none") == 1.0).all())


def test_constant_images_give_the_luminance_term():
    from mirror_nerf_amd import metrics
    a, b, c1 = np.float32(0.2), np.float32(0.6), 1e-4
    want = (2.0 * float(a) * float(b) + c1) / (float(a) ** 2 + float(b) ** 2 + c1)
    p, t = np.full((40, 45, 3), a, np.float32), np.full((40, 45, 3), b, np.float32)
    assert abs(float(metrics.structural_similarity(_dev(p), _dev(t))) - want) <= TOL
    assert abs(float(metrics.ssim(_dev(_chw(p)), _dev(_chw(t)))) - want) <= TOL
    got_map = metrics.ssim(_dev(_chw(p)), _dev(_chw(t)), reduction="none")
    assert float((got_map.double() - want).abs().max()) <= TOL


def test_layouts_are_read_in_place_and_agree_bit_for_bit():
    """The same data as a contiguous (H, W, 3) tensor, as a non-contiguous (H, W, 3) view cut out of a larger RGBA buffer and
    as a (1, 3, H, W) tensor (permuted to the layout each entry point takes) give the same bits."""
    from mirror_nerf_amd import metrics
    p, t = R.pair("smooth_noise", 37, 53)
    dp, dt = _dev(p), _dev(t)
    big_p = torch.full((40, 60, 4), 7.0, device=DEV)
    big_t = torch.full((40, 60, 4), -3.0, device=DEV)
    big_p[2:39, 5:58, :3] = dp
    big_t[2:39, 5:58, :3] = dt
    vp, vt = big_p[2:39, 5:58, :3], big_t[2:39, 5:58, :3]
    assert not vp.is_contiguous()
    cp, ct = _dev(_chw(p)), _dev(_chw(t))                      # (1, 3, H, W)

    s0 = metrics.structural_similarity(dp, dt)
    assert torch.equal(metrics.structural_similarity(vp, vt), s0)
    assert torch.equal(metrics.structural_similarity(vp, dt), s0)                   # each image has its own strides
    s_chw = metrics.structural_similarity(cp.permute(0, 2, 3, 1), ct.permute(0, 2, 3, 1))
    assert s_chw.shape == (1,) and torch.equal(s_chw[0], s0)

    k0 = metrics.ssim(cp, ct)
    assert torch.equal(metrics.ssim(dp.permute(2, 0, 1)[None], dt.permute(2, 0, 1)[None]), k0)
    assert torch.equal(metrics.ssim(vp.permute(2, 0, 1)[None], vt.permute(2, 0, 1)[None]), k0)
    assert torch.equal(metrics.ssim(vp.permute(2, 0, 1)[None], vt.permute(2, 0, 1)[None], reduction="none"),
                       metrics.ssim(cp, ct, reduction="none"))
    assert float(big_p[0, 0, 0]) == 7.0 and float(big_p[5, 5, 3]) == 7.0           # nothing was written around the view


def test_a_stack_of_frames_equals_the_single_frames_bit_for_bit():
    from mirror_nerf_amd import metrics
    pairs = [R.pair(R.KINDS[i % 4], 37, 53, seed=i) for i in range(5)]
    sp = _dev(np.stack([p for p, _ in pairs]))
    st = _dev(np.stack([t for _, t in pairs]))
    got = metrics.structural_similarity(sp, st)
    assert got.shape == (5,) and got.dtype == torch.float32
    for i, (p, t) in enumerate(pairs):
        assert torch.equal(got[i], metrics.structural_similarity(_dev(p), _dev(t))), i
        assert abs(float(got[i]) - R.structural_similarity(p, t)) <= TOL
    # metrics.ssim over a batch: the mean over every element, and the per-image maps
    bp, bt = sp.permute(0, 3, 1, 2), st.permute(0, 3, 1, 2)
    want = np.concatenate([R.ssim_map(_chw(p), _chw(t)) for p, t in pairs])
    assert abs(float(metrics.ssim(bp, bt)) - float(want.mean())) <= TOL
    got_map = metrics.ssim(bp, bt, reduction="none")
    assert float(np.max(np.abs(got_map.cpu().numpy().astype(np.float64) - want))) <= TOL
    for i in range(5):
        assert torch.equal(got_map[i], metrics.ssim(bp[i:i + 1], bt[i:i + 1], reduction="none")[0]), i


def test_two_runs_are_bit_identical():
    from mirror_nerf_amd import metrics
    p, t = R.pair("hard_edge", 800, 800)
    dp, dt = _dev(p), _dev(t)
    a, b = metrics.structural_similarity(dp, dt), metrics.structural_similarity(dp, dt)
    assert torch.equal(a, b)
    cp, ct = dp.permute(2, 0, 1)[None], dt.permute(2, 0, 1)[None]
    assert torch.equal(metrics.ssim(cp, ct), metrics.ssim(cp, ct))
    assert torch.equal(metrics.ssim(cp, ct, reduction="none"), metrics.ssim(cp, ct, reduction="none"))


def test_frame_metrics():
    from mirror_nerf_amd import metrics
    p, t = R.pair("smooth_noise", 64, 64)
    dp, dt = _dev(p), _dev(t)
    psnr, s = metrics.frame_metrics(dp, dt)
    assert psnr.dim() == 0 and s.dim() == 0
    assert torch.equal(psnr, metrics.psnr(dp, dt))
    assert torch.equal(s, metrics.structural_similarity(dp, dt))
    pairs = [R.pair(R.KINDS[i % 4], 64, 64, seed=10 + i) for i in range(5)]
    sp, st = _dev(np.stack([a for a, _ in pairs])), _dev(np.stack([b for _, b in pairs]))
    psnr, s = metrics.frame_metrics(sp, st)
    assert psnr.shape == (5,) and s.shape == (5,)
    for i in range(5):
        assert torch.equal(psnr[i], metrics.psnr(sp[i], st[i])), i
        assert torch.equal(s[i], metrics.structural_similarity(sp[i], st[i])), i
        want = -10.0 * np.log10(np.mean((pairs[i][0].astype(np.float64) - pairs[i][1]) ** 2))
        assert abs(float(psnr[i]) - want) <= 1e-4


def test_an_image_smaller_than_the_window_is_refused():
    from mirror_nerf_amd import metrics
    a = torch.zeros(5, 64, 3, device=DEV)
    with pytest.raises(RuntimeError, match="mnrf_ssim: image smaller than the window"):
        metrics.structural_similarity(a, a)
    with pytest.raises(RuntimeError, match="mnrf_ssim: image smaller than the window"):
        metrics.structural_similarity(a.permute(1, 0, 2), a.permute(1, 0, 2))
    b = torch.zeros(1, 3, 2, 64, device=DEV)
    with pytest.raises(RuntimeError, match="mnrf_ssim: image smaller than the window"):
        metrics.ssim(b, b)
    assert float(metrics.structural_similarity(a, a, win_size=5)) == 1.0


def test_eval_metrics_tool(tmp_path):
    """scripts/eval_metrics.py on a made-up split: RGB results, an RGBA ground truth of another size (blended on white and
    resized to the result's size) -- against the restatement on the images the tool's own loader returns."""
    import json
    import os
    import subprocess
    import sys
    Image = pytest.importorskip("PIL.Image")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "scripts"))
    try:
        import eval_metrics as tool
    finally:
        sys.path.pop(0)
    scene, res_dir = tmp_path / "scene", tmp_path / "results"
    (scene / "test").mkdir(parents=True)
    res_dir.mkdir()
    frames, want_psnr, want_ssim = [], [], []
    for i in range(3):
        p, t = R.pair(R.KINDS[i], 40, 56, seed=20 + i)
        Image.fromarray(np.round(p * 255).astype(np.uint8)).save(res_dir / f"rgb_fine_{i:03d}.png")
        big = np.kron(np.round(t * 255).astype(np.uint8), np.ones((2, 2, 1), np.uint8))       # (80, 112, 3)
        alpha = np.full(big.shape[:2] + (1,), 255, np.uint8)
        alpha[:10] = 128
        Image.fromarray(np.concatenate([big, alpha], -1), "RGBA").save(scene / "test" / f"{i}.png")
        frames.append({"file_path": f"test/{i}.png"})
        a, wh = tool.load_image(str(res_dir / f"rgb_fine_{i:03d}.png"))
        b, _ = tool.load_image(str(scene / "test" / f"{i}.png"), resize_wh=wh)
        assert a.shape == b.shape == (40, 56, 3) and a.dtype == b.dtype == np.float32
        want_ssim.append(R.structural_similarity(a, b))
        want_psnr.append(-10.0 * np.log10(np.mean((a.astype(np.float64) - b) ** 2)))
    (scene / "transforms_test.json").write_text(json.dumps({"frames": frames}))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "eval_metrics.py"), "--split_path",
                        str(scene / "transforms_test.json"), "--res_img_dir", str(res_dir)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    words = r.stdout.strip().splitlines()[-1].split()
    assert words[:2] == ["Mean", "PSNR"] and words[3] == "SSIM" and words[5:] == ["LPIPS", "n/a"], r.stdout
    assert abs(float(words[2]) - np.mean(want_psnr)) <= 1e-4
    assert abs(float(words[4]) - np.mean(want_ssim)) <= TOL
