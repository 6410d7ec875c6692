"""The float64 hash-grid reference of tests/torch_ref.py and the clouds of tests/tcnn_cases.py, checked on their own (no GPU): the
reference pieces against brute-force loops on tiny tables and against the fp32 oracle, the clouds against what they claim, and the
cap on the conditioning mask that tests/test_hip_tcnn_fp64.py relies on."""
import numpy as np
import pytest
import torch

from oracle import mirror_nerf_oracle as O
from tests import tcnn_cases as C
from tests import torch_ref as R

# three levels, one of each kind: 3^3 = 27 nodes in 32 entries (dense), 5^3 = 125 nodes in 40 entries (hashed, modulo),
# 9^3 = 729 nodes in 64 entries (hashed, power of two)
TINY = dict(offsets=np.array([0, 32, 72, 136], dtype=np.int64), S=1.0, H=2, n_levels=3, level_dim=2, bound=1.5)


def _tiny_inputs(n=40, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = ((torch.rand(n, 3, generator=g) * 2 - 1) * 1.5).float()
    x[0] = torch.tensor([1.5, -1.5, 0.3])           # on two faces of the box (0.0 would be a cell face of every level here)
    x[1] = torch.tensor([2.0, 0.0, 0.0])            # outside
    x[2] = torch.tensor([0.0, 0.0, -1.6])           # outside
    table = torch.randn(136, 2, generator=g, dtype=torch.float64)
    return x, table


def _brute_index(loc, hsize, res):
    stride, index, d = 1, 0, 0
    while d < 3 and stride <= hsize:
        index += int(loc[d]) * stride
        stride *= res + 1
        d += 1
    if stride > hsize:
        index = 0
        for k, prime in enumerate((1, 2654435761, 805459861)):
            index ^= (int(loc[k]) * prime) % 2 ** 32
    return (index % 2 ** 32) % hsize


def _brute(x, table, cfg, g_enc=None):
    """Loops over samples, levels and corners in Python floats (float64): encoding, per-entry contribution counts, per-level S,
    and the two sums of the rounding bound (derivative sum, weighted value sum)."""
    B, L = x.shape[0], cfg["n_levels"]
    enc = np.zeros((B, 2 * L))
    n_e = np.zeros(int(cfg["offsets"][-1]), dtype=np.int64)
    S = np.zeros(L)
    dsum, wsum = np.zeros((B, 2 * L)), np.zeros((B, 2 * L))
    bound = cfg["bound"]
    for i in range(B):
        u32 = [np.float32(np.float32(x[i, a]) + np.float32(bound)) / np.float32(2 * bound) for a in range(3)]
        if any(v < 0 or v > 1 for v in u32):
            continue
        u = [(float(x[i, a]) + bound) / (2 * bound) for a in range(3)]
        for lv in range(L):
            scale = float(np.float32(2.0 ** (lv * cfg["S"]) * cfg["H"] - 1.0))
            res = int(np.ceil(scale)) + 1
            off0, hsize = int(cfg["offsets"][lv]), int(cfg["offsets"][lv + 1] - cfg["offsets"][lv])
            pos = [u[a] * scale + 0.5 for a in range(3)]
            pg = [int(np.floor(p)) for p in pos]
            fr = [pos[a] - pg[a] for a in range(3)]
            if g_enc is not None:
                S[lv] += max(abs(g_enc[i, 2 * lv]), abs(g_enc[i, 2 * lv + 1]))
            for c in range(8):
                bit = [(c >> a) & 1 for a in range(3)]
                wa = [fr[a] if bit[a] else 1 - fr[a] for a in range(3)]
                e = off0 + _brute_index([pg[a] + bit[a] for a in range(3)], hsize, res)
                n_e[e] += 1
                for f in range(2):
                    v = float(table[e, f])
                    enc[i, 2 * lv + f] += wa[0] * wa[1] * wa[2] * v
                    wsum[i, 2 * lv + f] += wa[0] * wa[1] * wa[2] * abs(v)
                    dsum[i, 2 * lv + f] += (wa[1] * wa[2] + wa[0] * wa[2] + wa[0] * wa[1]) * abs(v)
    return enc, n_e, S, dsum, wsum


def test_tiny_table_has_one_level_of_each_kind():
    facts = C.level_facts(TINY)
    assert [f["mode"] for f in facts] == [0, 2, 1]


def test_grid_index_matches_brute_force_and_the_oracle():
    rs = np.random.RandomState(0)
    for hsize, res in ((32, 2), (40, 4), (64, 8), (C.ODD_ENTRIES, 31), (16384, 4000), (13824, 23)):
        loc = rs.randint(0, res + 1, (200, 3))
        got = R.tcnn_grid_index(torch.from_numpy(loc), hsize, res).numpy()
        want = np.array([_brute_index(row, hsize, res) for row in loc])
        assert np.array_equal(got, want), (hsize, res)
        assert np.array_equal(got, O._grid_index(loc.astype(np.uint32), hsize, res)), (hsize, res)
        assert got.max() < hsize


def test_encoding_counts_and_sums_match_brute_force():
    x, table = _tiny_inputs()
    g_enc = torch.randn(x.shape[0], 6, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    enc, n_e, S, _d, _w = _brute(x.numpy(), table.numpy(), TINY, g_enc.numpy())
    got = R.tcnn_encode(x, table, TINY, pos="f64")
    assert float((got - torch.from_numpy(enc)).abs().max()) <= 1e-13
    assert bool((got[1] == 0).all()) and bool((got[2] == 0).all()) and bool((got[0] != 0).any())      # outside / on the face
    assert np.array_equal(R.tcnn_entry_counts(x, TINY).numpy(), n_e)
    assert int(n_e.sum()) == 8 * 3 * (x.shape[0] - 2)
    assert float((R.tcnn_level_sums(g_enc, x, TINY) - torch.from_numpy(S)).abs().max()) <= 1e-12
    # pos = "f32" differs from "f64" by the rounding of pos only: the weights move by at most 2 ulp32(pos) each
    near = R.tcnn_encode(x, table, TINY, pos="f32")
    assert 0 < float((near - got).abs().max()) <= 1e-5


def test_encoding_is_differentiable_with_the_exact_slope():
    """d enc / d x through `xd`: against central differences of the float64 encoding, away from the cell faces."""
    x, table = _tiny_inputs(n=12, seed=5)
    x = x[3:]
    xd = x.double().clone().requires_grad_(True)
    enc = R.tcnn_encode(x, table, TINY, "f32", xd)
    cot = torch.randn(enc.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    (g,) = torch.autograd.grad((enc * cot).sum(), xd)
    h = 1e-4      # in fp32-representable steps the "f64" encoding is exact to 1e-16: the difference quotient is good to 1e-8
    for a in range(3):
        step = torch.zeros(3)
        step[a] = h
        hi, lo = (x + step).float(), (x - step).float()
        fd = ((R.tcnn_encode(hi, table, TINY, "f64") - R.tcnn_encode(lo, table, TINY, "f64")) * cot).sum(-1) / (hi - lo)[:, a].double()
        same_cell = torch.ones(x.shape[0], dtype=torch.bool)
        for scale, _r, _o, _h in R.tcnn_levels(TINY):
            same_cell &= (torch.floor(R.tcnn_pos(hi, 1.5, scale, "f64")) == torch.floor(R.tcnn_pos(lo, 1.5, scale, "f64"))).all(-1)
        assert int(same_cell.sum()) >= 3
        assert float((fd - g[:, a])[same_cell].abs().max()) <= 1e-6 * float(g.abs().max())


def test_plane_bound_matches_brute_force_off_the_faces():
    x, table = _tiny_inputs()
    _e, _n, _S, dsum, wsum = _brute(x.numpy(), table.numpy(), TINY)
    got = R.tcnn_plane_bound(x, table, TINY)
    assert not bool(R.tcnn_near_face(x, TINY).any())
    eps = 2.0 ** -23
    for lv, (scale, _r, _o, _h) in enumerate(R.tcnn_levels(TINY)):
        p = R.tcnn_pos(x, 1.5, scale, "f64")
        ulp = torch.exp2(torch.floor(torch.log2(p)) - 23).amax(-1)
        want = 2 * ulp[:, None] * torch.from_numpy(dsum[:, 2 * lv:2 * lv + 2]) + 12 * eps * torch.from_numpy(wsum[:, 2 * lv:2 * lv + 2])
        want[1:3] = 0                      # outside the box
        assert float((got[:, 2 * lv:2 * lv + 2] - want).abs().max()) <= 1e-18 + 1e-12 * float(want.max())


@pytest.mark.parametrize("name,bound", [("small", 1.0), ("odd", 1.0), ("mid", 1.0)])
def test_plane_bound_holds_for_the_fp32_oracle(name, bound):
    """The oracle's encoding is an fp32 evaluation by other code (numpy): it must lie within the derived bound of the float64
    reference -- on the random cloud and on the cloud of faces, corners and cell faces -- and the bound must stay a rounding
    bound, not a licence: nowhere above 2 ulp32(finest scale) x 3 axes x 2 max |v| (eight corners, the
    other two weights adding up to 1 on either side of the axis) + 12 eps32 x max |v|."""
    cfg = C.table_config(name, bound)
    table = (torch.rand(int(cfg["offsets"][-1]), 2, generator=C.gen("table", name), dtype=torch.float64) - 0.5)
    x = torch.cat([C.random_cloud(300, bound), C.edges_cloud(bound, cfg)[0], C.one_cell_cloud(bound, cfg, 32)])
    u32 = C.pos32(x, bound, 1.0)[0]
    fp32 = O.hashgrid_encode(u32.numpy(), table.float().numpy(), cfg)
    ref = R.tcnn_encode(x, table.float().double(), cfg, pos="f64")
    bnd = R.tcnn_plane_bound(x, table.float().double(), cfg)
    err = (torch.from_numpy(fp32).double() - ref).abs()
    assert bool((err <= bnd).all()), float((err - bnd).max())
    top = C.level_facts(cfg)[-1]["scale"]
    cap = 2 * 2.0 ** (np.floor(np.log2(top + 0.5)) - 23) * 3 * 2 * 0.5 + 12 * 2.0 ** -23 * 0.5
    assert float(bnd.max()) <= cap <= 1e-3 and float(err.max()) > 0
    # the oracle computes its cells in fp32 like pos = "f32"
    same = R.tcnn_encode(x, table.float().double(), cfg, pos="f32")
    assert float((torch.from_numpy(fp32).double() - same).abs().max()) <= 12 * 2.0 ** -23 * 0.5


def test_table_configurations_reach_every_level_and_accumulation_kind():
    kinds = {n: C.level_facts(C.table_config(n, 1.0)) for n in C.TABLES}
    assert {f["copies"] for f in kinds["std"]} == {32, 8, 0} and {f["mode"] for f in kinds["std"]} == {0, 1}
    assert {f["copies"] for f in C.level_facts(C.table_config("std", 6.0))} == {32, 8, 0}
    assert {f["copies"] for f in kinds["small"]} == {32} and [f["mode"] for f in kinds["small"]][:3] == [0, 0, 1]
    assert {f["copies"] for f in kinds["mid"] if f["mode"]} == {8} and sum(f["mode"] == 1 for f in kinds["mid"]) >= 10
    assert {f["mode"] for f in kinds["odd"]} == {0, 2} and all(f["hsize"] == C.ODD_ENTRIES for f in kinds["odd"] if f["mode"])
    assert {f["copies"] for f in kinds["odd"]} == {32}
    from mirror_nerf_amd.mirror_nerf_tcnn import hashgrid_config
    for b in (1.0, 6.0):
        assert np.array_equal(C.table_config("std", b)["offsets"], hashgrid_config(b)["offsets"])


def _cells(x, bound, cfg, lv):
    return torch.floor(C.pos32(x, bound, C.level_facts(cfg)[lv]["scale"])[1]).long()


def _run_lengths(cells):
    change = (cells[1:] != cells[:-1]).any(-1)
    edges = [0] + (change.nonzero()[:, 0] + 1).tolist() + [cells.shape[0]]
    return tuple(b - a for a, b in zip(edges[:-1], edges[1:]))


@pytest.mark.parametrize("bound", [1.0, 6.0])
def test_clouds_do_what_they_claim(bound):
    cfg = C.table_config("std", bound)
    facts = C.level_facts(cfg)
    # runs: the run lengths at level 0, one run ending on lane 127 and one crossing lane 192
    x = C.runs_cloud(bound, cfg)
    assert _run_lengths(_cells(x, bound, cfg, 0)) == C.RUN_LENGTHS
    assert {1, 2, 63, 64, 65} <= set(C.RUN_LENGTHS) and sum(C.RUN_LENGTHS[:3]) == 128 and sum(C.RUN_LENGTHS[:4]) < 192 < sum(C.RUN_LENGTHS[:5])
    # one_cell: one cell of level 8, which the run aggregation covers (its key holds resolutions below 1023)
    x = C.one_cell_cloud(bound, cfg)
    assert x.shape[0] == 256 and len(torch.unique(_cells(x, bound, cfg, C.ONE_CELL_LEVEL), dim=0)) == 1
    assert facts[C.ONE_CELL_LEVEL]["res"] < 1023
    # edges: u == 0 and u == 1 exactly, the +bound neighbour rounds onto the face and the -bound neighbour is outside, and the
    # cell-face points have an integer pos at level 0
    x, parts = C.edges_cloud(bound, cfg)
    u = C.pos32(x, bound, 1.0)[0]
    assert bool((u[parts["box"]] == 0).any()) and bool((u[parts["box"]] == 1).any()) and bool((u[13] == 0.5).all())
    past = u[parts["past"]]
    oob = ((past < 0) | (past > 1)).any(-1)
    assert oob.tolist() == [True, False, True, False, True, False]
    pos0 = C.pos32(x, bound, facts[0]["scale"])[1]
    on3 = (pos0[parts["face3"]] == torch.round(pos0[parts["face3"]])).all(-1)
    # (where x is coarser than u no float lands on the integer: those points stay within 4 ulp of it, on either side)
    assert on3.numel() == 15 and int(on3.sum()) >= 10
    on1 = (pos0[parts["face1"]] == torch.round(pos0[parts["face1"]])).any(-1)
    assert on1.numel() == 45 and int(on1.sum()) >= 30
    assert bool(R.tcnn_near_face(x, cfg)[parts["face3"]].all()) and bool(R.tcnn_near_face(x, cfg)[parts["face1"]].all())
    # all_out: the middle tile wholly outside, the others wholly inside
    x, keep = C.all_out_cloud(bound)
    oob = R.tcnn_unit(x, bound)[2]
    assert bool(oob[256:512].all()) and not bool(oob[keep].any()) and int(keep.sum()) == 512


def _expected_share(cfg):
    return 3 * 8 * 2.0 ** -23 * sum(f["scale"] for f in C.level_facts(cfg))


def test_conditioning_mask_stays_under_its_cap_on_the_random_clouds():
    """The GPU tests compare normals and dL/d position off tcnn_near_face only.  Expected share of masked samples:
    3 axes x 8 ulp x 2^-23 x sum of the level scales = 1.6 % at bound 1 and 10 % at bound 6; the cap is twice that, 5 % and 20 %,
    and holds for the committed seeds at every sample count the GPU tests run."""
    assert 0.012 <= _expected_share(C.table_config("std", 1.0)) <= 0.025
    assert 0.08 <= _expected_share(C.table_config("std", 6.0)) <= 0.10
    sizes = sorted(set(C.FWD_B + C.BWD_B + (C.WRAP_FWD, C.WRAP_BWD)))
    for name in C.TABLES:
        cfg = C.table_config(name, 1.0)
        for B in sizes if name == "std" else (257,):
            share = float(R.tcnn_near_face(C.random_cloud(B, 1.0), cfg).float().mean())
            assert share <= 0.05, (name, B, share)
    cfg = C.table_config("std", 6.0)
    for B in (257, C.FX_SMALL_B, C.TRAIN_B, C.WRAP_FX):
        share = float(R.tcnn_near_face(C.random_cloud(B, 6.0), cfg).float().mean())
        assert share <= 0.20, (B, share)
        if B >= C.TRAIN_B:
            assert share >= 0.25 * _expected_share(cfg)          # (the mask is not empty either: it is the predicted effect)


def test_fixed_point_rule_brackets_the_measured_sizes():
    """The shim's rule: fixed point at the training step's sample count, fp32 atomics at the size where the yardstick
    was measured to fail."""
    from mirror_nerf_amd.mirror_nerf_tcnn import FIXED_MAX_SAMPLES
    assert C.FX_SMALL_B < C.TRAIN_B <= FIXED_MAX_SAMPLES < C.WRAP_FX


def _random_field_weights(cfg, seed=4):
    g = torch.Generator().manual_seed(seed)
    shapes = {"sigma_net.0.weight": (64, 32), "sigma_net.1.weight": (16, 64), "color_net.0.weight": (64, 31), "color_net.1.weight": (64, 64),
              "color_net.2.weight": (3, 64), "normal_net.0.weight": (64, 15), "normal_net.1.weight": (3, 64),
              "is_mirror_net.0.weight": (32, 15), "is_mirror_net.0.bias": (32,), "is_mirror_net.2.weight": (1, 32), "is_mirror_net.2.bias": (1,)}
    w = {k: (torch.randn(*s, generator=g, dtype=torch.float64) * 0.3) for k, s in shapes.items()}
    w["encoder.embeddings"] = torch.rand(int(cfg["offsets"][-1]), 2, generator=g, dtype=torch.float64) - 0.5
    return w


def test_second_order_magnitude_sums_dominate_the_double_backward():
    """The sums of magnitudes behind the second-order bounds (tcnn_hess_sums, tcnn_second_order_table_abs) against torch's double
    backward through normal = l2n(-d sigma / dx) alone: each is the same sum as the gradient with every term's magnitude, so it
    dominates the gradient entry by entry -- and not by orders (the terms do not all cancel)."""
    cfg = C.table_config("small", 1.0)
    w = {k: v.requires_grad_(True) for k, v in _random_field_weights(cfg).items()}
    x = torch.cat([C.random_cloud(40, 1.0), torch.tensor([[1.5, 0.0, 0.0]])])
    d = C.directions(41, "second")
    c = torch.randn(41, 3, generator=C.gen("c"), dtype=torch.float64)
    acts = {}
    o = R.tcnn_field64(w, x, d, cfg, with_normal=True, acts=acts)
    (o["normal"] * c).sum().backward()
    wd = {k: v.detach() for k, v in w.items()}
    table = wd["encoder.embeddings"]
    q, dq = R.tcnn_sigma_enc_grad(wd, acts)
    g = o["grad_sigma"].double()
    gn = g.norm(dim=-1).clamp_min(1e-300)
    n = -g / gn[:, None]
    t = (c - n * (n * c).sum(-1, keepdim=True)) / gn[:, None]
    # |d g_b| of the rounding of q alone is small against |g| itself: q and its bound are consistent
    assert float((dq / q.abs().clamp_min(1e-12)).median()) < 1e-4
    # d sigma / dx from q and the encoding's own derivative sums: |g_a| <= A_a(q)
    A = R.tcnn_dx_sums(x, table, cfg, q)[0]
    assert bool((g.abs() <= A * (1 + 1e-9) + 1e-300).all()) and float((g.abs() / A.clamp_min(1e-300))[:40].median()) > 1e-3
    H = R.tcnn_hess_sums(x, table, cfg, q)
    bound_x = (t.abs()[:, None, :] * H).sum(-1)
    gx = o["xd"].grad
    assert bool((gx.abs() <= bound_x * (1 + 1e-9) + 1e-300).all()) and bool((gx[40] == 0).all())
    assert float((gx.abs() / bound_x.clamp_min(1e-300))[:40].median()) > 1e-3
    T = R.tcnn_second_order_table_abs(x, table, cfg, wd, acts, o["grad_sigma"], c)
    gt = w["encoder.embeddings"].grad
    assert bool((gt.abs() <= T * (1 + 1e-9) + 1e-300).all()) and bool(((T == 0) == (gt == 0)).all())
    # the whole per-sample bound stays a rounding bound.  On this white-noise table g = d sigma / dx cancels a hundredfold in its
    # own sum and its error enters t squared-conditioned, so the worst case is a few per cent of the gradient -- a sample that took
    # a neighbour's value would be off by the gradient itself
    tol = R.tcnn_second_order_dx_bound(x, table, cfg, wd, acts, o["grad_sigma"], c)
    assert float((tol / gx.abs().clamp_min(1e-300))[:40].median()) < 0.1 and bool((tol[40] == 0).all())
