"""Seeded synthetic inputs of the per-ray kernel tests (tests/test_hip_rays_fp64.py on the GPU, tests/test_torch_ref_cpu.py for
the references alone).  Everything is built on the CPU in float32 from a torch.Generator, so both files see the same numbers.
TEST INFRASTRUCTURE ONLY."""
import torch

COMPOSITE_S = (1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
COMPOSITE_REGIMES = ("thin", "opaque_inside", "opaque_straddle", "opaque_first", "opaque_last", "opaque_two", "empty",
                     "empty_zero", "last_only", "duplicate", "noise")
# (S, n_importance): totals 4, 64, 65, 128, 129, 192, 256, 257 and 512
RESAMPLE_SHAPES = ((3, 1), (3, 61), (4, 60), (5, 60), (64, 64), (64, 65), (64, 128), (128, 128), (128, 129), (255, 1), (256, 256))
RESAMPLE_REGIMES = ("uniform", "zero", "hot_1", "hot_S-2", "hot_0", "hot_S-1", "pow8")


def gen(*key):
    """A generator seeded by the case: the same key gives the same numbers in every test and on every machine."""
    seed = 0
    for k in key:
        for ch in str(k):
            seed = (seed * 131 + ord(ch)) % 2147483629
    return torch.Generator().manual_seed(seed)


def opaque_runs(S, regime, ray):
    """[(start, length)] of the opaque runs of a ray: 1 to 8 samples whose alpha is exactly 1.  `opaque_first` keeps to 3 samples:
    behind k opaque samples everything is of the order 1e-10^k, and with the run in front the WHOLE row of a gradient is; float32
    holds 1e-30 to full precision but not 1e-40, so a longer run would leave a row with nothing to compare.  `opaque_two`
    reaches the denormals (1e-40 and below) behind its second run, where the row still has its entries in front."""
    if regime == "opaque_inside":
        runs = [(min(10, S // 2), 1 + ray % 8)]
    elif regime == "opaque_straddle":       # S > 64: covers samples 63 and 64
        runs = [(62 - ray % 3, 3 + ray % 3 + ray % 4)]
    elif regime == "opaque_first":
        runs = [(0, 1 + ray % 3)]
    elif regime == "opaque_last":
        n = 1 + ray % 8
        runs = [(max(S - n, 0), n)]
    elif regime == "opaque_two":
        runs = [(S // 4, 2 + ray % 4), (max(3 * S // 4, S // 4 + 6), 2 + (ray // 2) % 4)]
    else:
        return []
    return [(a, min(n, S - a)) for a, n in runs if a < S]


def composite_inputs(S, N, regime, seed=0):
    """rays (N,8), z (N,S) sorted in [0.1, 6], sigma, noise (or None), rgb, m, pn, nrm: float32 CPU tensors."""
    g = gen("composite", S, N, regime, seed)
    r = lambda *s: torch.rand(*s, generator=g)          # noqa: E731
    rn = lambda *s: torch.randn(*s, generator=g)        # noqa: E731
    rays = rn(N, 8)
    out = dict(rays=rays, rgb=r(N, S, 3), m=r(N, S), pn=_l2n(rn(N, S, 3)), nrm=_l2n(rn(N, S, 3)), noise=None)
    if regime.startswith("opaque"):
        # steps of 0.1..1 units, 2 units behind every opaque sample, scaled to span [0.1, 6]: at S = 256 an opaque sample's
        # step is at least 5.9 * 2 / (255 + 16 * 2) = 0.04, so a sigma of at most 2000 reaches sigma * delta >= 40 there
        raw = (r(N, max(S - 1, 1)) * 0.9 + 0.1).double()
        for i in range(N):
            for a, n in opaque_runs(S, regime, i):
                raw[i, a:min(a + n, S - 1)] = 2.0
        z = 0.1 + 5.9 * torch.cat([torch.zeros(N, 1, dtype=torch.float64), torch.cumsum(raw, 1) / raw.sum(1, keepdim=True)], 1)
        z = z[:, :S].float()
    else:
        z = torch.sort(r(N, S) * 5.9 + 0.1, 1)[0]
    sigma = rn(N, S) * 3
    if regime == "thin":
        out["noise"] = rn(N, S) * 0.3
    elif regime == "noise":
        out["noise"] = rn(N, S) * 3          # flips the sign of sigma + noise on about half of the samples
    elif regime == "empty":
        sigma = -r(N, S) * 3
        out["noise"] = r(N, S) * (-sigma)    # 0 <= noise <= -sigma: the sum is never positive
        sigma[:, ::3] = 0.0
        out["noise"][:, ::3] = 0.0           # and exactly 0 on every third sample
    elif regime == "empty_zero":
        sigma = torch.zeros(N, S)
    elif regime == "last_only":
        sigma = -sigma.abs()
        sigma[0::2, S - 1] = 1e-12           # delta is 1e10 there: alpha = 1 - exp(-0.01)
        sigma[1::2, S - 1] = 1e-6            # alpha = 1 - exp(-1e4) = 1
    elif regime == "duplicate":
        for a in range(0, S - 1, 4):
            z[:, a + 1] = z[:, a]            # delta = 0, as a merge of coarse and fine depths produces
    elif regime.startswith("opaque"):
        delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full((N, 1), 1e10)], 1)
        for i in range(N):
            for a, n in opaque_runs(S, regime, i):
                lo = torch.clamp(40.0 / delta[i, a:a + n], min=50.0)
                assert float(lo.max()) <= 2000.0
                sigma[i, a:a + n] = lo + r(n) * (2000.0 - lo)
                # alpha is exactly 1 in float32 AND in float64 (exp(-40) = 4e-18 is below half an ulp of 1 in both)
                assert bool((delta[i, a:a + n].double() * sigma[i, a:a + n].double() >= 39.99).all())
    out.update(z=z, sigma=sigma)
    return out


def _l2n(x):
    return x / x.norm(dim=-1, keepdim=True)


def resample_inputs(S, n_imp, N, regime, per_ray, seed=0):
    """z (N,S) sorted, weights (N,S) and u ((n_imp,) shared linspace or (N, n_imp) uniform): float32 CPU tensors."""
    g = gen("resample", S, n_imp, N, regime, per_ray, seed)
    z = torch.sort(torch.rand(N, S, generator=g) * 5.9 + 0.1, 1)[0]
    w = torch.zeros(N, S)
    if regime == "uniform":
        w = torch.rand(N, S, generator=g) * 0.5 + 0.5
    elif regime == "pow8":
        w = torch.rand(N, S, generator=g) ** 8
    elif regime.startswith("hot_"):
        w[:, {"hot_1": 1, "hot_S-2": S - 2, "hot_0": 0, "hot_S-1": S - 1}[regime]] = 1.0
    u = torch.rand(N, n_imp, generator=g) if per_ray else torch.linspace(0, 1, n_imp)
    return z, w, u


def resample_undecided(cdf64, u64, raw64, per_ray, eps=1e-5, tol=1e-6):
    """(N, n_imp) bool: the samples whose value the float64 reference alone cannot decide -- u within `tol` of an entry of the
    cdf, the selected bin's c1 - c0 within `tol` of eps (where the denominator switches to 1), and the u = 1.0 that ends the
    shared linspace.  Two refinements, both of which leave FEWER samples aside:
      - entry 0 of the cdf is the constant 0 in every arithmetic, and u = 0 gives b0 + (0 - 0) / denom * (b1 - b0) = the first
        mid-point whatever the cdf and the denominator are: always decided;
      - where the two bins that meet at the entry both have c1 - c0 >= eps + tol the inverse cdf is continuous across the
        entry: the end of one bin and the start of the next are the same depth, so the value is decided although the bin is
        not.  (S = 64 with 65 shared u and equal weights has u = 0.5 = cdf[31] by construction; set aside with the u = 1.0
        that would be 2 of 65 samples, past the 2 % cap, in three weight regimes.)  Only an entry next to a switched
        denominator leaves the value open."""
    width = cdf64[:, 1:] - cdf64[:, :-1]                                    # width[k] = cdf[k+1] - cdf[k], k = 0..nw-1
    steep = width < eps + tol
    beside = steep.clone()                                                 # entry k (1..nw): bins k-1 and k
    beside[:, :-1] |= steep[:, 1:]
    near = (((u64[:, :, None] - cdf64[:, None, 1:]).abs() <= tol) & beside[:, None, :]).any(-1)
    sw = (raw64 - eps).abs() <= tol
    last = torch.zeros_like(near)
    if not per_ray:
        last = u64 >= 1.0
    return (near | sw | last) & (u64 > 0)


def resample_slope(raw64, span64, eps=1e-5):
    """(N, n_imp): d sample / d cdf of the selected bin, (b1 - b0) / denom -- what an error of the cdf is multiplied by."""
    return span64.abs() / torch.where(raw64 < eps, torch.ones_like(raw64), raw64)
