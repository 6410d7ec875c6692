"""Shared case tables of the hash-grid field tests (tests/test_hip_tcnn_fp64.py on the GPU, tests/test_tcnn_ref_cpu.py for the
references and the clouds alone): sample counts at the kernels' block, group, tile and persistent-grid edges, table
configurations that reach every level kind and every accumulation kind of csrc/mnrf_tcnn.hip, and seeded position clouds.
Everything is built on the CPU in float32, so both files see the same numbers.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

from oracle import mirror_nerf_oracle as O

# forward: the VALU kernel's 512-thread block, the matrix-pipe kernel's 16-sample groups and 256-sample tiles
FWD_B = (1, 15, 16, 17, 255, 256, 257, 511, 512, 513)
# backward: the 64-lane run aggregation and the 256-sample tiles
BWD_B = (1, 63, 64, 65, 255, 256, 257)
# one tile more than the persistent grids hold, plus a ragged tail: some workgroup takes a second tile
WRAP_FWD = 512 * 256 + 77      # tcnn_mfma_kernel: min(n_tiles, 512) workgroups
WRAP_BWD = 256 * 256 + 77      # tcnn_bwd_kernel / tcnn_bwd2_kernel: min(ntiles, 256)
WRAP_FX = 2048 * 256 + 77      # tcnn_scatter_fx_kernel: min(nt, 2048)
TRAIN_B = 196608               # 1024 rays x 192 samples: the training step's fine pass
FX_SMALL_B = 7968              # the size test_tcnn_fixed_point_table_gradient runs at

# (rays, samples per ray) of the level-major encoding launch: thread map of tcnn_encode_kernel
ENCODE_SHAPES = ((32, 8),      # one patch of 32 rays x 8 depths
                 (256, 8),     # 8 blocks: patch map and the XCD permutation
                 (64, 24),     # 6 blocks: patch map, flat block order
                 (33, 8),      # rays % 32 != 0: the flat fallback
                 (32, 12),     # spr % 8 != 0: the flat fallback
                 (256, 48),    # the shape tests/test_hip_tcnn.py runs
                 (36, 16))     # rays % 32 != 0 although the sample count is a multiple of 32 (and of 8 * 32): still the flat
                               # fallback -- the patch map would need 4 blocks where the launch has 3

TABLES = ("std", "small", "mid", "odd")
ODD_ENTRIES = 8 * 1999         # a hashed level that is no power of two: the integer modulo (mode 2)


def table_config(name, bound=1.0):
    """The hash-grid geometry `name`: dict like hashgrid_config's (offsets, S, H, n_levels, level_dim, bound)."""
    log2 = {"std": 19, "small": 14, "mid": 17, "odd": 14}[name]
    cfg = O.hashgrid_config(bound, log2_hashmap_size=log2)
    if name == "odd":
        sizes = np.diff(cfg["offsets"])
        sizes = np.where(sizes == 2 ** log2, ODD_ENTRIES, sizes)
        cfg["offsets"] = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return cfg


def level_facts(cfg):
    """Per level what the launchers of csrc/mnrf_tcnn.hip derive (level_modes, plan_copies): dicts with scale (the fp32 value as a
    Python float), res, off0, hsize, mode (0 dense, 1 hashed with a mask, 2 hashed with a modulo) and copies (32, 8 or 0)."""
    out = []
    for lv in range(cfg["n_levels"]):
        scale = np.float32(np.exp2(np.float64(lv) * np.float64(cfg["S"])) * np.float64(cfg["H"]) - 1.0)
        res = int(np.ceil(scale)) + 1
        off0, off1 = int(cfg["offsets"][lv]), int(cfg["offsets"][lv + 1])
        hsize = off1 - off0
        dense = (res + 1) ** 3 <= hsize
        mode = 0 if dense else (1 if hsize & (hsize - 1) == 0 else 2)
        copies = 32 if hsize <= 32768 else (8 if hsize <= 262144 else 0)
        out.append(dict(scale=float(scale), res=res, off0=off0, hsize=hsize, mode=mode, copies=copies))
    return out


def gen(*key):
    """A generator seeded by the case: the same key gives the same numbers in every test and on every machine."""
    seed = 0
    for k in key:
        for ch in str(k):
            seed = (seed * 131 + ord(ch)) % 2147483629
    return torch.Generator().manual_seed(seed)


def pos32(x, bound, scale):
    """The kernels' own cell coordinate, operation by operation in fp32: u = (x + bound) / (2 bound), pos = u * scale + 0.5
    (two roundings: the library is built without contraction).  x: fp32 tensor; returns (u, pos)."""
    b = torch.tensor(bound, dtype=torch.float32)
    u = (x.float() + b) / torch.full_like(x.float(), 2.0 * bound)
    return u, u * torch.tensor(scale, dtype=torch.float32) + 0.5


# seeds of the `random` clouds: chosen once so that the conditioning mask stays under its cap (tests/test_tcnn_ref_cpu.py asserts it)
RANDOM_SEED = 0


def directions(B, *key):
    return torch.nn.functional.normalize(torch.randn(B, 3, generator=gen("dir", B, *key)), dim=-1)


def random_cloud(B, bound, seed=RANDOM_SEED):
    """Uniform in the open box."""
    return ((torch.rand(B, 3, generator=gen("random", B, bound, seed)) * 2 - 1) * (bound * 0.999)).float()


def _cell_face_coordinate(n, bound, scale0):
    """An fp32 x whose fp32 pos at level 0 is exactly the integer n (searched among the neighbours of the real solution)."""
    x = np.float32((n - 0.5) / scale0 * 2.0 * bound - bound)
    cand = [x]
    for _ in range(8):
        cand = [np.nextafter(cand[0], np.float32(-np.inf))] + cand + [np.nextafter(cand[-1], np.float32(np.inf))]
    c = torch.tensor(np.array(cand, dtype=np.float32))
    pos = pos32(c, bound, scale0)[1]
    hit = (pos == float(n)).nonzero()
    return float(c[int(hit[len(hit) // 2])]) if len(hit) else float(x)


def edges_cloud(bound, cfg):
    """Exact faces, edges, corners and the centre of the box (27 points of {-bound, 0, bound}^3); one float past each of the six
    faces; points whose level-0 pos is an integer on all three axes (15) and on one axis (45).  Returns (xyz, parts): parts maps
    a name to the slice of its rows."""
    g = gen("edges", bound)
    scale0 = level_facts(cfg)[0]["scale"]
    b32 = np.float32(bound)
    rows, parts = [], {}
    box = [[sx * bound, sy * bound, sz * bound] for sx in (-1, 0, 1) for sy in (-1, 0, 1) for sz in (-1, 0, 1)]
    parts["box"] = slice(0, 27)
    rows += box
    past = []
    for a in range(3):
        for sgn in (-1.0, 1.0):
            p = ((torch.rand(3, generator=g) * 2 - 1) * 0.9 * bound).tolist()
            p[a] = sgn * float(np.nextafter(b32, np.float32(np.inf)))
            past.append(p)
    parts["past"] = slice(27, 33)
    rows += past
    n_cells = int(round(scale0))
    coords = [_cell_face_coordinate(n, bound, scale0) for n in range(1, n_cells + 1)]
    face3 = [[c, c, c] for c in coords]
    parts["face3"] = slice(33, 33 + len(face3))
    rows += face3
    face1 = []
    for a in range(3):
        for c in coords:
            p = ((torch.rand(3, generator=g) * 2 - 1) * 0.9 * bound).tolist()
            p[a] = c
            face1.append(p)
    parts["face1"] = slice(33 + len(face3), 33 + len(face3) + len(face1))
    rows += face1
    return torch.tensor(rows, dtype=torch.float32), parts


ONE_CELL_LEVEL = 8


def one_cell_cloud(bound, cfg, n=256):
    """n samples strictly inside ONE cell of level 8 near the middle of the box: every wave of the backward is one run there."""
    g = gen("one_cell", bound, n)
    scale = level_facts(cfg)[ONE_CELL_LEVEL]["scale"]
    cell = torch.tensor([int(scale * 0.5) + 1, int(scale * 0.5) - 2, int(scale * 0.5) + 3], dtype=torch.float64)
    pos = cell + 0.1 + 0.8 * torch.rand(n, 3, generator=g, dtype=torch.float64)
    return (((pos - 0.5) / scale) * 2.0 * bound - bound).float()


RUN_LENGTHS = (63, 1, 64, 2, 65, 61, 128, 1, 31)      # lanes 0-62 | 63 | 64-127 (ends on a wave boundary) | 128-129 | 130-194 (crosses
                                                     # one) | 195-255 | 256-383 (two whole waves) | 384 | 385-415 (ragged tile)


def runs_cloud(bound, cfg):
    """Samples in the order a ray would give them whose runs of equal level-0 cells have the lengths RUN_LENGTHS: consecutive runs
    sit in neighbouring cells along x, the samples of a run are spread inside their cell."""
    g = gen("runs", bound)
    scale = level_facts(cfg)[0]["scale"]
    rows = []
    for k, n in enumerate(RUN_LENGTHS):
        cell = torch.tensor([2 + k, 7, 5], dtype=torch.float64)
        pos = cell + 0.05 + 0.9 * torch.rand(n, 3, generator=g, dtype=torch.float64)
        pos[:, 0] = cell[0] + 0.05 + 0.9 * torch.sort(torch.rand(n, generator=g, dtype=torch.float64))[0]
        rows.append(((pos - 0.5) / scale) * 2.0 * bound - bound)
    return torch.cat(rows).float()


def all_out_cloud(bound):
    """768 samples = three 256-sample tiles: inside, wholly outside the box, inside.  Returns (xyz, keep): keep selects the 512
    samples of the cloud without the outside tile."""
    g = gen("all_out", bound)
    x = ((torch.rand(768, 3, generator=g) * 2 - 1) * 0.95 * bound).float()
    out = x[256:512]
    axis = torch.randint(0, 3, (256,), generator=g)
    sign = torch.where(torch.rand(256, generator=g) < 0.5, -1.0, 1.0)
    out[torch.arange(256), axis] = sign * bound * (1.05 + torch.rand(256, generator=g))
    keep = torch.ones(768, dtype=torch.bool)
    keep[256:512] = False
    return x, keep


def ray_cloud(n_rays, spr, bound, *key):
    """Rays (n, 8) that cross the box and depths (n, spr) along them, some samples in front of and behind the box."""
    g = gen("rays", n_rays, spr, bound, *key)
    o = (torch.rand(n_rays, 3, generator=g) * 2 - 1) * 0.3 * bound
    d = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1)
    rays = torch.cat([o - 1.2 * bound * d, d, torch.zeros(n_rays, 1), torch.full((n_rays, 1), 2.4 * bound)], 1).float()
    z = torch.linspace(0.0, 2.4 * bound, spr)[None] + (2.4 * bound / max(spr, 1)) * 0.5 * torch.rand(n_rays, spr, generator=g)
    return rays.contiguous(), z.float().contiguous()


def cotangents(B, *key, zero_every=7):
    """dL/d(sigma, rgb, pred_normal, is_mirror): normal deviates with exact zeros on every `zero_every`-th sample of sigma and rgb."""
    g = gen("cot", B, *key)
    c = dict(sigma=torch.randn(B, generator=g), rgb=torch.randn(B, 3, generator=g), pred_normal=torch.randn(B, 3, generator=g),
             is_mirror=torch.randn(B, generator=g))
    c["sigma"][::zero_every] = 0.0
    c["rgb"][1::zero_every] = 0.0
    return c
