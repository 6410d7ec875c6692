"""The work plan of the plane-fed weight-gradient GEMM restated in Python from the closed forms of
mirror_nerf_amd/csrc/mnrf_dwp.h: what dwp_plan_kernel must leave in the DwpDevPlan block at the head of mnrf_dw_planes2_n's
workspace for given live row counts.  Held to the header itself on the CPU (tests/test_dwp_plan_ref_cpu.py compares it with
tests/csrc/dwp_plan_check.cpp `plans`, which compiles the header), read by tests/test_hip_field_live_fp64.py.  No GPU needed."""
import struct

JOBS = 17                # DWP_JOBS
MAX_EVAL = 8             # DWP_MAX_EVAL
MAX_WEIGHT = 64          # DWP_MAX_WEIGHT
# dwp_weight(j) = 2 * (na + nx) of dwp_job(j): L1 (16 + 4), L2..L4, L5 hidden, L5 encoding (16 + 4), L6..L8, final, normal | mirror .0,
# dir_encoding final columns (8 + 16), its view columns (8 + 2), sigma (1 + 16), rgb / normal_net.1 / is_mirror_net.2 (1 + 8)
WEIGHTS = (40, 64, 64, 64, 64, 40, 64, 64, 64, 64, 64, 48, 20, 34, 18, 18, 18)

# struct DwpDevPlan { struct DwpPlan { int n_eval; int n_sb[8]; int kind[8]; int G; long long T; } plan; short g_lo[136], g_hi[136]; }
OFFSETS = dict(n_eval=0, n_sb=4, kind=36, G=68, T=72, g_lo=80, g_hi=80 + 2 * JOBS * MAX_EVAL)
SIZEOF = 80 + 4 * JOBS * MAX_EVAL
DEVPLAN_FLOATS = (SIZEOF + 15) // 16 * 4      # DWP_DEVPLAN_FLOATS: the block's room at the head of the workspace


def has(kind, j):
    """dwp_has: an evaluation of kind 1 (second-order planes) has the trunk jobs and sigma only."""
    return kind == 0 or j <= 8 or j == 13


def sample_blocks(samples):
    """dwp_sample_blocks: planes are written by whole 128-sample tiles of four 32-sample blocks."""
    return 4 * ((samples + 127) // 128)


def live_blocks(live, spr, capacity_samples):
    """n_sb of an evaluation: min(4 ceil(live spr / 128), capacity blocks); live None = the capacity, a negative count = 0."""
    cap = sample_blocks(capacity_samples)
    if live is None:
        return cap
    return min(sample_blocks(max(live, 0) * spr), cap)


def stages(n_sb, kinds, j, e):
    return n_sb[e] if has(kinds[e], j) else 0


def total(n_sb, kinds):
    return sum(stages(n_sb, kinds, j, e) * WEIGHTS[j] for j in range(JOBS) for e in range(len(n_sb)))


def pick_G(T, cus):
    return min(max(T // (4 * MAX_WEIGHT), 1), cus)


def owner(c, T, G):
    """dwp_owner: the g with floor(g T / G) <= c < floor((g + 1) T / G)."""
    return ((c + 1) * G - 1) // T


def plan(n_sb, kinds, cus):
    """dict(n_eval, n_sb, kind, T, G, g_lo, g_hi): virtual job v = j * n_eval + e; (1, 0) where it has no stages."""
    n_eval = len(n_sb)
    kinds = [1 if k else 0 for k in kinds]
    T = total(n_sb, kinds)
    G = pick_G(T, cus)
    lo, hi, P = [], [], 0
    for j in range(JOBS):
        for e in range(n_eval):
            n = stages(n_sb, kinds, j, e)
            if n > 0:
                lo.append(owner(P, T, G))
                hi.append(owner(P + (n - 1) * WEIGHTS[j], T, G))
            else:
                lo.append(1)
                hi.append(0)
            P += n * WEIGHTS[j]
    assert P == T
    return dict(n_eval=n_eval, n_sb=list(n_sb), kind=kinds, T=T, G=G, g_lo=lo, g_hi=hi)


def parse(block):
    """The fields of a DwpDevPlan block (bytes, at least SIZEOF of them) as plan() names them; n_sb / kind over all MAX_EVAL
    entries, g_lo / g_hi over the JOBS * n_eval virtual jobs."""
    assert len(block) >= SIZEOF
    n_eval = struct.unpack_from("<i", block, OFFSETS["n_eval"])[0]
    nv = JOBS * max(0, min(n_eval, MAX_EVAL))
    return dict(n_eval=n_eval, n_sb=list(struct.unpack_from(f"<{MAX_EVAL}i", block, OFFSETS["n_sb"])),
                kind=list(struct.unpack_from(f"<{MAX_EVAL}i", block, OFFSETS["kind"])),
                G=struct.unpack_from("<i", block, OFFSETS["G"])[0], T=struct.unpack_from("<q", block, OFFSETS["T"])[0],
                g_lo=list(struct.unpack_from(f"<{nv}h", block, OFFSETS["g_lo"])),
                g_hi=list(struct.unpack_from(f"<{nv}h", block, OFFSETS["g_hi"])))
