"""tests/dwp_plan_ref.py -- the Python restatement of the GEMM work plan that the live-count GPU tests hold dwp_plan_kernel to --
against the header it restates: tests/csrc/dwp_plan_check.cpp `plans` compiles mirror_nerf_amd/csrc/mnrf_dwp.h with g++ and
prints the layout of DwpDevPlan, the job weights, dwp_sample_blocks around the tile edges and, for plans given on its command
line, T, G and the owners of every virtual job.  A few dozen seeded plans: 1..8 evaluations, both kinds, empty evaluations, a plan with nothing live, small and large
CU counts (G capped by either T / 256 or the CUs)."""
import os
import random
import subprocess

from tests import dwp_plan_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plans():
    rnd = random.Random(11)
    out = [(256, [0], [0]), (256, [0, 0, 0], [0, 1, 0]), (256, [4], [1]), (1, [4, 8], [0, 1]), (256, [2048, 516], [0, 0])]
    for it in range(43):
        n = 1 + rnd.randrange(PR.MAX_EVAL)
        n_sb, kinds = [], []
        for _ in range(n):
            c = rnd.randrange(4)
            n_sb.append(0 if c == 0 else 4 * (1 + rnd.randrange(3)) if c == 1 else 4 * rnd.randrange(600) if c == 2 else 4 * rnd.randrange(60000))
            kinds.append(int(rnd.randrange(3) == 0))
        out.append(((256, 304, 1, 64)[it % 4], n_sb, kinds))
    return out


def test_plan_restatement_matches_the_header(tmp_path):
    exe = tmp_path / "dwp_plan_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "mirror_nerf_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csrc", "dwp_plan_check.cpp"), "-o", str(exe)], check=True)
    plans = _plans()
    args = ["plans"]
    for cus, n_sb, kinds in plans:
        args += [str(cus), str(len(n_sb))]
        for a, b in zip(n_sb, kinds):
            args += [str(a), str(b)]
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 3 + len(plans)
    lay = lines[0].split()
    assert lay[0] == "layout"
    lay = dict(zip(lay[1::2], map(int, lay[2::2])))
    assert lay.pop("sizeof") == PR.SIZEOF and lay.pop("floats") == PR.DEVPLAN_FLOATS
    assert lay.pop("jobs") == PR.JOBS and lay.pop("max_eval") == PR.MAX_EVAL
    assert lay == PR.OFFSETS
    w = lines[1].split()
    assert w[0] == "weights" and tuple(map(int, w[1:])) == PR.WEIGHTS and max(PR.WEIGHTS) == PR.MAX_WEIGHT
    sb = lines[2].split()      # dwp_sample_blocks itself, around the tile edges: what live_blocks builds on
    assert sb[0] == "sample_blocks" and len(sb) > 30
    for B, blocks in zip(map(int, sb[1::2]), map(int, sb[2::2])):
        assert PR.sample_blocks(B) == blocks, (B, blocks)
        assert PR.live_blocks(B, 1, B + 1000) == blocks and PR.live_blocks(B + 5, 1, B) == blocks and PR.live_blocks(None, 1, B) == blocks
        if B % 64 == 0:
            assert PR.live_blocks(B // 64, 64, B + 1000) == blocks
    empty = 0
    for (cus, n_sb, kinds), line in zip(plans, lines[3:]):
        t = line.split()
        assert t[0] == "plan" and t[1] == "T" and t[3] == "G" and t[5] == "owners"
        own = list(map(int, t[6:]))
        p = PR.plan(n_sb, kinds, cus)
        assert (p["T"], p["G"]) == (int(t[2]), int(t[4])), (n_sb, kinds, cus)
        assert p["g_lo"] == own[0::2] and p["g_hi"] == own[1::2], (n_sb, kinds, cus)
        assert len(own) == 2 * PR.JOBS * len(n_sb)
        empty += sum(1 for lo, hi in zip(p["g_lo"], p["g_hi"]) if lo > hi)
    assert empty > 100      # virtual jobs without stages (an empty evaluation, a head job of kind 1) are among the cases


def test_live_blocks_closed_form():
    """n_sb = min(4 ceil(live spr / 128), capacity blocks): whole tiles, the clamps at zero and at the capacity."""
    assert [PR.live_blocks(v, 1, 513) for v in (0, 1, 128, 129, 512, 513, 600, -3, None)] == [0, 4, 4, 8, 16, 20, 20, 0, 20]
    assert [PR.live_blocks(v, 64, 9 * 64) for v in (1, 2, 3, 8, 9)] == [4, 4, 8, 16, 20]
    assert [PR.live_blocks(v, 192, 5 * 192) for v in (1, 2, 3)] == [8, 12, 20]


def test_parse_reads_what_the_layout_says():
    import struct
    p = PR.plan([4, 0, 12], [0, 1, 1], 256)
    blk = bytearray(PR.DEVPLAN_FLOATS * 4)
    struct.pack_into("<i8i8ii", blk, 0, 3, *(p["n_sb"] + [0] * 5), *(p["kind"] + [0] * 5), p["G"])
    struct.pack_into("<q", blk, PR.OFFSETS["T"], p["T"])
    struct.pack_into(f"<{len(p['g_lo'])}h", blk, PR.OFFSETS["g_lo"], *p["g_lo"])
    struct.pack_into(f"<{len(p['g_hi'])}h", blk, PR.OFFSETS["g_hi"], *p["g_hi"])
    q = PR.parse(bytes(blk))
    assert q["n_eval"] == 3 and q["n_sb"][:3] == p["n_sb"] and q["kind"][:3] == p["kind"]
    assert (q["T"], q["G"], q["g_lo"], q["g_hi"]) == (p["T"], p["G"], p["g_lo"], p["g_hi"])
