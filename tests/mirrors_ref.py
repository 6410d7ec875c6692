"""A numpy float32 restatement of mnrf_place_mirrors (csrc/mnrf_mirrors.hip), written from THE RULE in include/mnrf.h
(DESIGN 4.5c): every step is one IEEE float32 operation in the documented order -- the kernel is compiled without
contraction, with correctly rounded division and square root -- so this is what the kernel must return bit for bit
(tests/test_hip_mirrors.py).  The axis kind repeats the expressions of tests/apps_ref.py place_mirror, which
tests/test_mirrors_cpu.py holds it to.

A mirror is the dict PlacedMirror.as_dict() gives (or `axis` / `frame` below): every number is the C float the entry point
receives."""
import numpy as np

from tests import apps_ref as AR

F = np.float32


def axis(axis, position, normal, rect, shape="rect"):
    """axis: AR.PLANE_X / AR.PLANE_Y or "x" / "y"."""
    a = {AR.PLANE_X: "x", AR.PLANE_Y: "y"}.get(axis, axis)
    assert a in ("x", "y")
    return dict(kind="axis", shape=shape, axis=a, position=float(F(position)), normal=tuple(float(F(v)) for v in normal),
                rect=tuple(float(F(v)) for v in rect), center=(0.0,) * 3, e_u=(0.0,) * 3, e_w=(0.0,) * 3)


def frame(center, normal, e_u, e_w, rect, shape="rect"):
    """The frame as given (rounded to float32): nothing is normalised here."""
    t = lambda v: tuple(float(F(x)) for x in v)  # noqa: E731
    return dict(kind="frame", shape=shape, axis=None, position=None, center=t(center), normal=t(normal), e_u=t(e_u), e_w=t(e_w), rect=t(rect))


def intersect(rays, m):
    """Mirror m on the rays -> dict(x (n,3), u, w, inside, dist, s), float32."""
    rays = np.asarray(rays, F)
    o, d = [rays[:, j] for j in range(3)], [rays[:, 3 + j] for j in range(3)]
    r0, r1, r2, r3 = (F(v) for v in m["rect"])
    with np.errstate(all="ignore"):
        if m["kind"] == "axis":
            a = 1 if m["axis"] == "y" else 0
            b = 1 - a
            pos = F(m["position"])
            t = (pos - o[a]) / d[a]
            u = t * d[b] + o[b]
            w = t * d[2] + o[2]
            x = [None, None, w]
            x[a], x[b] = np.full_like(u, pos), u
        else:
            c, n = [F(v) for v in m["center"]], [F(v) for v in m["normal"]]
            eu, ew = [F(v) for v in m["e_u"]], [F(v) for v in m["e_w"]]
            e = [c[j] - o[j] for j in range(3)]
            num = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]
            den = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]
            t = num / den
            x = [t * d[j] + o[j] for j in range(3)]
            r = [x[j] - c[j] for j in range(3)]
            u = (eu[0] * r[0] + eu[1] * r[1]) + eu[2] * r[2]
            w = (ew[0] * r[0] + ew[1] * r[1]) + ew[2] * r[2]
        if m["shape"] == "ellipse":
            uc, ru = (r0 + r1) * F(0.5), (r1 - r0) * F(0.5)
            wc, rw = (r2 + r3) * F(0.5), (r3 - r2) * F(0.5)
            a_, b_ = (u - uc) / ru, (w - wc) / rw
            q = a_ * a_ + b_ * b_
            inside = ~(q > F(1.0))
        else:
            q = None
            inside = ~((u < r0) | (w < r2) | (u > r1) | (w > r3))
        e = [o[j] - x[j] for j in range(3)]
        dist = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        f = [x[j] - o[j] for j in range(3)]
        s = (f[0] * d[0] + f[1] * d[1]) + f[2] * d[2]
    out = dict(x=np.stack(x, 1).astype(F), u=u.astype(F), w=w.astype(F), inside=inside, dist=dist.astype(F), s=s.astype(F))
    if q is not None:
        out["q"] = q.astype(F)
    return out


def place_mirrors(rays, depth, mask, normal, x_surface, mirrors, near, any_in=0):
    """-> dict: the edited copies `depth`, `mask`, `normal`, `x_surface`, the byte mask `mask_bool`, `index` (int32, the mirror
    each ray took or -1), the flag `any`, and what decided, per mirror: `per` = [dict(x, u, w, inside, dist, s, blocked, hit)]."""
    assert 1 <= len(mirrors) <= 8
    rays = np.asarray(rays, F)
    depth, mask = np.array(depth, F), np.array(mask, F)
    normal, x_surface = np.array(normal, F), np.array(x_surface, F)
    n = rays.shape[0]
    depth0, near = depth.copy(), F(near)
    best = np.full(n, -1, np.int32)
    best_dist = np.zeros(n, F)
    best_x = np.zeros((n, 3), F)
    per = []
    for k, m in enumerate(mirrors):
        p = intersect(rays, m)
        with np.errstate(all="ignore"):
            p["blocked"] = (p["dist"] > depth0) & (depth0 > near)
            p["hit"] = p["inside"] & (p["s"] > 0) & ~p["blocked"]
            take = p["hit"] & ((best < 0) | (p["dist"] <= best_dist))
        best[take] = k
        best_dist[take] = p["dist"][take]
        best_x[take] = p["x"][take]
        per.append(p)
    won = best >= 0
    x_surface[won] = best_x[won]
    depth[won] = best_dist[won]
    for k, m in enumerate(mirrors):
        normal[best == k] = np.array(m["normal"], F)
    merged = (mask != 0) | won
    return dict(depth=depth, mask=merged.astype(F), normal=normal, x_surface=x_surface, mask_bool=merged.astype(np.uint8), index=best,
                any=int(any_in) | int(merged.any()), per=per)
