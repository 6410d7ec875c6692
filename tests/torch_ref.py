"""Plain-torch restatements of the floating-point kernels that have a backward pass (field MLP, compositing) and of
the per-ray kernels around them (resampling, reflection, blend, ray gradients), in the dtype of their inputs (fp32, or float64 with the kernel's own
activation masks: `field(..., masks=)`).  TEST INFRASTRUCTURE ONLY: the GPU tests differentiate these with
torch.autograd to check the hand-written HIP backward kernels; the product never imports this."""
import torch


def l2n(x):
    eps = torch.tensor(torch.finfo(torch.float32).eps, device=x.device, dtype=x.dtype)
    return x / torch.sqrt(torch.maximum((x * x).sum(-1, keepdim=True), eps))


def embed(x, n):
    out = [x]
    for k in range(n):
        out += [torch.sin((2.0 ** k) * x), torch.cos((2.0 ** k) * x)]
    return torch.cat(out, -1)


# the activations of the field MLP: ReLU behind L1..L8 and dir_encoding, LeakyReLU(0.01) behind is_mirror_net.0
MASK_NAMES = tuple(f"L{i + 1}" for i in range(8)) + ("dir", "mir")


def masks_of(pre):
    """Activation masks of pre-activations (dict name -> tensor, MASK_NAMES): 1 where y > 0, else 0 (ReLU) or 0.01 (the
    LeakyReLU of is_mirror_net.0).  torch's own convention at y == 0: the gradient there is 0 (ReLU) or 0.01."""
    out = {}
    for n, y in pre.items():
        pos = y > 0
        out[n] = pos.to(y.dtype) if n != "mir" else torch.where(pos, torch.ones_like(y), torch.full_like(y, 0.01))
    return out


def field(w, xyz, dir_emb, with_normal=False, cut_normal=False, cut_mirror=False, keep_mirror=None, masks=None, acts=None,
          n_bands=10):
    """w: dict name -> tensor (reference parameter names); returns sigma (B), rgb, pred_normal, is_mirror (B)
    [, normal = l2n(-d sigma/d xyz) built with create_graph=True like utils/func.py:10-25].
    n_bands: frequency bands of the position encoding (Embedding(n_bands): 10, 6, 0 -> 63, 39, 3 input channels of
    xyz_encoding_1 / the skip; the view encoding arrives embedded, as wide as dir_encoding.0 expects).  A head whose
    parameters `w` does not hold (normal_net.*, is_mirror_net.*: predict_normal / predict_mirror_mask off,
    models/mirror_nerf.py:80-99) is absent: None stands in its place.
    cut_normal / cut_mirror / keep_mirror (B, bool): the heads see geo_feat.detach() (mirror_nerf.py:154-183).
    masks (dict MASK_NAMES -> tensor shaped like the pre-activation, held constant): every activation becomes y * mask, so
    that the function is the piecewise-linear piece a kernel's own ReLU masks select (pre-activations within rounding of 0
    then cannot flip between the kernel and this reference).  acts: a dict, filled with the pre-activations (MASK_NAMES) and
    the inputs of the Linears ("enc", "h1".."h8", "fin", "hd", "hn", "hm")."""
    if with_normal and not xyz.requires_grad:
        xyz = xyz.requires_grad_(True)
    keep = acts if acts is not None else {}

    def act(name, y):
        keep[name] = y
        if masks is not None:
            return y * masks[name]
        return torch.nn.functional.leaky_relu(y, 0.01) if name == "mir" else torch.relu(y)

    enc = embed(xyz, n_bands)
    keep["enc"] = enc
    h = enc
    for i in range(8):
        if i == 4:
            h = torch.cat([enc, h], -1)
        h = act(f"L{i + 1}", h @ w[f"xyz_encoding_{i+1}.0.weight"].T + w[f"xyz_encoding_{i+1}.0.bias"])
        keep[f"h{i + 1}"] = h
    sigma = (h @ w["sigma.weight"].T + w["sigma.bias"])[:, 0]
    fin = h @ w["xyz_encoding_final.weight"].T + w["xyz_encoding_final.bias"]
    keep["fin"] = fin
    hd = act("dir", torch.cat([fin, dir_emb], -1) @ w["dir_encoding.0.weight"].T + w["dir_encoding.0.bias"])
    keep["hd"] = hd
    rgb = torch.sigmoid(hd @ w["rgb.0.weight"].T + w["rgb.0.bias"])
    hN = h.detach() if cut_normal else h
    hM = h.detach() if cut_mirror else h
    if keep_mirror is not None and not cut_mirror:
        hM = torch.where(keep_mirror[:, None], h, h.detach())
    pn = m = None
    if "normal_net.0.weight" in w:
        hn = hN @ w["normal_net.0.weight"].T + w["normal_net.0.bias"]
        keep["hn"] = hn
        pn = l2n(hn @ w["normal_net.1.weight"].T + w["normal_net.1.bias"])
    if "is_mirror_net.0.weight" in w:
        hm = act("mir", hM @ w["is_mirror_net.0.weight"].T + w["is_mirror_net.0.bias"])
        keep["hm"] = hm
        m = torch.sigmoid(hm @ w["is_mirror_net.2.weight"].T + w["is_mirror_net.2.bias"])[:, 0]
    if with_normal:
        (grad,) = torch.autograd.grad(sigma, xyz, torch.ones_like(sigma), create_graph=True, retain_graph=True)
        return sigma, rgb, pn, m, l2n(-grad)
    return sigma, rgb, pn, m


def composite(rays, sigma, z, noise, rgb, is_mirror, pn, nrm, white_back=False, detach_mask=False, keep_mirror=None,
              detach_normal=False):
    """models/rendering.py:181-264, 362-367 on (N,S) tensors (detach_*: rendering.py:223-247)."""
    deltas = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], -1)
    sv = sigma if noise is None else sigma + noise
    alphas = 1 - torch.exp(-deltas * torch.relu(sv))
    shifted = torch.cat([torch.ones_like(alphas[:, :1]), 1 - alphas + 1e-10], -1)
    w = alphas * torch.cumprod(shifted[:, :-1], -1)
    op = w.sum(1)
    out = {"weights": w, "opacity": op}
    rgb_map = (w[..., None] * rgb).sum(1)
    if white_back:
        rgb_map = rgb_map + 1 - op[:, None]
    depth = (w * z).sum(1)
    wm = w.detach() if detach_mask else w
    if keep_mirror is not None and not detach_mask:
        wm = torch.where(keep_mirror[:, None], w, w.detach())
    wn = w.detach() if detach_normal else w
    out.update(rgb=rgb_map, depth=depth)
    if is_mirror is not None:      # (a field without the head: the map is not formed)
        out["mask"] = (wm * is_mirror).sum(1)
    if pn is not None:
        out["sn"] = (wn[..., None] * pn).sum(1)
    if nrm is not None and pn is None:
        out["sng"] = (wn[..., None] * nrm).sum(1)
    elif nrm is not None:
        out["sng"] = (wn[..., None] * nrm).sum(1)
        out["nd"] = (wn * ((nrm - pn) ** 2).sum(-1)).sum(1)
    out["xs"] = rays[:, :3] + rays[:, 3:6] * depth[:, None]
    return out


def reflect(rays, x_surface, normal, mask, compact):
    """train.py:217-252 with torch ops (reference for ReflectFn)."""
    n = l2n(normal)
    w = l2n(-rays[:, 3:6])
    cos = (w * n).sum(-1)
    rdir = 2 * cos[:, None] * n - w
    far = rays[:, 7:8]
    sec = torch.cat([x_surface, rdir, torch.ones_like(far) * 0.1, far], -1)
    if compact:
        sec = sec[mask != 0]
    return sec


def blend(base, sec, mask, compact):
    """train.py:263-296 with torch ops (reference for BlendFn)."""
    if compact:
        part = base.clone().detach()
        part[mask != 0] = sec
    else:
        part = sec
    m = mask[:, None]
    return m * part + (1 - m) * base


def sample_pdf(bins, weights, n_importance, u, eps=1e-5):
    """models/rendering.py:7-51 in the dtype of its inputs.  bins (N, S-1): the mid-points; weights (N, S-2): weights[:, 1:-1];
    u (n_importance,) shared by the rays or (N, n_importance)."""
    return sample_pdf_info(bins, weights, n_importance, u, eps)[0]


def sample_pdf_info(bins, weights, n_importance, u, eps=1e-5):
    """sample_pdf and what it decided on the way: (samples, cdf (N, S-1), u (N, n_importance), c1 - c0 before the `< eps`
    replacement, b1 - b0 of the selected bin)."""
    n_rays, n_s = weights.shape
    weights = weights + eps
    pdf = weights / weights.sum(-1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[:, :1]), cdf], -1)
    u = u.to(cdf.dtype).expand(n_rays, n_importance).contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below = torch.clamp_min(inds - 1, 0)
    above = torch.clamp_max(inds, n_s)
    c0, c1 = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    b0, b1 = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    raw = c1 - c0
    denom = torch.where(raw < eps, torch.ones_like(raw), raw)
    return b0 + (u - c0) / denom * (b1 - b0), cdf, u, raw, b1 - b0


def mids(z):
    """models/rendering.py:313-315: the interval mid-points of the depths."""
    return 0.5 * (z[:, :-1] + z[:, 1:])


def merge_sorted(z, fine):
    """models/rendering.py:324: coarse and fine depths in one sorted row."""
    return torch.sort(torch.cat([z, fine], -1), -1)[0]


def ray_grads(d_xyz, z, d_dir, spr):
    """include/mnrf.h mnrf_ray_grads: g_rays (N, 8) = [sum_s dL/dx_s | sum_s z_s dL/dx_s | 0 0] and g_de (N, 27) = the sum of the
    first 27 columns of d_dir (N * spr, 32) over each ray's samples.  d_xyz (N * spr, 3), z (N, spr)."""
    n = z.shape[0]
    g = d_xyz.reshape(n, spr, 3)
    g_rays = torch.cat([g.sum(1), (z[..., None] * g).sum(1), torch.zeros_like(g[:, 0, :2])], -1)
    g_de = d_dir.reshape(n, spr, -1)[:, :, :27].sum(1)
    return g_rays, g_de


def hashgrid_encode(x01, table, cfg):
    """Multiresolution hash encoding with torch ops (differentiable in `table` and, through the interpolation weights, in
    `x01`; twice differentiable): cells, hashing and level geometry follow the oracle (`hashgrid_encode` / `_grid_index`,
    i.e. models/gridencoder/src/gridencoder.cu:51-272), the table look-up is a gather.  x01 (B,3) fp32 in [0,1];
    table (n_entries, 2).  Returns (B, 2 * n_levels), level-major."""
    import numpy as np
    from oracle import mirror_nerf_oracle as O
    oob = ((x01 < 0) | (x01 > 1)).any(-1)
    feats = []
    for lv in range(cfg["n_levels"]):
        off0, off1 = int(cfg["offsets"][lv]), int(cfg["offsets"][lv + 1])
        scale = float(np.float32(np.exp2(np.float64(lv) * np.float64(cfg["S"])) * np.float64(cfg["H"]) - 1.0))
        res = int(np.ceil(np.float32(scale))) + 1
        pos = x01 * scale + 0.5
        pg = torch.floor(pos).detach()
        fr = (pos - pg).to(table.dtype)
        pgi = pg.cpu().numpy().astype(np.int64).clip(0).astype(np.uint32)
        acc = 0
        for c in range(8):
            wgt = 1
            loc = np.empty_like(pgi)
            for a in range(3):
                bit = (c >> a) & 1
                wgt = wgt * (fr[:, a] if bit else 1 - fr[:, a])
                loc[:, a] = pgi[:, a] + np.uint32(bit)
            idx = torch.from_numpy(O._grid_index(loc, off1 - off0, res)).to(x01.device) + off0
            acc = acc + wgt[:, None] * table[idx]
        feats.append(torch.where(oob[:, None], torch.zeros_like(acc), acc))
    return torch.cat(feats, -1)


def sh4(d):
    """Real spherical harmonics of degree 4 (16 values) of the raw direction: models/shencoder/src/shencoder.cu:49-79."""
    X, Y, Z = d[:, 0], d[:, 1], d[:, 2]
    xy, xz, yz, x2, y2, z2 = X * Y, X * Z, Y * Z, X * X, Y * Y, Z * Z
    return torch.stack([
        torch.full_like(X, 0.28209479177387814), -0.48860251190291987 * Y, 0.48860251190291987 * Z, -0.48860251190291987 * X,
        1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.94617469575755997 * z2 - 0.31539156525251999,
        -1.0925484305920792 * xz, 0.54627421529603959 * x2 - 0.54627421529603959 * y2,
        0.59004358992664352 * Y * (-3.0 * x2 + y2), 2.8906114426405538 * xy * Z, 0.45704579946446572 * Y * (1.0 - 5.0 * z2),
        0.3731763325901154 * Z * (5.0 * z2 - 3.0), 0.45704579946446572 * X * (1.0 - 5.0 * z2),
        1.4453057213202769 * Z * (x2 - y2), 0.59004358992664352 * X * (-x2 + 3.0 * y2)], -1)


def tcnn_field_with_normal(w, x6, cfg):
    """tcnn_field plus normal = l2n(-d sigma/dx) built with create_graph=True (models/mirror_nerf_tcnn.py:172-218,
    utils/func.py:10-25): torch's double backward through it is the reference for the second-order kernel."""
    if not x6.requires_grad:
        x6 = x6.requires_grad_(True)
    sigma, rgb, pn, m = tcnn_field(w, x6, cfg)
    (grad,) = torch.autograd.grad(sigma, x6, torch.ones_like(sigma), create_graph=True, retain_graph=True)
    return sigma, rgb, pn, m, l2n(-grad[:, :3])


def tcnn_field(w, x6, cfg, detach_normal=False, detach_mirror=None):
    """MirrorNeRFTcnn.forward (models/mirror_nerf_tcnn.py:220-259) with torch ops: the hash-grid cells and interpolation
    weights follow the oracle (`hashgrid_encode` / `_grid_index`), the table look-up is a differentiable gather.
    w: dict of torch tensors (state_dict names), x6 (B,6) = [xyz, raw direction].  Returns sigma (B), rgb, pred_normal,
    is_mirror (B)."""
    xyz, d = x6[:, :3], x6[:, 3:6]
    bound = cfg["bound"]
    # cell coordinates in fp32 like the kernel (a cell of the finest level is 2e-4 of the box: fp64 coordinates would
    # differ from the kernel's by 1e-4 of a cell); everything after the interpolation weights runs in the dtype of w
    xf = xyz.float()
    x01 = (xf + bound) / torch.full_like(xf, 2 * bound)     # a tensor divisor: torch turns "/ scalar" into "* (1/scalar)" on the GPU
    enc = hashgrid_encode(x01, w["encoder.embeddings"], cfg)
    h = torch.relu(enc @ w["sigma_net.0.weight"].T) @ w["sigma_net.1.weight"].T
    sigma, geo = h[:, 0], h[:, 1:]
    # the --detach_density_* options (models/mirror_nerf_tcnn.py:186-215): detach_mirror = True (all samples) or a (B,) bool
    # tensor of the samples whose mirror head sees geo_feat.detach()
    geo_n = geo.detach() if detach_normal else geo
    pn = l2n(torch.relu(geo_n @ w["normal_net.0.weight"].T) @ w["normal_net.1.weight"].T)
    sh = sh4(d)
    hc = torch.relu(torch.cat([sh, geo], -1) @ w["color_net.0.weight"].T)
    hc = torch.relu(hc @ w["color_net.1.weight"].T)
    rgb = torch.sigmoid(hc @ w["color_net.2.weight"].T)
    if detach_mirror is None:
        geo_m = geo
    elif detach_mirror is True:
        geo_m = geo.detach()
    else:
        geo_m = torch.where(detach_mirror[:, None], geo.detach(), geo)
    hm = torch.nn.functional.leaky_relu(geo_m @ w["is_mirror_net.0.weight"].T + w["is_mirror_net.0.bias"], 0.01)
    m = torch.sigmoid(hm @ w["is_mirror_net.2.weight"].T + w["is_mirror_net.2.bias"])[:, 0]
    return sigma, rgb, pn, m


# ------------------------------------------------------------------------------------------ hash-grid field, float64, any table
# The pieces below take the level offsets AS GIVEN (any sizes: dense, power-of-two hashed, any other hashed size), run on the
# device of their inputs and never leave it, so a reference over 10^5..10^6 samples takes seconds.
_PRIMES = (1, 2654435761, 805459861)


def tcnn_levels(cfg):
    """Per level: (scale as the fp32 value the launchers compute, res = ceil(scale) + 1, first entry, entries)."""
    import numpy as np
    out = []
    for lv in range(cfg["n_levels"]):
        scale = np.float32(np.exp2(np.float64(lv) * np.float64(cfg["S"])) * np.float64(cfg["H"]) - 1.0)
        out.append((float(scale), int(np.ceil(scale)) + 1, int(cfg["offsets"][lv]), int(cfg["offsets"][lv + 1] - cfg["offsets"][lv])))
    return out


def tcnn_grid_index(loc, hsize, res):
    """get_grid_index of gridencoder (gridtype hash, align_corners false) on an int64 tensor loc (..., 3) of node coordinates:
    the dense index while the running stride (a power of res + 1) still fits the level, else the 32-bit spatial hash; `% hsize`
    in either case."""
    stride, index, d = 1, torch.zeros_like(loc[..., 0]), 0
    while d < 3 and stride <= hsize:
        index = index + loc[..., d] * stride
        stride *= res + 1
        d += 1
    if stride > hsize:
        index = torch.zeros_like(loc[..., 0])
        for k in range(3):
            index = index ^ ((loc[..., k] * _PRIMES[k]) & 0xFFFFFFFF)
    return (index & 0xFFFFFFFF) % hsize


def tcnn_unit(x, bound):
    """(u64, u32, oob): the [0, 1] coordinate in float64 and in fp32, and the box test as the field takes it -- on the fp32
    coordinate u = fl((x + bound) / (2 bound)), like gridencoder's own `inputs` (x one float past +bound rounds back onto the face)."""
    xf = x.detach().float()
    u32 = (xf + torch.full_like(xf, bound)) / torch.full_like(xf, 2.0 * bound)
    oob = ((u32 < 0) | (u32 > 1)).any(-1)
    return (xf.double() + bound) / (2.0 * bound), u32, oob


def tcnn_pos(x, bound, scale, pos="f32"):
    """Cell coordinate of fp32 positions x (B, 3) at a level, float64 tensor.  pos = "f32": the value the kernels compute, operation by
    operation in fp32 (divide, multiply, add: no contraction); "f64": the same expression in float64."""
    u64, u32, _ = tcnn_unit(x, bound)
    if pos == "f64":
        return u64 * scale + 0.5
    return (u32 * torch.tensor(scale, dtype=torch.float32, device=x.device) + 0.5).double()


def _corners(p, table, off0, hsize, res):
    """Nodes and weights of the cell of p (B, 3) float64: idx (B, 8) int64 into `table`, fr (B, 3)."""
    pg = torch.floor(p)
    fr = p - pg
    pgi = pg.long().clamp_(min=0)
    bits = torch.tensor([[(c >> a) & 1 for a in range(3)] for c in range(8)], device=p.device)        # (8, 3)
    idx = tcnn_grid_index(pgi[:, None, :] + bits[None], hsize, res) + off0
    return idx, fr, bits


def tcnn_encode(x, table, cfg, pos="f32", xd=None):
    """The multiresolution encoding in the dtype of `table` (float64 for a reference): (B, 2 * n_levels), level-major; zero outside
    the box.  x (B, 3) fp32 positions.  The cell and the fractional coordinate come from tcnn_pos(pos=...).  xd: a float64 leaf
    holding the same positions: the result is then differentiable (twice) in xd through the interpolation weights, with the exact
    derivative scale / (2 bound) of pos."""
    bound = cfg["bound"]
    oob = tcnn_unit(x, bound)[2]
    feats = []
    for scale, res, off0, hsize in tcnn_levels(cfg):
        p = tcnn_pos(x, bound, scale, pos)
        idx, fr, bits = _corners(p, table, off0, hsize, res)
        fr = fr.to(table.dtype)
        if xd is not None:
            fr = fr + (xd - xd.detach()) * (scale / (2.0 * bound))
        w = torch.where(bits[None].bool(), fr[:, None, :], 1 - fr[:, None, :]).prod(-1)               # (B, 8)
        acc = (w[..., None] * table[idx]).sum(1)
        feats.append(torch.where(oob[:, None], torch.zeros_like(acc), acc))
    return torch.cat(feats, -1)


def tcnn_entry_counts(x, cfg):
    """n_e: how many (sample, corner) contributions each table entry receives from the in-box samples of x -- the number of
    adds a scatter makes to it (entries,) int64.  Cells as the kernels see them (pos = "f32")."""
    bound = cfg["bound"]
    inside = ~tcnn_unit(x, bound)[2]
    n = torch.zeros(int(cfg["offsets"][-1]), dtype=torch.int64, device=x.device)
    for scale, res, off0, hsize in tcnn_levels(cfg):
        idx, _fr, _bits = _corners(tcnn_pos(x, bound, scale), None, off0, hsize, res)
        n.index_add_(0, idx[inside].reshape(-1), torch.ones(int(inside.sum()) * 8, dtype=torch.int64, device=x.device))
    return n


def tcnn_level_sums(g_enc, x, cfg):
    """S per level of a backward pass: the sum over the in-box samples of max(|e0|, |e1|), e = dL/d encoding (B, 2 * n_levels).
    No entry of the level can collect more than S in either feature (the weights of a sample add up to 1)."""
    inside = ~tcnn_unit(x, cfg["bound"])[2]
    e = g_enc.detach().double().view(g_enc.shape[0], -1, 2).abs().amax(-1)
    return (e * inside[:, None]).sum(0)


def _ulp32(v):
    """Spacing of the fp32 numbers at |v| (float64 tensor)."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 23)


def tcnn_plane_bound(x, table, cfg):
    """Per-element rounding bound of an fp32 evaluation of the encoding planes against tcnn_encode(pos="f64"): (B, 2 * n_levels).
    pos = u * scale + 0.5 carries at most 2 ulp of fp32 error (the division in u; the multiply-add, contracted or not), and the
    interpolation itself is a three-factor weight times a value summed over eight corners (12 roundings at most):
        |d feature| <= 2 ulp32(pos) * sum_axes |d feature / d pos_axis| + 12 eps32 * sum_corners |w_c v_c|.
    Both sums are evaluated here in float64, with |.| taken corner by corner.  The interpolant is continuous but its derivative
    jumps at a cell face: where pos lies within 4 ulp of an integer on some axis the fp32 evaluation may sit in the neighbouring
    cell, so the bound is the largest over the cells that meet there (pos mirrored at the face, axis by axis)."""
    bound = cfg["bound"]
    eps = 2.0 ** -23
    oob = tcnn_unit(x, bound)[2]
    out = []
    for scale, res, off0, hsize in tcnn_levels(cfg):
        p = tcnn_pos(x, bound, scale, "f64")
        ulp = _ulp32(p).amax(-1)
        near = (p - torch.round(p)).abs() <= 4 * _ulp32(p)
        best = torch.zeros(x.shape[0], 2, dtype=torch.float64, device=x.device)
        for flip in range(8):
            fl = torch.tensor([(flip >> a) & 1 for a in range(3)], device=x.device).bool()
            sel = near & fl[None]
            if flip and not bool(sel.any()):
                continue
            q = torch.where(sel, 2 * torch.round(p) - p, p).clamp_min(0.0)
            idx, fr, bits = _corners(q, table, off0, hsize, res)
            wa = torch.where(bits[None].bool(), fr[:, None, :], 1 - fr[:, None, :])                    # (B, 8, 3)
            v = table[idx].double().abs()                                                              # (B, 8, 2)
            dsum = sum((wa[..., (a + 1) % 3] * wa[..., (a + 2) % 3])[..., None] * v for a in range(3)).sum(1)
            wsum = (wa.prod(-1)[..., None] * v).sum(1)
            best = torch.maximum(best, 2 * ulp[:, None] * dsum + 12 * eps * wsum)
        out.append(torch.where(oob[:, None], torch.zeros_like(best), best))
    return torch.cat(out, -1)


def tcnn_near_face(x, cfg, ulps=4):
    """Conditioning mask (B,) bool: at some level and axis pos lies within `ulps` ulp32(pos) of an integer -- two correct fp32
    evaluations may then sit in different cells, and everything that is a DERIVATIVE of the interpolant (density-gradient normal,
    dL/d position) differs by a jump.  Samples outside the box are never masked."""
    bound = cfg["bound"]
    near = torch.zeros(x.shape[0], dtype=torch.bool, device=x.device)
    for scale, _res, _off0, _hsize in tcnn_levels(cfg):
        p = tcnn_pos(x, bound, scale, "f64")
        near |= ((p - torch.round(p)).abs() <= ulps * _ulp32(p)).any(-1)
    return near & ~tcnn_unit(x, bound)[2]


def tcnn_heads(w, enc, d, acts=None):
    """Everything of MirrorNeRFTcnn.forward behind the encoding (models/mirror_nerf_tcnn.py:228-259), as in tcnn_field above:
    sigma (B), rgb, pred_normal, is_mirror (B), geo_feat.  acts: a dict, filled with the ReLU / LeakyReLU pre-activations."""
    keep = acts if acts is not None else {}
    keep["s0"] = enc @ w["sigma_net.0.weight"].T
    h = torch.relu(keep["s0"]) @ w["sigma_net.1.weight"].T
    keep["h16"] = h
    if h.requires_grad:
        h.retain_grad()                # dL/d (sigma, geo_feat): what tcnn_enc_grad_bound starts from
    sigma, geo = h[:, 0], h[:, 1:]
    keep["n0"] = geo @ w["normal_net.0.weight"].T
    pn = l2n(torch.relu(keep["n0"]) @ w["normal_net.1.weight"].T)
    keep["c0"] = torch.cat([sh4(d), geo], -1) @ w["color_net.0.weight"].T
    keep["c1"] = torch.relu(keep["c0"]) @ w["color_net.1.weight"].T
    rgb = torch.sigmoid(torch.relu(keep["c1"]) @ w["color_net.2.weight"].T)
    keep["m0"] = geo @ w["is_mirror_net.0.weight"].T + w["is_mirror_net.0.bias"]
    hm = torch.nn.functional.leaky_relu(keep["m0"], 0.01)
    m = torch.sigmoid(hm @ w["is_mirror_net.2.weight"].T + w["is_mirror_net.2.bias"])[:, 0]
    return sigma, rgb, pn, m, geo


def tcnn_field64(w, x, d, cfg, with_normal=False, acts=None):
    """The whole field in float64 over the fp32 positions x (B, 3) and directions d (B, 3), cells as the kernels see them.
    w: float64 tensors under the state_dict names (leaves that want gradients).  Returns a dict: sigma, rgb, pred_normal,
    is_mirror, geo_feat, enc (retains its gradient: dL/d encoding for tcnn_level_sums), xd and dd (the float64 leaves of position
    and direction) and, with_normal, normal = l2n(-d sigma / d x) built with create_graph=True."""
    xd = x.detach().double().clone().requires_grad_(True)
    dd = d.detach().double().clone().requires_grad_(True)
    enc = tcnn_encode(x, w["encoder.embeddings"], cfg, "f32", xd)
    if enc.requires_grad:
        enc.retain_grad()
    sigma, rgb, pn, m, geo = tcnn_heads(w, enc, dd, acts)
    out = dict(sigma=sigma, rgb=rgb, pred_normal=pn, is_mirror=m, geo_feat=geo, enc=enc, xd=xd, dd=dd)
    if with_normal:
        (grad,) = torch.autograd.grad(sigma, xd, torch.ones_like(sigma), create_graph=True, retain_graph=True)
        out["normal"] = l2n(-grad)
        out["grad_sigma"] = grad.detach()
    return out


def tcnn_enc_grad_bound(w, acts, g16):
    """Per-sample bound on the fp32 rounding of e = dL/d encoding = W_s0^T (mask * (W_s1^T g16)), g16 = dL/d (sigma, geo_feat) (B, 16):
    (B, 32).  Two dot products of 16 and 64 terms on top of a g16 that three heads of at most two 64-term layers each have summed
    into: (16 + 64 + 2 * 64 + 48) = 256 roundings at most on any path, each relative to the sum of the magnitudes of its terms, so
    |d e_k| <= 256 eps32 * (|W_s0|^T (mask * (|W_s1|^T |g16|)))_k -- with the sample's own g16 and mask, not a batch maximum."""
    mask = (acts["s0"].detach() > 0).to(g16.dtype)
    mag = ((g16.detach().abs() @ w["sigma_net.1.weight"].detach().abs()) * mask) @ w["sigma_net.0.weight"].detach().abs()
    return 256 * 2.0 ** -23 * mag


def tcnn_sigma_enc_grad(w, acts):
    """(q, dq): q = d sigma / d encoding = W_s0^T (mask * W_s1[0]) per sample (B, 32) in float64, and the bound of its fp32 rounding,
    64 eps32 * |W_s0|^T (mask * |W_s1[0]|) (one 64-term dot product; the mask selects exactly)."""
    mask = (acts["s0"].detach() > 0).double()
    w0, w1 = w["sigma_net.0.weight"].detach().double(), w["sigma_net.1.weight"].detach().double()[0]
    return (mask * w1) @ w0, 64 * 2.0 ** -23 * ((mask * w1.abs()) @ w0.abs())


def tcnn_hess_sums(x, table, cfg, e):
    """H[:, a, b] (a != b; the diagonal is 0: the interpolant is linear along each axis) = (1 / 2 bound)^2 sum_levels scale^2
    sum_corners w_third (|e0 v0| + |e1 v1|): the sum of the magnitudes of the terms of d^2 <e, encoding> / dx_a dx_b.  (B, 3, 3)."""
    bound = cfg["bound"]
    inside = ~tcnn_unit(x, bound)[2]
    H = torch.zeros(x.shape[0], 3, 3, dtype=torch.float64, device=x.device)
    e = e.detach().double().abs()
    for lv, (scale, res, off0, hsize) in enumerate(tcnn_levels(cfg)):
        idx, fr, bits = _corners(tcnn_pos(x, bound, scale), table, off0, hsize, res)
        wa = torch.where(bits[None].bool(), fr[:, None, :], 1 - fr[:, None, :])
        ev = (table[idx].double().abs() * e[:, None, 2 * lv:2 * lv + 2]).sum(-1)
        for a in range(3):
            for b in range(3):
                if a != b:
                    H[:, a, b] += (scale / (2.0 * bound)) ** 2 * (wa[..., 3 - a - b] * ev).sum(1)
    return H * inside[:, None, None]


def tcnn_second_order_dx_bound(x, table, cfg, w, acts, grad_sigma, g_normal):
    """Per-sample, per-axis bound (B, 3) on an fp32 evaluation of the part of dL/dx that arrives through normal = l2n(-g),
    g = d sigma / dx:   dL/dx_a = sum_{b != a} t_b H_ab,   t = -(c - n <n, c>) / |g|  (c = dL/d normal),
    H_ab = d g_b / dx_a = (1 / 2 bound)^2 sum_levels scale^2 sum_corners +-w_third <q, v>,  q = d sigma / d encoding.
      - the 128-term sum H_ab: 136 eps32 of the sum of its magnitudes, plus that sum taken with the rounding bound dq of q;
      - t: g itself is such a sum (136 eps32 * its magnitudes + the same with dq): |dg|; the projection and the division by |g|
        turn it into |dt| <= 3 |c| |dg| / |g|^2, plus 16 eps32 |c| / |g| for their own roundings -- the 1 / |grad sigma| of the
        sample, squared where its own error enters."""
    eps = 2.0 ** -23
    q, dq = tcnn_sigma_enc_grad(w, acts)
    g = grad_sigma.double()
    gn = g.norm(dim=-1).clamp_min(1e-300)
    c = g_normal.double()
    cn = c.norm(dim=-1)
    n = -g / gn[:, None]
    t = -(c - n * (n * c).sum(-1, keepdim=True)) / gn[:, None]
    dg = 136 * eps * tcnn_dx_sums(x, table, cfg, q)[0] + tcnn_dx_sums(x, table, cfg, dq)[0]
    dt = 3 * cn * dg.norm(dim=-1) / gn ** 2 + 16 * eps * cn / gn
    Hq = tcnn_hess_sums(x, table, cfg, q)
    dH = 136 * eps * Hq + tcnn_hess_sums(x, table, cfg, dq)
    tol = (t.abs()[:, None, :] * dH).sum(-1) + dt[:, None] * Hq.sum(-1)
    return torch.where(tcnn_unit(x, cfg["bound"])[2][:, None], torch.zeros_like(tol), tol)      # (outside the box: g = 0, nothing flows)


def tcnn_second_order_table_abs(x, table, cfg, w, acts, grad_sigma, g_normal):
    """Per table entry the sum of the MAGNITUDES of the contributions it receives through normal = l2n(-d sigma / dx):
    sum_samples sum_b |t_b| (scale / 2 bound) sum_corners (w_b' w_b'') |q_k|, t as in tcnn_second_order_dx_bound.  (entries, 2)."""
    bound = cfg["bound"]
    q = tcnn_sigma_enc_grad(w, acts)[0].abs()
    g = grad_sigma.double()
    gn = g.norm(dim=-1).clamp_min(1e-300)
    c = g_normal.double()
    n = -g / gn[:, None]
    t = ((c - n * (n * c).sum(-1, keepdim=True)) / gn[:, None]).abs()
    inside = (~tcnn_unit(x, bound)[2]).double()
    out = torch.zeros(int(cfg["offsets"][-1]), 2, dtype=torch.float64, device=x.device)
    for lv, (scale, res, off0, hsize) in enumerate(tcnn_levels(cfg)):
        idx, fr, bits = _corners(tcnn_pos(x, bound, scale), table, off0, hsize, res)
        wa = torch.where(bits[None].bool(), fr[:, None, :], 1 - fr[:, None, :])
        ww = sum(t[:, None, a] * wa[..., (a + 1) % 3] * wa[..., (a + 2) % 3] for a in range(3)) * (scale / (2.0 * bound))
        contrib = (ww * inside[:, None])[..., None] * q[:, None, 2 * lv:2 * lv + 2]                   # (B, 8, 2)
        out.index_add_(0, idx.reshape(-1), contrib.reshape(-1, 2))
    return out


def tcnn_dx_sums(x, table, cfg, g_enc):
    """The absolute sums that bound an fp32 evaluation of dL/dx = (1 / 2 bound) sum_levels scale sum_corners +-(w_b w_c) (e0 v0 + e1 v1),
    e = dL/d encoding (B, 2 * n_levels), in float64: (A, J), both (B, 3).
    A[:, a]: the same sum with every term's magnitude (what the rounding of the products and of the 128-term sum scales with);
    J[:, a]: (1 / 2 bound) sum_levels scale sum_corners (w_b w_c) (|v0| + |v1|) (what an error of e is multiplied by)."""
    bound = cfg["bound"]
    inside = ~tcnn_unit(x, bound)[2]
    A = torch.zeros(x.shape[0], 3, dtype=torch.float64, device=x.device)
    J = torch.zeros_like(A)
    e = g_enc.detach().double().abs()
    for lv, (scale, res, off0, hsize) in enumerate(tcnn_levels(cfg)):
        idx, fr, bits = _corners(tcnn_pos(x, bound, scale), table, off0, hsize, res)
        wa = torch.where(bits[None].bool(), fr[:, None, :], 1 - fr[:, None, :])                        # (B, 8, 3)
        v = table[idx].double().abs()                                                                  # (B, 8, 2)
        ev = (v * e[:, None, 2 * lv:2 * lv + 2]).sum(-1)                                               # (B, 8)
        for a in range(3):
            ww = wa[..., (a + 1) % 3] * wa[..., (a + 2) % 3]
            A[:, a] += scale / (2.0 * bound) * (ww * ev).sum(1)
            J[:, a] += scale / (2.0 * bound) * (ww * v.sum(-1)).sum(1)
    return A * inside[:, None], J * inside[:, None]


def tcnn_relu_margin(w, acts, enc, d):
    """(B,) float64: the smallest |pre-activation| / (sum of the magnitudes of the terms of its dot product) over every ReLU /
    LeakyReLU unit of the field.  Where it is below a few fp32 roundings of a 64-term sum two correct evaluations may take different
    sides of the kink, and their GRADIENTS for that sample differ by a jump."""
    geo = (torch.relu(acts["s0"]) @ w["sigma_net.1.weight"].T)[:, 1:]
    ins = {"s0": (enc, "sigma_net.0.weight"), "n0": (geo, "normal_net.0.weight"), "m0": (geo, "is_mirror_net.0.weight"),
           "c0": (torch.cat([sh4(d), geo], -1), "color_net.0.weight"), "c1": (torch.relu(acts["c0"]), "color_net.1.weight")}
    worst = None
    for name, (inp, wn) in ins.items():
        mag = inp.detach().abs() @ w[wn].detach().abs().T
        if name == "m0":
            mag = mag + w["is_mirror_net.0.bias"].detach().abs()
        r = (acts[name].detach().abs() / mag.clamp_min(1e-300)).amin(-1)
        worst = r if worst is None else torch.minimum(worst, r)
    return worst
