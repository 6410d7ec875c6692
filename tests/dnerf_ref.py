"""A float64 restatement of the D-NeRF object field and its renderer, for the tests of mirror_nerf_amd/dnerf.py: the module
DirectTemporalNeRF (deformation net, x + dx, canonical net) and render_rays / raw2outputs / sample_pdf of the D-NeRF code base,
written from their description in torch, evaluated in whatever dtype the inputs have (float64 in the tests).
tests/test_dnerf_ref_cpu.py pins it against values captured from the reference itself (fixtures G27)."""
import numpy as np
import torch

# the weights of fixture G27-model: the density head and the deformation head of a random-init field are nearly constant in
# space without a gain
MODEL_SEED = 7
MODEL_TWEAKS = [["_occ.alpha_linear.weight", "mul", 1000.0], ["_time_out.weight", "mul", 5.0]]


def make_state_dicts(seed, n_models=1):
    """`n_models` state dicts (name -> float32 ndarray) of DirectTemporalNeRF modules built one after the other behind ONE
    manual_seed, as create_nerf builds network_fn and then network_fine."""
    from mirror_nerf_amd.dnerf import DirectTemporalNeRF
    torch.manual_seed(seed)
    return [{k: v.detach().numpy().copy() for k, v in DirectTemporalNeRF().state_dict().items()} for _ in range(n_models)]


def module_of(sd, device=None, zero_canonical=True):
    from mirror_nerf_amd.dnerf import DirectTemporalNeRF
    m = DirectTemporalNeRF(zero_canonical=zero_canonical)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return (m.to(device) if device is not None else m).eval()


def embed(x, n_freqs):
    """[x, sin(x 2^0), cos(x 2^0), sin(x 2^1) ...]: the argument is formed as x * freq."""
    out = [x]
    for k in range(n_freqs):
        out += [torch.sin(x * 2.0 ** k), torch.cos(x * 2.0 ** k)]
    return torch.cat(out, -1)


def _lin(sd, name, h):
    w = torch.as_tensor(sd[name + ".weight"]).to(device=h.device, dtype=h.dtype)
    b = torch.as_tensor(sd[name + ".bias"]).to(device=h.device, dtype=h.dtype)
    return h @ w.T + b


def _trunk(sd, prefix, first, enc):
    """8 Linears with ReLU behind each; behind the one at index 4 the encoding is put in FRONT of the activations."""
    h = first
    for i in range(8):
        h = torch.relu(_lin(sd, f"{prefix}.{i}", h))
        if i == 4:
            h = torch.cat([enc, h], -1)
    return h


def deformation(sd, xyz, t):
    """The deformation net: -> dx (B,3) of the positions (B,3) at time t (a float, rounded to float32 as the caller's is)."""
    enc = embed(xyz, 10)
    te = embed(torch.full((xyz.shape[0], 1), float(t), dtype=torch.float32, device=xyz.device).to(xyz.dtype), 10)
    return _lin(sd, "_time_out", _trunk(sd, "_time", torch.cat([enc, te], -1), enc))


def canonical(sd, pts, viewdirs):
    """The canonical NeRF: -> cat[rgb raw, alpha raw] (B,4) at the (moved) points (B,3) for unit directions (B,3)."""
    enc = embed(pts, 10)
    h = _trunk(sd, "_occ.pts_linears", enc, enc)
    alpha = _lin(sd, "_occ.alpha_linear", h)
    feat = _lin(sd, "_occ.feature_linear", h)
    hv = torch.relu(_lin(sd, "_occ.views_linears.0", torch.cat([feat, embed(viewdirs, 4)], -1)))
    return torch.cat([_lin(sd, "_occ.rgb_linear", hv), alpha], -1)


def field(sd, xyz, viewdirs, t, zero_canonical=True):
    """-> (cat[rgb raw, alpha raw] (B,4), dx (B,3)) at time t (a float) for positions (B,3) and unit directions (B,3): the
    canonical net at x + dx, one add in the inputs' dtype; at t = 0 with zero_canonical the deformation net is not asked."""
    if float(t) == 0.0 and zero_canonical:
        return canonical(sd, xyz, viewdirs), torch.zeros_like(xyz)
    dx = deformation(sd, xyz, t)
    return canonical(sd, xyz + dx, viewdirs), dx


def composite(raw, z, rays_d, white_bkgd):
    """raw (N,S,4), z (N,S) -> rgb_map, disp_map, acc_map, weights, depth_map."""
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], -1) * torch.norm(rays_d[:, None, :], dim=-1)
    alpha = 1.0 - torch.exp(-torch.relu(raw[..., 3]) * dists)
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10], -1), -1)[:, :-1]
    w = alpha * trans
    rgb_map = (w[..., None] * torch.sigmoid(raw[..., :3])).sum(-2)
    depth, acc = (w * z).sum(-1), w.sum(-1)
    disp = 1.0 / torch.max(1e-10 * torch.ones_like(depth), depth / acc)
    if white_bkgd:
        rgb_map = rgb_map + (1.0 - acc[:, None])
    return rgb_map, disp, acc, w, depth


def sample_pdf(bins, weights, n):
    """n deterministic inverse-CDF samples of the piecewise-constant pdf `weights` over `bins`."""
    weights = weights + 1e-5
    cdf = torch.cumsum(weights / weights.sum(-1, keepdim=True), -1)
    cdf = torch.cat([torch.zeros_like(cdf[:, :1]), cdf], -1)
    u = torch.linspace(0.0, 1.0, n).to(cdf.dtype).expand(cdf.shape[0], n).contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below, above = (inds - 1).clamp(min=0), inds.clamp(max=cdf.shape[-1] - 1)
    c0, c1 = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    b0, b1 = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    denom = c1 - c0
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    return b0 + (u - c0) / denom * (b1 - b0)


def render(sd, sd_fine, ray_batch, N_samples, N_importance=0, white_bkgd=False, lindisp=False, zero_canonical=True):
    """ray_batch (N,12): o, d, near, far, time, unit direction -> the reference's dict.  sd_fine: None for a single model."""
    o, d, view = ray_batch[:, 0:3], ray_batch[:, 3:6], ray_batch[:, 9:12]
    near, far, t = ray_batch[:, 6:7], ray_batch[:, 7:8], float(ray_batch[0, 8])
    N = ray_batch.shape[0]
    # the steps and their complement are fp32 tensors whatever the rays' dtype is (a float64 run of the reference keeps them)
    steps = torch.linspace(0.0, 1.0, N_samples)
    rest, steps = (1.0 - steps).to(ray_batch.dtype), steps.to(ray_batch.dtype)
    z = 1.0 / (1.0 / near * rest + 1.0 / far * steps) if lindisp else near * rest + far * steps

    def query(state, z):
        S = z.shape[1]
        pts = (o[:, None, :] + d[:, None, :] * z[:, :, None]).reshape(-1, 3)
        raw, dx = field(state, pts, view[:, None, :].expand(N, S, 3).reshape(-1, 3), t, zero_canonical)
        return raw.view(N, S, 4), dx.view(N, S, 3)
    if N_importance > 0:
        w = composite(query(sd, z)[0], z, d, white_bkgd)[3]
        zs = sample_pdf(0.5 * (z[:, 1:] + z[:, :-1]), w[:, 1:-1], N_importance)
        z = torch.sort(torch.cat([z, zs], -1), -1)[0]
    raw, dx = query(sd if sd_fine is None else sd_fine, z)
    rgb_map, disp, acc, _w, depth = composite(raw, z, d, white_bkgd)
    return {"rgb_map": rgb_map, "disp_map": disp, "acc_map": acc, "depth_map": depth, "z_vals": z, "position_delta": dx}
