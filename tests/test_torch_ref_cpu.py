"""CPU tests of the float64 reference the field-backward tests differentiate (tests/torch_ref.py `field(..., masks=)`)."""
import torch

from tests import torch_ref as TR


def _weights(seed):
    from tests.golden import weights as GW
    sd = GW.apply_tweaks(GW.make_state_dict(seed, 1)[0], GW.OPAQUE)
    return {k: torch.from_numpy(v).double() for k, v in sd.items()}


def _inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(B, 3, generator=g, dtype=torch.float64) * 4 - 2
    de = TR.embed(TR.l2n(torch.randn(B, 3, generator=g, dtype=torch.float64)), 4)
    return xyz, de


def test_masked_field_equals_the_relu_field_bit_for_bit():
    """With the masks of its own forward, y * mask is relu(y) / leaky_relu(y) exactly: outputs (the density-gradient normal
    included) and first-order gradients are the same bits as the plain version."""
    w = _weights(5)
    xyz, de = _inputs(64, 0)
    acts = {}
    with torch.no_grad():
        TR.field(w, xyz, de, acts=acts)
    masks = TR.masks_of({n: acts[n] for n in TR.MASK_NAMES})
    assert all(int((m != 1).sum()) > 0 for m in masks.values())          # every activation has inactive units here
    res = []
    for mk in (None, masks):
        wl = {k: v.clone().requires_grad_(True) for k, v in w.items()}
        x = xyz.clone().requires_grad_(True)
        d = de.clone().requires_grad_(True)
        outs = TR.field(wl, x, d, with_normal=True, masks=mk)
        sum((o * (i + 1)).sum() for i, o in enumerate(outs[:4])).backward()
        res.append([o.detach() for o in outs] + [x.grad, d.grad] + [wl[k].grad for k in sorted(wl)])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_masked_field_double_backward_matches_gradcheck():
    """The second-order path (the density-gradient normal, differentiated again) of the masked reference against finite
    differences: with the masks held constant the function is smooth, so gradcheck holds at every point."""
    w = _weights(11)
    xyz, de = _inputs(3, 1)
    acts = {}
    with torch.no_grad():
        TR.field(w, xyz, de, acts=acts)
    masks = TR.masks_of({n: acts[n] for n in TR.MASK_NAMES})
    small = ("sigma.bias", "xyz_encoding_8.0.bias", "xyz_encoding_1.0.bias")

    def fn(x, d, *vals):
        wl = dict(w)
        for k, v in zip(small, vals):
            wl[k] = v
        sigma, rgb, pn, m, nrm = TR.field(wl, x, d, with_normal=True, masks=masks)
        return sigma, rgb, pn, m, nrm

    args = [xyz.clone().requires_grad_(True), de.clone().requires_grad_(True)] + \
           [w[k].clone().requires_grad_(True) for k in small]
    assert torch.autograd.gradcheck(fn, args, eps=1e-6, atol=1e-7, rtol=1e-5)
