"""The forward-only split kernels evaluate two head pairs of MirrorNeRF folded into one Linear each (csrc/mnrf_layout.h
OFF_FOLD_FWD): normal_net = Linear(256,128) -> Linear(128,3) with no activation between, and xyz_encoding_final, whose output
only feeds dir_encoding.  Folded in fp64 and rounded to fp32 as the packer does, the oracle's per-sample rgb and predicted normal
on the fixtures' fine samples move by far less than the 1e-4 parity tolerance (<= 1e-5 here); sigma and the mirror head do not move."""
import numpy as np
import pytest

from oracle import mirror_nerf_oracle as O
from tests.golden import fixtures as FX


def fold(sd):
    """State dict with the two folded maps in place, written as identity layers around them so that the oracle runs unchanged."""
    f = dict(sd)
    w1, b1 = sd["normal_net.0.weight"].astype(np.float64), sd["normal_net.0.bias"].astype(np.float64)
    w2, b2 = sd["normal_net.1.weight"].astype(np.float64), sd["normal_net.1.bias"].astype(np.float64)
    f["normal_net.0.weight"] = (w2 @ w1).astype(np.float32)
    f["normal_net.0.bias"] = (w2 @ b1 + b2).astype(np.float32)
    f["normal_net.1.weight"] = np.eye(3, dtype=np.float32)
    f["normal_net.1.bias"] = np.zeros(3, np.float32)
    wf, bf = sd["xyz_encoding_final.weight"].astype(np.float64), sd["xyz_encoding_final.bias"].astype(np.float64)
    wd, bd = sd["dir_encoding.0.weight"], sd["dir_encoding.0.bias"].astype(np.float64)
    f["dir_encoding.0.weight"] = np.concatenate([(wd[:, :256].astype(np.float64) @ wf).astype(np.float32), wd[:, 256:]], 1)
    f["dir_encoding.0.bias"] = (wd[:, :256].astype(np.float64) @ bf + bd).astype(np.float32)
    f["xyz_encoding_final.weight"] = np.eye(256, dtype=np.float32)
    f["xyz_encoding_final.bias"] = np.zeros(256, np.float32)
    return f


@pytest.mark.parametrize("name", ["g4_fine_test", "g11_trained_render_test", "g11_rough_render_test"])
def test_folded_heads_keep_the_oracle_outputs(name):
    fx = FX.Fixture(name)
    sd = fx.state_dicts()[-1]      # the fine model
    rays = fx.inputs["rays"].astype(np.float32)
    z = fx.outputs["z_vals_fine"].astype(np.float32)
    xyz = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)
    dirs = np.repeat(O.embedding(rays[:, 3:6], 4), z.shape[1], axis=0)
    x = np.concatenate([xyz, dirs], 1).astype(np.float32)
    want = O.field_forward(sd, x)
    got = O.field_forward(fold(sd), x)
    for k in ("sigma", "is_mirror"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("rgb", "pred_normal"):
        err = float(np.max(np.abs(got[k] - want[k])))
        assert err <= 1e-5, (name, k, err)
