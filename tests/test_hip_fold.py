"""The full forward-only split kernels read the FOLDED stream (csrc/mnrf_layout.h OFF_FOLD_FWD): normal_net's two Linears as one
3 x 256 map, xyz_encoding_final folded into dir_encoding.  The training forward keeps the unfolded heads.  On the same samples the
two must give the same sigma and mirror probability bit for bit (their arithmetic is untouched) and rgb / predicted normal
within 1e-5."""
import pytest
import torch

from tests.golden import fixtures as FX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _module(sd):
    import mirror_nerf_amd as M
    m = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal="normal_net.0.weight" in sd,
                     predict_mirror_mask="is_mirror_net.0.weight" in sd)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV)


def _train_forward(model, xyz, de):
    """Outputs of the split training forward (unfolded stream, fp32 rows) on the same samples."""
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd.weights import packed_of
    L, p = _lib.lib(), _lib.ptr
    B = xyz.shape[0]
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=DEV)  # noqa: E731
    o = (f(B), f(B, 3), f(B, 3), f(B), f(B, 3))
    sx, sm = f(L.mnrf_train_save_floats(B)), torch.zeros(L.mnrf_train_mask_words(B), dtype=torch.int64, device=DEV)
    _lib.check(L.mnrf_field_forward_train(p(packed_of(model)), B, p(xyz), 3, None, None, 1, p(de), 27, *[p(t) for t in o], p(sx),
                                          p(sm), p(f(B)), p(f(B)), _lib.MNRF_SPLIT_F16, _lib.stream()), "mnrf_field_forward_train")
    return dict(zip(("sigma", "rgb", "pred_normal", "is_mirror"), o[:4]))


@pytest.mark.parametrize("which", ["g11_trained", "g4_fine"])
def test_folded_forward_matches_the_unfolded_training_forward(which):
    import mirror_nerf_amd as M
    from mirror_nerf_amd import mirror_nerf as MN
    old = MN.PRECISION
    MN.set_precision("split")
    try:
        sd = FX.Fixture("g11_trained_render_test" if which == "g11_trained" else "g4_fine_test").state_dicts()[-1]
        model = _module(sd)
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        B = 192 * (cus + 3) + 5      # ragged, more tiles than CUs: the dynamic tile queue of the 48-sample kernel
        torch.manual_seed(7)
        xyz = (torch.rand(B, 3, device=DEV) * 2.4 - 1.2).contiguous()
        de = M.Embedding(4)(torch.nn.functional.normalize(torch.randn(B, 3, device=DEV), dim=1)).contiguous()
        want = _train_forward(model, xyz, de)
        torch.cuda.synchronize()
        for geo in (False, True):      # 48 samples per wave; 32 samples per wave (a geo_feat request)
            got = MN.field_forward(model, B, xyz=xyz, dir_emb=de, dir_stride=27, want_geo=geo)
            torch.cuda.synchronize()
            for k in ("sigma", "is_mirror"):
                assert torch.equal(got[k].reshape(-1), want[k].reshape(-1)), (k, geo)
            for k in ("rgb", "pred_normal"):
                err = float((got[k] - want[k]).abs().max())
                assert err <= 1e-5, (k, geo, err)
    finally:
        MN.set_precision(old)


def test_fold_is_deterministic_and_batched_equals_one_by_one():
    """mnrf_fold_weights_n: a fixed summation order and no atomics in the values -- two models folded in one launch give the
    images that two single-model calls give, bit for bit."""
    import ctypes
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd.weights import _param_pointers, pack_states, param_refs
    L = _lib.lib()
    sds = FX.Fixture("g11_trained_render_test").state_dicts()
    models = [_module(sd) for sd in sds]
    states = [{full: sub._parameters[pname] for sub, pname, full in param_refs(m)} for m in models]
    imgs = {}
    for mode in ("batched", "single"):
        out = pack_states(states, [torch.zeros(L.mnrf_packed_floats(), device=DEV) for _ in states])      # (regions nobody writes stay zero)
        keep, arr = [], (ctypes.c_void_p * (_lib.N_PARAMS * 2))()
        for i, st in enumerate(states):
            _param_pointers(st, arr, i * _lib.N_PARAMS, keep)
        ptrs = (ctypes.c_void_p * 2)(*[o.data_ptr() for o in out])
        if mode == "batched":
            _lib.check(L.mnrf_fold_weights_n(2, arr, ptrs, _lib.stream()), "mnrf_fold_weights_n")
        else:
            for i in range(2):
                one = (ctypes.c_void_p * _lib.N_PARAMS)(*arr[i * _lib.N_PARAMS:(i + 1) * _lib.N_PARAMS])
                _lib.check(L.mnrf_fold_weights_n(1, one, (ctypes.c_void_p * 1)(ptrs[i]), _lib.stream()), "mnrf_fold_weights_n")
        torch.cuda.synchronize()
        imgs[mode] = out
    for a, b in zip(imgs["batched"], imgs["single"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
