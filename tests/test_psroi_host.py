"""CPU checks of the deformable PS-ROI pooling boundary and of its yardstick tests/psroi_ref.py: the shims export the reference's
names, host tensors are refused, DCNPooling has the reference's parameters, and the restatement is pinned by the known answer of
model/DCNv2/test.py's zero-offset check, by closed forms, by gradcheck and by the exactness conditions of the lattice case that
tests/test_gpu_psroi.py compares bit for bit."""
import numpy as np
import pytest
import torch

import psroi_ref as R


# ------------------------------------------------------------------------------------------------ (a) the host boundary
def test_shims_export_the_pooling_names():
    import model.DCNv2.dcn_v2 as d
    import model.DCNv2.dcn_v2_func as f
    from m3dssd_amd.host import dcn, ops
    for n in ("DCNv2Pooling", "DCNPooling"):
        assert getattr(d, n) is getattr(dcn, n)
    assert f.DCNv2PoolingFunction is dcn.DCNv2PoolingFunction
    for n in ("psroi_pooling_forward", "psroi_pooling_backward", "psroi_pooling"):
        assert callable(getattr(ops, n))
    fn = f.DCNv2PoolingFunction(0.25, 7, 16, False, trans_std=0.1)
    assert fn.part_size == 7 and fn._infer_shape(torch.zeros(2, 16, 8, 8), torch.zeros(5, 5)) == (5, 16, 7, 7)
    with pytest.raises(AssertionError):
        f.DCNv2PoolingFunction(0.25, 7, 16, False, trans_std=1.5)


def test_host_tensors_raise_not_implemented():
    from m3dssd_amd.host import ops
    from model.DCNv2.dcn_v2 import DCNv2Pooling, DCNPooling
    data, rois, c0, c1, trans = R.zero_offset_case()
    with pytest.raises(NotImplementedError):
        ops.psroi_pooling_forward(data, rois, trans, *c1)
    with pytest.raises(NotImplementedError):
        ops.psroi_pooling_backward(torch.zeros(2, 16, 7, 7), data, rois, trans, *c1)
    with pytest.raises(NotImplementedError):
        ops.psroi_pooling(data, rois, trans, *c1)
    with pytest.raises(NotImplementedError):
        DCNv2Pooling(0.25, 7, 16, True)(data, rois, data.new_empty(0))
    with pytest.raises(NotImplementedError):
        DCNPooling(0.25, 7, 16, False, trans_std=0.1, deform_fc_dim=8)(data, rois)


def test_dcn_pooling_parameters():
    from model.DCNv2.dcn_v2 import DCNPooling
    m = DCNPooling(spatial_scale=0.25, pooled_size=7, output_dim=32, no_trans=False, group_size=1, part_size=None, sample_per_part=4,
                   trans_std=0.1, deform_fc_dim=64)
    keys = set(m.state_dict())
    assert keys == {"offset_fc.%d.%s" % (i, p) for i in (0, 2, 4) for p in ("weight", "bias")} | \
        {"mask_fc.%d.%s" % (i, p) for i in (0, 2) for p in ("weight", "bias")}
    assert tuple(m.offset_fc[0].weight.shape) == (64, 7 * 7 * 32) and tuple(m.offset_fc[4].weight.shape) == (7 * 7 * 2, 64)
    assert tuple(m.mask_fc[2].weight.shape) == (7 * 7, 64)
    for t in (m.offset_fc[4].weight, m.offset_fc[4].bias, m.mask_fc[2].weight, m.mask_fc[2].bias):
        assert not t.any()
    assert m.offset_fc[0].weight.any() and m.mask_fc[0].weight.any()
    assert m.part_size == 7 and m.deform_fc_dim == 64
    assert not list(DCNPooling(0.25, 7, 32, True).state_dict())


# ------------------------------------------------------------------------------------------------ (b) test.py's zero-offset case
def test_restatement_on_the_zero_offset_case():
    data, rois, c0, c1, trans = R.zero_offset_case()
    out, cnt = R.psroi_ref(data.double(), rois, None, c0)
    assert (cnt == 16).all()
    for i, mean in enumerate(R.ZERO_OFFSET_MEANS):
        assert abs(out[i].mean().item() - mean) < 5e-8, (i, out[i].mean().item())
    out_t, cnt_t = R.psroi_ref(data.double(), rois, trans.double(), c1)
    assert torch.equal(out.view(torch.int64), out_t.view(torch.int64)) and torch.equal(cnt, cnt_t)


# ------------------------------------------------------------------------------------------------ (c) closed forms
def _random_case(seed, N=2, C=8, H=20, W=24, n=6, D=8, G=1, P=3, part=3, S=2, K=1, std=0.1, no_trans=False):
    g = torch.Generator().manual_seed(seed)
    data = torch.randn(N, C, H, W, generator=g)
    rois = R.make_rois(n, N, seed + 1, xy_max=4 * W, wh_max=2 * W, integer=False)
    trans = None if no_trans else torch.randn(n + 1, 2 * K, part, part, generator=g)
    return data, rois, trans, (no_trans, 0.25, D, G, P, part, S, std)


def test_constant_data_gives_the_constant():
    for seed, G in ((3, 1), (4, 2)):
        data, rois, trans, conf = _random_case(seed, C=8 * G * G, G=G, P=4, part=2, D=8, K=2)
        data = torch.full_like(data, 2.5)
        out, cnt = R.psroi_ref(data.double(), rois, trans.double(), conf)
        assert (cnt > 0).any() and (cnt == 0).any()                  # regions drawn partly outside the map
        assert (out[cnt > 0] - 2.5).abs().max() < 1e-14
        assert not out[cnt == 0].any()


def test_ramp_data_gives_the_mean_of_the_ramp():
    """data = a*x + b*y in every channel, all samples strictly inside the map: bilinear interpolation reproduces the ramp, so a
    bin is the ramp at the mean of its S*S sample coordinates."""
    N, C, H, W, a, b = 1, 4, 40, 48, 0.75, -1.25
    ys, xs = torch.arange(H).double().view(H, 1), torch.arange(W).double().view(1, W)
    data = (a * xs + b * ys).expand(N, C, H, W).contiguous()
    rois = torch.tensor([[0, 30.2, 41.7, 110.4, 99.1], [0, 60.0, 50.5, 121.3, 120.9], [0, 35.5, 36.5, 37.4, 38.6]])
    g = torch.Generator().manual_seed(5)
    trans = (torch.rand(3, 2, 3, 3, generator=g) - 0.5).double()
    conf = (False, 0.25, 4, 1, 3, 3, 3, 0.1)
    w, h, cnt = R.sample_coords(data.shape, rois, trans, conf)
    assert (cnt == 9).all() and w.min() > 0 and w.max() < W - 1 and h.min() > 0 and h.max() < H - 1
    out, _ = R.psroi_ref(data, rois, trans, conf)
    want = a * w.mean(-1) + b * h.mean(-1)                              # [n, K = 1, P, P]
    assert (out - want.expand(3, 4, 3, 3)).abs().max() < 1e-12


# ------------------------------------------------------------------------------------------------ (d) gradcheck
@pytest.mark.parametrize("G,K", [(1, 1), (2, 2)])
def test_gradcheck_of_the_restatement(G, K):
    g = torch.Generator().manual_seed(7 + G)
    N, H, W, D, P, part, S = 2, 6, 7, K, 2 * G, G, 2        # small: gradcheck perturbs every input
    data = torch.randn(N, D * G * G, H, W, generator=g).double().requires_grad_(True)
    rois = torch.tensor([[0, 3.3, 2.1, 20.2, 17.7], [1, -6.0, 9.4, 14.9, 40.3], [1, 10.1, 4.2, 24.6, 19.5]])
    trans = torch.randn(4, 2 * K, part, part, generator=g).double().requires_grad_(True)
    conf = (False, 0.25, D, G, P, part, S, 0.1)
    assert torch.autograd.gradcheck(lambda d, t: R.psroi_ref(d, rois, t, conf, coord32=False)[0], (data, trans), eps=1e-6, atol=1e-7,
                                    rtol=1e-5)
    out, cnt, gd, gt = R.ref_grads(data, rois, trans, torch.ones(3, D, P, P), conf, coord32=False)
    assert not gt[3].any() and gt[:3].any()                            # the row of trans past n


# ------------------------------------------------------------------------------------------------ (e) the part index
def test_part_index_is_the_float32_expression():
    diff = []
    for P in range(1, 33):
        f = R.part_index(P, P).tolist()
        for ph in range(P):
            v = int(np.floor(np.float32(np.float32(ph) / np.float32(P)) * np.float32(P)))
            assert f[ph] == v
            if v != (ph * P) // P:
                diff.append((ph, P))
    assert diff == [(13, 22), (7, 23), (14, 23), (15, 29)]
    assert R.group_index(7, 7).tolist() == list(range(7)) and R.group_index(6, 3).tolist() == [0, 0, 1, 1, 2, 2]
    assert R.round_half_away(torch.tensor([0.5, 1.5, 2.5, -0.5, -2.5, 0.49999997, 2.4, -2.6])).tolist() == [1, 2, 3, -1, -3, 0, 2, -3]


# ------------------------------------------------------------------------------------------------ (f) the lattice case
def _is_multiple(t, k):
    s = t.double() * 2.0 ** k
    return bool((s == torch.round(s)).all())


def test_lattice_case_is_exact():
    data, rois, trans, go, conf = R.lattice_case()
    D, G, P, part, S = conf[2], conf[3], conf[4], conf[5], conf[6]
    assert tuple(data.shape) == (2, 16, 32, 32) and (D, G, P, part, S) == (4, 2, 4, 2, 4) and trans.shape[1] == 4
    assert set(data.unique().tolist()) == {-3., -2., -1., 1., 2., 3.}
    assert _is_multiple(trans, 3) and trans.abs().max() <= 0.25 and _is_multiple(go, 2) and go.abs().max() <= 2
    w32, h32, cnt = R.sample_coords(data.shape, rois, trans, conf, coord32=True)
    w64, h64, cnt64 = R.sample_coords(data.shape, rois, trans, conf, coord32=False)
    assert torch.equal(w32, w64) and torch.equal(h32, h64) and torch.equal(cnt, cnt64)      # no coordinate operation rounds
    assert (cnt == 16).all()
    for t, size in ((w32, 32), (h32, 32)):
        assert ((t * 4) % 2 == 1).all()                                # odd multiples of 1/4: never an integer
        assert t.min() > 0 and t.max() < size - 1                      # never clamped
    out, _, gd, gt = R.ref_grads(data, rois, trans, go, conf)
    Td, Ad, Tt, At = R.grad_terms(data, rois, trans, go, conf)
    # weights are multiples of 1/16, grad_out / 16 of 1/64, trans_std * roi size is 4 or 8: every term of every sum is a multiple of
    # 2^-10 (forward: 2^-4 before the division by 16) and the sums of absolute values stay below 2^24 granules, so every partial
    # sum in any order is a float32 number
    assert _is_multiple(out, 8) and out.abs().max() <= 3 and torch.equal(out, out.float().double())
    for grad, A in ((gd, Ad), (gt, At)):
        assert _is_multiple(grad, 10) and _is_multiple(A, 10) and A.max() * 2.0 ** 10 < 2.0 ** 24
        assert torch.equal(grad, grad.float().double()) and (grad.abs() <= A).all()
    assert gd.any() and gt.any() and Td.max() > 1 and Tt.max() == 2 * 4 * 16
