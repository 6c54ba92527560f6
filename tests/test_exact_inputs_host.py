"""CPU tests of tests/exact_inputs.py: the premise of tests/test_gpu_exact.py.  For every generator and shape the GPU file uses,
the float64 reference must not change when every intermediate a kernel keeps narrow is rounded to that type (`assert_exact_under`);
the DCNv2 reference must equal the C oracle bit for bit; and the torch.equal comparison must see each structural error of the
sensitivity table at every seeded placement."""
import pytest
import torch

import exact_inputs as E
import test_gpu_exact as T

BF16, F16 = torch.bfloat16, torch.float16
SENS_SHAPE = (2, 128, 16, 40, 128, 3, 1)          # the first case of test_dcn_bf16_matches_oracle
PLACEMENTS = 30


def _oracle(ops):
    from oracle import dcn as odcn
    return odcn.dcn_v2_forward(ops["x"], ops["off"], ops["mask"], ops["weight"], ops["bias"], 1, ops["pad"], 1, ops["dg"]).double()


def _check_dcn(ops, patch=False, epilogue=True):
    ref = E.assert_exact_under(E.dcn_ref, ops, BF16)                      # implicit-GEMM tile / 1x1 kernel: fp32 corners, bf16 sample
    if patch:
        assert torch.equal(E.assert_exact_under(E.dcn_ref, ops, F16, F16), ref)      # patch kernel: fp16 corners, fma chain, sample, weights
    assert torch.equal(ref, _oracle(ops))                                 # the C oracle is fp32; the operands are exact in fp32
    x, wt = ops["x"], ops["weight"]
    assert (x != 0).all() and (wt != 0).all() and torch.equal(x, x.to(BF16).float()) and torch.equal(wt, wt.to(F16).float())
    if epilogue:
        scale, shift, res = E.dcn_epilogue_operands(sum(ops["x"].shape), ops, ref, act=1)
        pre = E.apply_epilogue(ref, scale, shift, res, act=0)
        assert float(pre.min()) >= 0                                      # LeakyReLU on, and the identity
        assert torch.equal(pre, pre.float().double()) and torch.equal(torch.log2(scale), torch.log2(scale).round())
    return ref


@pytest.mark.parametrize("shape", T.IGEMM_SHAPES)
def test_dcn_implicit_gemm_operands_are_exact(shape):
    n, c, h, w, co, k, pad = shape
    _check_dcn(E.dcn_operands(sum(shape), n, c, h, w, co, k, pad))


@pytest.mark.parametrize("shape,variant,at_radius", T.PATCH_CASES)
def test_dcn_patch_operands_are_exact(shape, variant, at_radius):
    ops = T.patch_operands(shape, at_radius)
    _check_dcn(ops, patch=True, epilogue=at_radius is None)
    if at_radius is not None:
        assert float(ops["off"].abs().max()) == {4: 8.75, 3: 5.75}[variant]


def test_dcn_hand_over_and_1x1_and_border_operands_are_exact():
    ops = T.handover_operands()
    _check_dcn(ops, patch=True, epilogue=False)
    assert float(ops["off"].abs().max()) == 10.25
    for n, h, w in [(2, 16, 40), (1, 9, 13), (3, 8, 16)]:
        ops = E.dcn_operands(n * 100 + h, n, 128, h, w, 128, 1, 0)
        ref = _check_dcn(ops, epilogue=False)
        with_res = ref + ops["x"].double()
        assert torch.equal(with_res, with_res.float().double())
    for c, co, k in [(64, 32, 1), (24, 32, 1), (32, 128, 3)]:
        h, w = (16, 24) if k == 1 else (16, 32)
        ops = T.border_operands(c, co, h, w, k)
        ref = E.assert_exact_under(E.dcn_ref, ops, F16 if k == 3 else BF16, F16 if k == 3 else torch.float32)
        assert torch.equal(ref, _oracle(ops))
    for shape in T.CONTROL_SHAPES:
        n, c, h, w, co, k, pad, dg = shape
        ops = E.dcn_operands(sum(shape), n, c, h, w, co, k, pad, dg=dg)
        assert torch.equal(E.assert_exact_under(E.dcn_ref, ops, torch.float32), _oracle(ops))


def test_dcn_reference_matches_the_loop_form_of_the_oracle():
    """The vectorised float64 reference against oracle/dcn.py:dcn_v2_forward_numpy (per-pixel loops) on random fp32 operands, border
    positions included: same corner rules."""
    from oracle import dcn as odcn
    g = torch.Generator().manual_seed(3)
    x, wt, b = torch.randn(1, 6, 7, 9, generator=g), torch.randn(5, 6, 3, 3, generator=g), torch.randn(5, generator=g)
    off, m = torch.randn(1, 18, 7, 9, generator=g) * 3.0, torch.rand(1, 9, 7, 9, generator=g)
    off[0, 0, 0, 0], off[0, 1, 0, 0] = 0.0, 10.0
    ref = E.dcn_ref(dict(x=x, off=off, mask=m, weight=wt, bias=b, stride=1, pad=1, dg=1))
    loop = torch.from_numpy(odcn.dcn_v2_forward_numpy(x.numpy(), off.numpy(), m.numpy(), wt.numpy(), b.numpy(), 1, 1, 1)).double()
    assert (ref - loop).abs().max().item() < 1e-5


def test_sensitivity_table_every_structural_error_is_seen(capsys):
    """One corner of one tap dropped at one pixel, the two low corners swapped, one 8-channel chunk of one tap dropped, two channels
    swapped in one tap for one output channel, one tap shifted by one column: the comparison of the GPU test (compare_exact =
    torch.equal on the output cast to the output type) reports each at every one of 30 seeded placements, in fp32 output mode; the
    bf16 output mode (one rounding of the same number) is counted.  Next to it: how many of the same errors, placed in the random
    operands of test_dcn_bf16_matches_oracle's first case, stay under that test's bound (1e-2 + 2^-8) * max|ref| -- logged, not
    asserted."""
    n, c, h, w, co, k, pad = SENS_SHAPE
    exact = E.dcn_operands(sum(SENS_SHAPE), n, c, h, w, co, k, pad)
    rand = E.tolerance_test_operands(SENS_SHAPE)
    scale = float(E.dcn_ref(rand).abs().max())
    bound = 1e-2 * scale + 2.0 ** -8 * scale
    table = {}
    for kind in E.PERTURBATIONS:
        seen32 = seen16 = hidden = 0
        for s in range(PLACEMENTS):
            _, wrong, right = E.perturbed_pixel(exact, kind, s)
            nd32, msg = E.compare_exact(wrong.float(), right, torch.float32, E.DCN_QUANTUM)
            nd16, _ = E.compare_exact(wrong.float().to(BF16).float(), right, BF16, E.DCN_QUANTUM)
            assert nd32 > 0 and "first difference at" in msg, (kind, s)
            seen32 += 1
            seen16 += nd16 > 0
            _, rwrong, rright = E.perturbed_pixel(rand, kind, s)
            hidden += float((rwrong - rright).abs().max()) < bound
        table[kind] = (seen32, seen16, hidden)
    with capsys.disabled():
        print("\nsensitivity (of %d placements): kind, seen exact fp32, seen exact bf16, under the 1e-2 bound on random operands" % PLACEMENTS)
        for kind, row in table.items():
            print("  %-22s %3d %3d %3d" % ((kind,) + row))


@pytest.mark.parametrize("G,n,h,w,cout", T.HEAD_SHAPES)
def test_head_operands_are_exact(G, n, h, w, cout):
    for hd in T.head_operands(G, n, h, w, cout):
        E.assert_exact_under(E.mlp_ref, hd, BF16)                         # form 1 keeps bf16 hidden maps; fp16 (form 2) is wider
        E.assert_exact_under(E.mlp_ref, hd, F16, weight_dtype=F16)
        assert torch.equal(hd["x"], T.head_operands(G, n, h, w, cout)[0]["x"]) and (hd["x"].abs() == 1).all()
        (w1, s1, t1), (w2, s2, t2), (w3, s3, t3) = hd["layers"]
        assert (w1 != 0).all() and (w3 != 0).all()
        assert ((w2 != 0).sum(1) == E.MLP_NNZ).all() and (w2.sum(1) == 0).all() and (w2 != 0).any(0).all()      # every input column used
        assert ((w1 * s1.view(-1, 1)).abs() == 1.0 / 16).all() and ((w2 * s2.view(-1, 1)).abs() <= 1).all() and (s1 != 1).any() and (s2 != 1).any()
        for sc in (s1, s2, s3):
            assert torch.equal(torch.log2(sc), torch.log2(sc).round())


@pytest.mark.parametrize("n,h,w,cout", T.TAIL_SHAPES)
def test_tail_operands_are_exact(n, h, w, cout):
    ops = T.tail_operands(n, h, w, cout)
    E.assert_exact_under(E.mlp_ref, ops, BF16)
    E.assert_exact_under(E.mlp_ref, ops, F16, weight_dtype=F16)
    assert all((l[0] != 0).all() for l in ops["layers"])


@pytest.mark.parametrize("n,h,w", T.QKVS_SHAPES)
def test_qkvs_operands_are_exact(n, h, w):
    ops = T.qkvs_operands(n, h, w)
    ref = E.assert_exact_under(E.mlp_ref, ops, BF16)
    assert torch.equal(ref, ref.float().to(BF16).double())                # the bf16 outputs hold the result exactly


@pytest.mark.parametrize("B,HW,keys", T.ATTEND_SHAPES)
def test_attend_operands_give_a_one_hot_softmax(B, HW, keys):
    for kp in (None, (keys + 31) // 32 * 32):
        ops = E.attend_operands(B * 100 + keys, B, HW, keys, kp=kp)
        ref = E.assert_exact_under(E.attend_ref, ops, BF16)
        S = torch.einsum("bpc,bkc->bpk", ops["q"].double().view(B, HW, -1), ops["khat"].double())
        top = S[:, :, :keys].topk(2, dim=-1)
        assert torch.equal(top.indices[..., 0], ops["target"]) and float((top.values[..., 0] - top.values[..., 1]).min()) >= 2 * E.ATT_GAIN > 104.0
        assert float(S[:, :, keys:].max()) > float(S[:, :, :keys].max())       # a padding key that was let in would win
        for b in range(B):
            assert ops["target"][b].unique().numel() == keys              # every key index is some query's target
        tv = torch.stack([ops["vhat"][b][:, ops["target"][b]].T for b in range(B)]).reshape(B * HW, -1).double()
        assert torch.equal(ref, (tv + ops["res"].double()) * ops["scale"].double() + ops["shift"].double())
        for k_ in ("q", "khat", "vhat", "res"):
            assert torch.equal(ops[k_], ops[k_].to(BF16).float())


@pytest.mark.parametrize("cin,H,W", T.TREE_SHAPES)
def test_tree_entry_operands_are_exact(cin, H, W):
    ops = T.tree_operands(cin, H, W)
    ref = E.assert_exact_under(E.tree_entry_ref, ops, F16)               # fp16 halo tile, fp16 folded weights, fp32 accumulators
    co = 2 * cin
    assert float(ref[:, :co].min()) >= 0                                 # t: LeakyReLU on, and the identity
    folded = ops["w1"] * ops["s1"].view(-1, 1, 1, 1)
    assert (ops["x"] != 0).all() and (folded != 0).all() and torch.equal(folded, folded.to(F16).float())
    import torch.nn.functional as Fn
    plain = Fn.leaky_relu(Fn.conv2d(ops["x"].double(), ops["w1"].double(), None, stride=2, padding=1) * ops["s1"].double().view(1, -1, 1, 1)
                          + ops["t1"].double().view(1, -1, 1, 1), 0.01)
    assert torch.equal(plain, ref[:, :co])                               # the unfold form of the reference == torch's convolution


@pytest.mark.parametrize("n,H,W,u8", T.FRONT_SHAPES)
def test_frontend_operands_are_exact(n, H, W, u8):
    import numpy as np
    import torch.nn.functional as Fn
    ops = T.front_operands(n, H, W, u8)
    ref = E.assert_exact_under(E.frontend_ref, ops, F16)                 # fp16 image tile, intermediates and folded weights (+ stem shift)
    img = E.frontend_image(ops)
    assert (img != 0).all() and torch.equal(img, img.float().to(F16).double())
    if u8:                                                               # the uint8 path as oracle/preprocess.py states it, in fp32: the same numbers
        from oracle import preprocess as opre
        pre = np.stack([opre.preprocess(f.numpy(), (H, W), np.float32(E.FRONT_MEAN), np.float32(E.FRONT_STDS)) for f in ops["frames"]])
        assert torch.equal(torch.from_numpy(pre).double(), img)
        assert all(float(m) == round(m) for m in E.FRONT_MEAN) and all(np.log2(s) == round(np.log2(s)) for s in E.FRONT_STDS)
    h = img
    for li, (wt, sc, sh, stride, pad) in enumerate(ops["layers"]):       # the unfold form of the reference == torch's convolutions
        assert (wt != 0).reshape(wt.shape[0], -1).any(0).all()           # every (input channel, tap) is used
        pre = Fn.conv2d(h, wt.double(), None, stride=stride, padding=pad) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
        assert float(pre.min()) >= 0                                     # LeakyReLU on, and the identity
        h = Fn.leaky_relu(pre, 0.01)
    assert torch.equal(h, ref)
    w0 = ops["layers"][1][0]
    assert (w0.sum(1) == 0).all() and ((w0 != 0).sum((1, 2, 3)) == 16).all()      # (+1, -1) pairs inside a tap: the common shift cancels
