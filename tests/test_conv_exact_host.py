"""CPU tests of tests/conv_exact.py: the premise of tests/test_gpu_conv_exact.py.  For every case of the matrix the GPU file
launches: the operands are exact in fp32 in any summation order (direct sums: the reference with fp32 accumulation in a
scrambled chunk order gives the same bits; Winograd: an fp32 emulation of the transform path with the product's packed U, in two
scrambled channel orders and the kernels' output grouping, equals the direct float64 convolution, and the order-independent
bound holds), and the torch.equal comparison sees every structural error of the sensitivity table.  conv_contract_ref itself is
checked against torch's convolution in float64 and against the loop form of the DCNv2 oracle."""
import pytest
import torch
import torch.nn.functional as Fn

import conv_exact as X
import exact_inputs as E

F64, F32 = torch.float64, torch.float32


def _operands_are_on_the_lattice(c, ops):
    assert (ops["x"] != 0).all() and (ops["weight"] != 0).all()
    if c["lattice"] != "direct":
        assert torch.equal(ops["weight"] / 9.0 * 2.0, (ops["weight"] / 9.0 * 2.0).round())      # multiples of 9 / 2
    if ops["scale"] is not None:
        assert torch.equal(torch.log2(ops["scale"]), torch.log2(ops["scale"]).round())
    if c["per_image"]:
        assert c["n"] == 2 and not torch.equal(ops["weight"][0], ops["weight"][1])


def _negative_branch_is_used(c, ref):
    """LeakyReLU cases compare both branches: some pre-activation of the exactly compared channels is negative, some is not."""
    if c["act"] == 1:
        pre = ref["pre"][:, :c["sig"]] if c["sig"] >= 0 else ref["pre"]
        assert bool((pre < 0).any()) and bool((pre > 0).any())
        neg = pre[pre < 0].to(F32)
        assert not torch.equal((neg * X.SLOPE32).to(F64), neg.to(F64) * 0.01)      # the fp32 multiply rounds: float64 * 0.01 would not do


def _sensitivity(c, ref):
    seen = {}
    for kind in X.ERRORS:
        if not X.applies(c, ref["ops"], kind):
            continue
        wrong = X.with_error(c, ref, kind)
        keep = slice(0, c["sig"]) if c["sig"] >= 0 else slice(None)      # the channels the GPU test compares exactly
        nd, msg = E.compare_exact(wrong[:, keep], ref["out"][:, keep].to(F64), F32, 1.0 / 256)
        assert nd > 0 and "first difference at" in msg, (c["name"], kind)
        seen[kind] = nd
    return seen


@pytest.mark.parametrize("c", X.DIRECT_CASES, ids=X.ids(X.DIRECT_CASES))
def test_direct_sum_case_is_exact_and_sensitive(c):
    ref = X.conv_contract_ref(c)
    _operands_are_on_the_lattice(c, ref["ops"])
    X.assert_exact_fp32(c, ref)
    assert float(ref["acc"].abs().max()) * 64 < 2 ** 24                  # quanta of 1/64 (deformable; 1/2 otherwise)
    _negative_branch_is_used(c, ref)
    seen = _sensitivity(c, ref)
    assert {"tap_dropped", "tap_one_column_off_first", "tap_one_column_off_last", "k_stage_dropped", "channels_swapped"} <= set(seen)
    assert ("dilation_ignored" in seen) == (c["dil"] > 1)


@pytest.mark.parametrize("c", X.WINOGRAD_CASES, ids=X.ids(X.WINOGRAD_CASES))
def test_winograd_case_is_exact_and_sensitive(c):
    ref = X.conv_contract_ref(c)
    ops = ref["ops"]
    _operands_are_on_the_lattice(c, ops)
    assert (c["lattice"] == "w44a") == (c["family"] != "w22" and c["cin"] <= 64)
    for seed in (1, 2):                                                   # two scrambled channel orders
        acc, bound = X.winograd_emulation(c, ops, seed)
        nd, msg = E.compare_exact(acc.to(F32), ref["acc"], F32, 1.0 / 128)
        assert nd == 0, (c["name"], msg)
        assert bound < 2 ** 24, (c["name"], bound)
    for key in ("acc", "pre"):
        assert torch.equal(ref[key], ref[key].to(F32).to(F64))
    _negative_branch_is_used(c, ref)
    seen = _sensitivity(c, ref)
    assert {"tap_dropped", "tap_one_column_off_first", "tap_one_column_off_last", "k_stage_dropped", "channels_swapped"} <= set(seen)


def test_pack_wino44_residues_do_not_reach_the_sum():
    """pack_wino44 computes U in float64 from a G whose sixths are not float64 numbers: where the exact U is 0 it leaves a residue
    of about 1e-16.  On the lattices used here every such residue is far below half a quantum of the fp32 partial sums it joins
    (the emulation above, which transforms with the packer's U, is what would notice otherwise); this pins their size."""
    c = next(k for k in X.W44 if k["lattice"] == "w44a")
    u = X.unpack_u(c, X.operands(c)["weight"][0]).to(F64)
    off = (u * 128 - (u * 128).round()).abs()
    assert float(off.max()) < 1e-9
    c = next(k for k in X.W44 if k["lattice"] == "w44b")
    u = X.unpack_u(c, X.operands(c)["weight"][0]).to(F64)
    assert float((u * 64 - (u * 64).round()).abs().max()) < 1e-9


# ---- conv_contract_ref itself --------------------------------------------------------------------------------------------------
def _random_ops(c, seed):
    g = E._gen(seed)
    ops = X.operands(c)
    for key, v in ops.items():
        if v is not None and key not in ("off", "mask"):
            ops[key] = torch.randn(v.shape, generator=g)
    if c["deform"]:
        ops["off"] = torch.randn(ops["off"].shape, generator=g) * 2.0
        ops["mask"] = torch.rand(ops["mask"].shape, generator=g)
    return ops


def _torch_ref(c, ops):
    outs = []
    for i in range(c["n"]):
        wt = ops["weight"][i if c["per_image"] else 0].double()
        outs.append(Fn.conv2d(ops["x"][i:i + 1].double(), wt, None, c["stride"], c["pad"], c["dil"]))
    y = torch.cat(outs)
    sc = 1.0 if ops["scale"] is None else ops["scale"].double().view(1, -1, 1, 1)
    sh = 0.0 if ops["shift"] is None else ops["shift"].double().view(1, -1, 1, 1)
    r = 0.0 if ops["res"] is None else ops["res"].double()
    y = (y + r) * sc + sh if c["res_mode"] == 1 else y * sc + sh + r
    if c["act"] == 1:
        y = Fn.leaky_relu(y, 0.01)
    if c["sig"] >= 0:
        pre = (torch.cat(outs) * sc + sh + r)
        y = torch.cat([y[:, :c["sig"]], torch.sigmoid(pre[:, c["sig"]:])], 1)
    return y.permute(0, 2, 3, 1).reshape(-1, c["cout"])


PLAIN_FEATURES = [
    X.case("ref_3x3", "igemm", cin=16, cout=5, h=7, w=9, k=3, res_mode=0),
    X.case("ref_3x3_stride2_res1", "igemm", cin=16, cout=5, h=8, w=10, k=3, stride=2, res_mode=1),
    X.case("ref_3x3_dil2_pad2", "igemm", cin=16, cout=5, h=7, w=9, k=3, dil=2, res_mode=1, shift=0),
    X.case("ref_5x5_dil3_stride2_pad1", "igemm", cin=16, cout=5, h=17, w=19, k=5, dil=3, stride=2, pad=1, scale=0),
    X.case("ref_1x1_per_image", "igemm", cin=16, cout=7, h=4, w=5, per_image=1, res_mode=1, act=0),
    X.case("ref_3x3_per_image_sigmoid", "igemm", cin=16, cout=7, h=4, w=6, k=3, per_image=1, res_mode=0, sig=4),
    X.case("ref_1x1_nothing", "igemm", cin=16, cout=3, h=3, w=3, scale=0, shift=0, act=0),
]


@pytest.mark.parametrize("c", PLAIN_FEATURES, ids=X.ids(PLAIN_FEATURES))
def test_contract_reference_matches_torch_convolution(c):
    for seed in (1, 2):
        ops = _random_ops(c, seed)
        ref = X.conv_contract_ref(c, ops)
        want = _torch_ref(c, ops)
        assert (ref["out"].double() - want).abs().max().item() < 1e-5 * (1 + want.abs().max().item())


@pytest.mark.parametrize("stride,pad,dil", [(1, 1, 1), (2, 1, 1), (1, 2, 2)])
def test_contract_reference_matches_the_loop_form_of_the_dcn_oracle(stride, pad, dil):
    from oracle import dcn as odcn
    h, w = (10, 12) if stride == 2 else (7, 9)
    c = X.case("ref_dcn", "igemm", n=1, cin=16, cout=5, h=h, w=w, k=3, stride=stride, pad=pad, dil=dil, deform=1, scale=0, shift=0, act=0)
    for seed in (1, 2):
        ops = _random_ops(c, seed)
        ops["off"][0, 0, 0, 0], ops["off"][0, 1, 0, 0] = 0.0, 10.0
        ref = X.conv_contract_ref(c, ops)
        loop = odcn.dcn_v2_forward_numpy(ops["x"].numpy(), ops["off"].numpy(), ops["mask"].numpy(), ops["weight"][0].numpy(),
                                         torch.zeros(5).numpy(), stride, pad, dil)
        loop = torch.from_numpy(loop).double().permute(0, 2, 3, 1).reshape(-1, 5)
        assert (ref["acc"] - loop).abs().max().item() < 1e-4


# ---- the PLAN pins, without a GPU ------------------------------------------------------------------------------------------------
def _geometry_desc(c):
    """The descriptor of a case as the library's queries read it: sizes and flags, no buffers (a query dereferences none)."""
    from m3dssd_amd import _hip
    d = _hip.ConvDesc()
    d.N, d.H, d.W, d.Cin, d.in_cs = c["n"], c["h"], c["w"], c["cin"], c["cin"] + c["in_x"]
    d.Cout, d.Cout_pad, d.out_cs, d.out_nchw = c["cout"], c["cout_pad"], c["cout"] + c["out_x"], c["planar"]
    d.kh, d.kw, d.stride, d.pad, d.dil, d.Ho, d.Wo = c["k"], c["k"], c["stride"], c["pad"], c["dil"], c["ho"], c["wo"]
    d.act, d.sigmoid_from = c["act"], c["sig"]
    if c["per_image"]:
        d.wgt_img_stride = c["cout_pad"] * c["k"] * c["k"] * c["cin"]
    if c["deform"]:
        d.dcn_offmask, d.dcn_om_cs = 16, 32                 # (only "deformable or not" is read)
    return d


@pytest.mark.parametrize("c", [k for k in X.CASES if k["family"] != "l0"], ids=X.ids([k for k in X.CASES if k["family"] != "l0"]))
def test_the_queries_answer_the_pinned_form_without_a_gpu(c):
    """The queries are host functions of the descriptor: what tests/test_gpu_conv_exact.py asserts before every launch holds on a
    machine without a GPU too, so a moved threshold fails the CPU suite already."""
    import ctypes
    import test_gpu_conv_exact as T
    from m3dssd_amd import _hip
    L = _hip.lib()
    d = _geometry_desc(c)
    if c["family"] == "igemm":
        splits = T._plan(L.m3d_conv2d_splitk_plan, d)[0]
        assert T._tile(d) + ((splits,) if len(c["expect"]) == 4 else ()) == c["expect"]
    elif c["family"] == "wave":
        assert T._wave_width(d) == c["expect"]
    elif c["family"] == "w22":
        assert L.m3d_wino_conv3x3_variant(ctypes.byref(d)) == 0 and T._plan(L.m3d_wino_conv3x3_splitk_plan, d) == (1, 0)
    else:
        assert L.m3d_wino44_applicable(ctypes.byref(d)) == 1
        assert (L.m3d_wino44_kpair(ctypes.byref(d)), T._plan(L.m3d_wino44_splitk_plan, d)[0]) == c["expect"]


def test_per_image_weights_on_a_32_channel_tile_need_whole_128_row_tiles():
    """choose_tile of csrc/igemm_conv.hip used to answer bm = 64 for per-image weights with Ho*Wo % 128 == 64 on the 32-channel
    tiles too, which are instantiated with 128 rows only: the launch ran a 128-row tile over two images with the weights of the
    first.  Such a descriptor is refused; the 64- and 128-channel tiles keep their bm = 64 fall-back."""
    import ctypes
    from m3dssd_amd import _hip
    L = _hip.lib()
    t = [ctypes.c_int() for _ in range(4)]
    for c in X.IGEMM_PER_IMAGE_REFUSED:
        assert L.m3d_conv2d_tile(ctypes.byref(_geometry_desc(c)), *[ctypes.byref(v) for v in t]) != 0
        assert b"per-image weights" in L.m3d_last_error()
    bk16 = X.case("bk16", "igemm", h=8, w=8, cin=48, cout=64, per_image=1)              # Cin % 32 != 0: the (128, 32, 16) tile
    assert L.m3d_conv2d_tile(ctypes.byref(_geometry_desc(bk16)), *[ctypes.byref(v) for v in t]) != 0
    ok = X.case("bn64", "igemm", h=8, w=8, cout=64, per_image=1)
    assert L.m3d_conv2d_tile(ctypes.byref(_geometry_desc(ok)), *[ctypes.byref(v) for v in t]) == 0 and t[0].value == 64
