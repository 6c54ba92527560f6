"""GPU tests (-m gpu) of the bf16 box heads and ANAB attention at the needed pixels only: the row-list forms of the fused bf16 head
(``m3d_head_mlp2_bf16_forward_rows``) and of the one-launch bf16 attention (``m3d_anab_attend_bf16_rows``) against the dense
launches of the same library, and the bf16 plan's detection-only tail through ``PipelinedDetector`` / ``FrameDetector`` with
``sparse_heads=True`` against the eager ``detect_batch`` of the same bf16 module.  Every comparison is ``torch.equal``: there are
no tolerances in this file."""
import ctypes
import functools

import pytest
import torch

import poison
from gpu_common import _dev, _nhwc16, _stream
from m3dssd_amd import _hip, synth

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SENT = -7.25                       # what the outputs hold before a row-list launch (exact in bf16 and fp32)
PAST = 1 << 30                     # what the list buffer holds past n_rows: out of every buffer if read
COUT = 36


# ------------------------------------------------------------------------------------ head kernel
def _cu_count():
    """hipDeviceAttributeMultiprocessorCount of the device: the attribute the library's launcher splits between the heads."""
    return torch.cuda.get_device_properties(_dev()).multi_processor_count


@functools.lru_cache(maxsize=None)
def _head_operands(G, n, h, w):
    """Packed operands of G heads over one bf16 map with pixel stride 136 (as test_fused_head_mlp_bf16_matches_torch_chain packs
    them) and the dense launch's output: the reference of every list, computed once and left unchanged."""
    from m3dssd_amd.engine_bf16 import pack_head2
    dev = _dev()
    g = torch.Generator().manual_seed(G * 100 + h)
    r = lambda t: t.to(BF16).float()
    xin = _nhwc16(r(torch.randn(n, 128, h, w, generator=g)), 136)
    w1 = r(torch.randn(G, 256, 128, generator=g) / 128 ** 0.5)
    w2 = r(torch.randn(G, 256, 256, generator=g) / 16)
    w3 = r(torch.randn(G, COUT, 256, generator=g) / 16)
    aff = [torch.rand(G, c, generator=g) + 0.5 for c in (256, 256, COUT)]
    sh = [torch.randn(G, c, generator=g) * 0.1 for c in (256, 256, COUT)]
    pk = pack_head2([(w1[i], aff[0][i], sh[0][i], w2[i], aff[1][i], sh[1][i], w3[i], aff[2][i], sh[2][i]) for i in range(G)], dev)
    HW = h * w
    d = _hip.Head2Bf16Desc()
    d.inp, d.in_cs, d.M = xin.data_ptr(), 136, n * HW
    d.w1f, d.w2f, d.w3, d.t1, d.t2, d.t3 = (t.data_ptr() for t in pk)
    d.Cout, d.HW, d.groups = COUT, HW, G
    d.out_group_off, d.out_img_stride = COUT * HW, (G * COUT + 1) * HW       # one plane per image that no head owns
    dense = torch.full((n, G * COUT + 1, HW), SENT, device=dev)
    d.out = dense.data_ptr()
    _hip.check(_hip.lib().m3d_head_mlp2_bf16_forward(ctypes.byref(d), _stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(dense).all() and not (dense[:, :G * COUT] == SENT).any() and (dense[:, G * COUT] == SENT).all()
    return d, dense, (xin, pk)


def _check_head_lists(G, n, h, w, lists):
    L, dev = _hip.lib(), _dev()
    d, dense, _keep = _head_operands(G, n, h, w)
    M, HW = n * h * w, h * w
    rows_buf = torch.empty(M, device=dev, dtype=torch.int32)
    n_rows = torch.zeros(1, device=dev, dtype=torch.int32)
    out = torch.empty_like(dense)
    sent = torch.full_like(dense, SENT)
    try:
        d.out = out.data_ptr()
        for name, rows in lists.items():
            assert rows.numel() <= M and (rows.numel() < 2 or (rows[1:] > rows[:-1]).all()), name
            rows_buf.fill_(PAST)
            rows_buf[:rows.numel()] = rows.to(dev, torch.int32)
            n_rows.fill_(rows.numel())
            listed = torch.zeros(M, dtype=torch.bool, device=dev)
            listed[rows.to(dev)] = True
            want = torch.where(listed.view(n, 1, HW), dense, sent)
            want[:, G * COUT] = SENT
            first = None
            for rep in range(2):                                 # two launches in a row give the same bits
                out.fill_(SENT)
                _hip.check(L.m3d_head_mlp2_bf16_forward_rows(ctypes.byref(d), rows_buf.data_ptr(), n_rows.data_ptr(), _stream()))
                torch.cuda.synchronize()
                assert torch.equal(out, want), (name, rep)
                first = out.clone() if first is None else first
                assert torch.equal(out.view(torch.int32), first.view(torch.int32)), (name, rep)
    finally:
        d.out = dense.data_ptr()


def test_head_rows_equal_dense_at_listed_pixels_and_write_nothing_else():
    """B = 2, HW = 640, two heads: empty, one entry, around one tile, every pixel, and a tile that spans both images."""
    n, h, w = 2, 20, 32
    perm = torch.randperm(n * h * w, generator=torch.Generator().manual_seed(23))
    lists = {"n%d" % k: perm[:k].sort().values for k in (0, 1, 127, 128, 129)}
    lists["all"] = torch.arange(n * h * w)
    lists["straddle"] = torch.arange(600, 700)
    _check_head_lists(2, n, h, w, lists)


def test_head_rows_with_eleven_heads_take_a_second_tile_per_workgroup():
    """Eleven heads share the compute units (CUs // 11 workgroups per head), so a list of more tiles than that sends a workgroup
    through the prefetch path to a second tile: the random list is sized from the device's CU count (3 000 entries = 24 tiles
    against 23 workgroups on 256 CUs); the full list has 30 tiles."""
    n, h, w = 2, 30, 64
    M = n * h * w
    wgs = max(1, _cu_count() // 11)
    k = min(128 * wgs + 56, M - 1)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(29))
    lists = {"random": perm[:k].sort().values, "all": torch.arange(M)}
    if wgs < M // 128:
        assert (k + 127) // 128 > wgs                            # the list has more tiles than a head has workgroups
    _check_head_lists(11, n, h, w, lists)


def test_head_rows_refuses_a_null_list():
    L, dev = _hip.lib(), _dev()
    d, dense, _keep = _head_operands(2, 2, 20, 32)
    out = torch.full_like(dense, SENT)
    one = torch.zeros(1, device=dev, dtype=torch.int32)
    try:
        d.out = out.data_ptr()
        for rows, n in ((None, one.data_ptr()), (one.data_ptr(), None)):
            rc = L.m3d_head_mlp2_bf16_forward_rows(ctypes.byref(d), rows, n, _stream())
            assert rc == -1 and b"row list" in L.m3d_last_error()
    finally:
        d.out = dense.data_ptr()
    torch.cuda.synchronize()
    assert (out == SENT).all()


# ------------------------------------------------------------------------------------ attention kernel
AB, AHW, CK, CK_PAD, CV, KEYS, KEYS_PAD = 3, 256, 168, 192, 128, 337, 384


@functools.lru_cache(maxsize=None)
def _attn_inputs():
    """Random bf16 operands; khat rows and vhatT columns past `keys` are NaN (the kernel must ignore them)."""
    dev = _dev()
    g = torch.Generator().manual_seed(41)
    q = torch.zeros(AB * AHW, CK_PAD)
    q[:, :CK] = torch.randn(AB * AHW, CK, generator=g) * 0.3
    khat = torch.zeros(AB, KEYS_PAD, CK_PAD)
    khat[:, :, :CK] = torch.randn(AB, KEYS_PAD, CK, generator=g)
    khat[:, KEYS:] = float("nan")
    vhatT = torch.randn(AB, CV, KEYS_PAD, generator=g)
    vhatT[:, :, KEYS:] = float("nan")
    res = torch.randn(AB * AHW, CV, generator=g)
    scale, shift = (torch.rand(CV, generator=g) + 0.5).to(dev), (torch.randn(CV, generator=g) * 0.2).to(dev)
    return tuple(t.to(BF16).to(dev).contiguous() for t in (q, khat, vhatT, res)) + (scale, shift)


def _attn_launch(fn, on, out, *row_list):
    q, khat, vhatT, res, scale, shift = _attn_inputs()
    rp, sp, hp = (res.data_ptr(), scale.data_ptr(), shift.data_ptr()) if on else (None, None, None)
    _hip.check(fn(q.data_ptr(), CK_PAD, khat.data_ptr(), vhatT.data_ptr(), AB, AHW, CK_PAD, KEYS, KEYS_PAD, CV, rp, CV if on else 0,
                  sp, hp, 1 if on else 0, out.data_ptr(), CV, *row_list, _stream()))
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _attn_dense(on):
    out = torch.full((AB * AHW, CV), SENT, device=_dev(), dtype=BF16)
    _attn_launch(_hip.lib().m3d_anab_attend_bf16, on, out)
    assert torch.isfinite(out.float()).all()
    return out


def _attn_row_lists():
    """The lists of tests/test_gpu_anab_rows.py."""
    g = torch.Generator().manual_seed(17)
    perm = torch.randperm(AB * AHW, generator=g)
    lists = {"n%d" % n: perm[:n].sort().values for n in (0, 1, 31, 32, 33, 127, 128, 129)}
    lists["all"] = torch.arange(AB * AHW)
    lists["straddle"] = torch.arange(200, 300)                    # its first 128 entries span images 0 and 1
    lists["no_image_1"] = torch.cat([perm[perm < AHW][:40], perm[perm >= 2 * AHW][:50]]).sort().values
    lists["three_per_image"] = torch.tensor([5, 100, 255, 256, 300, 511, 512, 640, 767])      # 9 entries, three images
    return lists


@pytest.mark.parametrize("on", [True, False])
def test_attend_rows_equal_dense_at_listed_pixels_and_write_nothing_else(on):
    """Residual, affine and LeakyReLU all on / all off."""
    L, dev = _hip.lib(), _dev()
    dense = _attn_dense(on)
    rows_buf = torch.empty(AB * AHW, device=dev, dtype=torch.int32)
    n_rows = torch.zeros(1, device=dev, dtype=torch.int32)
    out = torch.empty_like(dense)
    sent = torch.full_like(dense, SENT)
    for name, rows in _attn_row_lists().items():
        assert rows.numel() <= AB * AHW and (rows.numel() < 2 or (rows[1:] > rows[:-1]).all()), name
        rows_buf.fill_(PAST)
        rows_buf[:rows.numel()] = rows.to(dev, torch.int32)
        n_rows.fill_(rows.numel())
        listed = torch.zeros(AB * AHW, dtype=torch.bool, device=dev)
        listed[rows.to(dev)] = True
        want = torch.where(listed[:, None], dense, sent)
        out.fill_(SENT)
        _attn_launch(L.m3d_anab_attend_bf16_rows, on, out, rows_buf.data_ptr(), n_rows.data_ptr())
        assert torch.equal(out.view(torch.int16), want.view(torch.int16)), name


def test_attend_rows_refuses_a_null_list():
    L, dev = _hip.lib(), _dev()
    q, khat, vhatT, res, scale, shift = _attn_inputs()
    out = torch.full((AB * AHW, CV), SENT, device=dev, dtype=BF16)
    one = torch.zeros(1, device=dev, dtype=torch.int32)
    for rows, n in ((None, one.data_ptr()), (one.data_ptr(), None)):
        rc = L.m3d_anab_attend_bf16_rows(q.data_ptr(), CK_PAD, khat.data_ptr(), vhatT.data_ptr(), AB, AHW, CK_PAD, KEYS, KEYS_PAD, CV,
                                         None, 0, None, None, 0, out.data_ptr(), CV, rows, n, _stream())
        assert rc == -1 and b"row list" in L.m3d_last_error()
    torch.cuda.synchronize()
    assert (out == SENT).all()


# ------------------------------------------------------------------------------------ end to end
CROP = (128, 320)
B = 2
CONFIGS = ["base", "anab", "anab_fullalign"]


def _net(config, k):
    from model.M3d_inference_align import build
    flags = synth.config_flags(config)
    conf = synth.synth_conf(CROP, 0, batch_size=B, device="cuda:0", **flags)
    conf.nms_topN_pre = k
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0, **flags), strict=True)
    return net.to(_dev()).set_compute_dtype("bf16"), conf


def _batches():
    return [synth.synth_frames(B, CROP, s).to(_dev()) for s in (1234, 3, 4, 5)]


def _run_detectors(net, conf, xs):
    """Detections of the four batches from PipelinedDetector and FrameDetector with sparse heads, and the n_rows each left."""
    from m3dssd_amd.pipeline import FrameDetector, PipelinedDetector
    plan = net.engine().plan_for(B, *CROP)
    pipe = PipelinedDetector(net, conf, B, *CROP, sparse_heads=True)
    assert pipe.sparse_heads
    got_p = []
    for x in xs:
        r = pipe.step(x)
        if r is not None:
            got_p.append((r[0].clone(), r[1].clone()))
    r = pipe.flush()
    got_p.append((r[0].clone(), r[1].clone()))
    n_p = int(plan.named["n_rows"].item())
    fd = FrameDetector(net, conf, *CROP, batch=B, sparse_heads=True)
    assert fd.sparse_heads
    got_f = []
    for x in xs:
        r = fd.detect(x)
        got_f.append((r[0].clone(), r[1].clone()))
    n_f = int(plan.named["n_rows"].item())
    return got_p, got_f, (n_p, n_f)


@pytest.mark.parametrize("k", [200, 3000])
@pytest.mark.parametrize("config", CONFIGS)
def test_bf16_detectors_with_sparse_heads_equal_detect_batch(config, k):
    """Four different batches in a row: the staging rows that the previous batch left at pixels this batch does not need must not
    reach its detections."""
    from lib.rpn_util import detect_batch
    from m3dssd_amd.engine_bf16 import EngineBF16
    net, conf = _net(config, k)
    eng = net.engine()
    assert isinstance(eng, EngineBF16)
    plan = eng.plan_for(B, *CROP)
    with_center = synth.config_flags(config).get("center_align", True)
    # the tail replaces exactly the ops between anchor_select and bundle_outputs, one selection pass in front
    assert [op[0] for op in plan.tail] == ["need_rows"] + [op[0] for op in plan.ops[plan.tail_start:-1]]
    assert plan.ops[plan.tail_start - 1][0] == "anchor_select" and plan.ops[-1][0] == "bundle_outputs"
    n_sparse = 0
    for dense_op, tail_op in zip(plan.ops[plan.tail_start:-1], plan.tail[1:]):
        dense_here = with_center and dense_op[0] == "bbox_x3d+bbox_y3d.mlp"
        if (dense_op[1] == "bf16_head2" and not dense_here) or dense_op[0] == "anab.attend":
            assert tail_op[3] is not dense_op[3], dense_op[0]    # the tail holds a launch of its own, not the dense op
            n_sparse += 1
        elif dense_op[0] != "center_align2d.offsets":
            assert tail_op is dense_op, dense_op[0]
    assert n_sparse >= 1
    xs = _batches()
    ref = []
    for x in xs:
        d, c = detect_batch(net, x, conf)
        ref.append((d.clone(), c.clone()))
    assert sum(int(c.sum()) for _, c in ref) > 0
    got_p, got_f, n = _run_detectors(net, conf, xs)
    for got in (got_p, got_f):
        assert len(got) == len(ref)
        for (gd, gc), (rd, rc) in zip(got, ref):
            assert torch.equal(gc, rc) and torch.equal(gd, rd)
    assert all(0 < v < B * (CROP[0] // 8) * (CROP[1] // 8) for v in n), n   # the list was short: the heads did not run dense


def test_bf16_sparse_detectors_do_not_depend_on_unwritten_memory():
    """The full configuration under the three fills of tests/poison.py: the box staging and feats_gl at the unneeded pixels and the
    selection workspace hold the fill; the three results are equal."""
    xs = _batches()
    results = []
    for fill in poison.FILLS:
        with poison.poisoned_allocations(fill) as stats:
            net, conf = _net("anab_fullalign", 3000)
            got_p, got_f, _ = _run_detectors(net, conf, xs)
        assert stats.from_file("m3dssd_amd/engine_bf16.py") > 0
        results.append(got_p + got_f)
    for other in results[1:]:
        for (d0, c0), (d1, c1) in zip(results[0], other):
            assert torch.equal(c0, c1) and torch.equal(d0, d1)


def test_bf16_plans_carry_a_tail_and_their_ops_are_unchanged(monkeypatch):
    """Plan-level, no forward: both shipped sizes carry a tail, sparse_heads=None follows the measured default, and plan.ops is,
    name for name and kind for kind, what the plan builder gives with the tail switched off (engine_bf16.SPARSE_TAIL)."""
    from m3dssd_amd import engine_bf16 as E16
    net, conf = _net("anab_fullalign", 3000)
    eng = net.engine()
    with_tail = [eng.plan_for(1, 128, 320), eng.plan_for(1, 384, 1280)]
    # sparse_heads=None: the fp32 rule (3000 rows can touch all 640 pixels of the small crop, at most 3000 of 7680 of the large one);
    # M3D_BF16_SPARSE_HEADS overrides it either way
    monkeypatch.setattr(E16, "SPARSE_HEADS", None)
    assert [eng.sparse_heads_default(p, 3000) for p in with_tail] == [False, True]
    assert eng.sparse_heads_default(with_tail[0], 200) is True
    monkeypatch.setattr(E16, "SPARSE_HEADS", "0")
    assert [eng.sparse_heads_default(p, 200) for p in with_tail] == [False, False]
    monkeypatch.setattr(E16, "SPARSE_HEADS", "1")
    assert [eng.sparse_heads_default(p, 3000) for p in with_tail] == [True, True]
    monkeypatch.setattr(E16, "SPARSE_TAIL", False)
    net0, _ = _net("anab_fullalign", 3000)
    eng0 = net0.engine()
    without = [eng0.plan_for(1, 128, 320), eng0.plan_for(1, 384, 1280)]
    for plan, plan0 in zip(with_tail, without):
        assert plan.tail is not None and plan0.tail is None
        assert [(op[0], op[1]) for op in plan.ops] == [(op[0], op[1]) for op in plan0.ops]
        assert plan.branches == plan0.branches
        assert plan.ops[plan.tail_start - 1][0] == "anchor_select" and plan.ops[-1][0] == "bundle_outputs"
        assert [op[0] for op in plan.tail] == ["need_rows"] + [op[0] for op in plan.ops[plan.tail_start:-1]]
        for name in ("need", "need_rows", "n_rows", "need_thresh", "sparse_k"):
            assert name in plan.named and name not in plan0.named
