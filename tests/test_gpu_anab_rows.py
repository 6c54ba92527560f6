"""GPU tests (-m gpu) of the ANAB attention at the needed pixels only: the row-list form of the one-launch fp32 attention
(``m3d_anab_attend_f32_rows``) against the dense launch of the same library, and the detection-only tail that uses it against the
dense plan and the eager ``detect_batch``.  Every comparison is ``torch.equal``: there are no tolerances in this file."""
import functools

import pytest
import torch

from gpu_common import _dev, _stream
from m3dssd_amd import _hip, synth

pytestmark = pytest.mark.gpu

B, HW, KEYS, KEYS_PAD = 3, 256, 337, 352
SENT = -7.25                       # what `out` holds before a row-list launch
PAST = 1 << 30                     # what the list buffer holds past n_rows: out of every buffer if read


# ------------------------------------------------------------------------------------ kernel level
@functools.lru_cache(maxsize=None)
def _inputs(ck, cv):
    """Random operands of one instantiation; khat rows and vhatT columns past `keys` are NaN (the kernel must ignore them)."""
    dev = _dev()
    g = torch.Generator().manual_seed(100 * ck + cv)
    ck_pad = (ck + 31) // 32 * 32
    q = (torch.randn(B * HW, ck_pad, generator=g) * 0.3).to(dev)
    khat = torch.randn(B, KEYS_PAD, ck_pad, generator=g)
    khat[:, KEYS:] = float("nan")
    vhatT = torch.randn(B, cv, KEYS_PAD, generator=g)
    vhatT[:, :, KEYS:] = float("nan")
    res = torch.randn(B * HW, cv, generator=g).to(dev)
    scale, shift = (torch.rand(cv, generator=g) + 0.5).to(dev), (torch.randn(cv, generator=g) * 0.2).to(dev)
    return q, khat.to(dev), vhatT.to(dev), res, scale, shift, ck_pad


def _launch(fn, ck, cv, res_mode, affine, out, *row_list):
    q, khat, vhatT, res, scale, shift, ck_pad = _inputs(ck, cv)
    sp, hp = (scale.data_ptr(), shift.data_ptr()) if affine else (None, None)
    _hip.check(fn(q.data_ptr(), ck_pad, khat.data_ptr(), ck_pad, vhatT.data_ptr(), B, HW, ck, KEYS, KEYS_PAD, cv, res.data_ptr(), cv,
                  res_mode, sp, hp, 1 if affine else 0, out.data_ptr(), cv, *row_list, _stream()))
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _dense(ck, cv, res_mode, affine):
    """The dense launch's output: the reference of every list, computed once and left unchanged."""
    out = torch.full((B * HW, cv), SENT, device=_dev())
    _launch(_hip.lib().m3d_anab_attend_f32, ck, cv, res_mode, affine, out)
    assert torch.isfinite(out).all() and not (out == SENT).any()
    return out


def _row_lists():
    g = torch.Generator().manual_seed(17)
    perm = torch.randperm(B * HW, generator=g)
    lists = {"n%d" % n: perm[:n].sort().values for n in (0, 1, 31, 32, 33, 127, 128, 129)}
    lists["all"] = torch.arange(B * HW)
    lists["straddle"] = torch.arange(200, 300)                    # its first 128 entries span images 0 and 1
    lists["no_image_1"] = torch.cat([perm[perm < HW][:40], perm[perm >= 2 * HW][:50]]).sort().values
    lists["three_per_image"] = torch.tensor([5, 100, 255, 256, 300, 511, 512, 640, 767])      # 9 entries, three images
    return lists


@pytest.mark.parametrize("res_mode,affine", [(0, False), (1, False), (0, True), (1, True)])
@pytest.mark.parametrize("ck,cv", [(168, 128), (64, 128), (168, 256)])
def test_rows_equal_dense_at_listed_pixels_and_write_nothing_else(ck, cv, res_mode, affine):
    L, dev = _hip.lib(), _dev()
    dense = _dense(ck, cv, res_mode, affine)
    rows_buf = torch.empty(B * HW, device=dev, dtype=torch.int32)
    n_rows = torch.zeros(1, device=dev, dtype=torch.int32)
    out = torch.empty_like(dense)
    sent = torch.full_like(dense, SENT)
    for name, rows in _row_lists().items():
        assert rows.numel() <= B * HW and (rows.numel() < 2 or (rows[1:] > rows[:-1]).all()), name
        rows_buf.fill_(PAST)
        rows_buf[:rows.numel()] = rows.to(dev, torch.int32)
        n_rows.fill_(rows.numel())
        listed = torch.zeros(B * HW, dtype=torch.bool, device=dev)
        listed[rows.to(dev)] = True
        want = torch.where(listed[:, None], dense, sent)
        first = None
        for rep in range(2):                                     # two launches in a row give the same bits
            out.fill_(SENT)
            _launch(L.m3d_anab_attend_f32_rows, ck, cv, res_mode, affine, out, rows_buf.data_ptr(), n_rows.data_ptr())
            assert torch.equal(out, want), (name, rep)
            first = out.clone() if first is None else first
            assert torch.equal(out.view(torch.int32), first.view(torch.int32)), (name, rep)


def test_rows_refuses_a_null_list():
    L, dev = _hip.lib(), _dev()
    out = torch.full((B * HW, 128), SENT, device=dev)
    q, khat, vhatT, res, scale, shift, ck_pad = _inputs(64, 128)
    one = torch.zeros(1, device=dev, dtype=torch.int32)
    for rows, n in ((None, one.data_ptr()), (one.data_ptr(), None)):
        rc = L.m3d_anab_attend_f32_rows(q.data_ptr(), ck_pad, khat.data_ptr(), ck_pad, vhatT.data_ptr(), B, HW, 64, KEYS, KEYS_PAD, 128,
                                        None, 0, 0, None, None, 0, out.data_ptr(), 128, rows, n, _stream())
        assert rc == -1 and b"row list" in L.m3d_last_error()
    torch.cuda.synchronize()
    assert (out == SENT).all()


# ------------------------------------------------------------------------------------ engine level
CROP = (128, 320)                  # the crop of tests/test_gpu_sparse_heads.py: 640 pixels, five attention tiles per image
EB, K = 2, 200
CASES = [("dla34", "anab_fullalign"), ("dla34", "anab"), ("dla102", "anab_fullalign")]


def _net(back_bone, config):
    from model.M3d_inference_align import build
    flags = synth.config_flags(config)
    conf = synth.synth_conf(CROP, 0, batch_size=EB, device="cuda:0", back_bone=back_bone, **flags)
    conf.nms_topN_pre = K
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0, back_bone=back_bone, **flags), strict=True)
    return net.to(_dev()), conf


@pytest.mark.parametrize("prefill_nan", [False, True])
@pytest.mark.parametrize("back_bone,config", CASES)
def test_tail_attends_at_needed_pixels_only(back_bone, config, prefill_nan, monkeypatch):
    from lib.rpn_util import detect_batch
    from m3dssd_amd import engine as E
    from m3dssd_amd.pipeline import PipelinedDetector
    monkeypatch.setattr(E, "ANAB_ROWS", True)                    # (M3D_ANAB_ROWS: read when the plan is built)
    net, conf = _net(back_bone, config)
    xs = [synth.synth_frames(EB, CROP, s).to(_dev()) for s in (1234, 3)]
    eng = net.engine()
    plan = eng.plan_for(EB, *CROP)
    A, hw = eng.A, plan.feat[0] * plan.feat[1]
    names = [op[0] for op in plan.tail]
    assert "anab.attend" in names and names == ["need_rows"] + [op[0] for op in plan.ops[plan.tail_start:-1]]
    dense_op = next(op for op in plan.ops if op[0] == "anab.attend")
    tail_op = next(op for op in plan.tail if op[0] == "anab.attend")
    assert tail_op[3] is not dense_op[3]                         # the tail holds a launch of its own, not the dense op
    gl, box = plan.named["feats_gl"], plan.named["box_planar"]
    for x in xs:
        with torch.no_grad():
            eng.forward(x)                                       # the dense plan
        torch.cuda.synchronize()
        gl_dense, box_dense = gl.t.clone(), box.clone()
        if prefill_nan:
            gl.t.fill_(float("nan"))
        plan.named["input_ptr"][0] = x.data_ptr()
        plan.named["sparse_k"][0] = K
        eng.run_plan(plan, 0, len(plan.ops) - 1, tail=True)
        torch.cuda.synchronize()
        need = plan.named["need"].bool()
        n = int(plan.named["n_rows"].item())
        assert 0 < n == int(need.sum()) < EB * hw
        got, want = gl.t.view(EB * hw, gl.cs), gl_dense.view(EB * hw, gl.cs)
        assert torch.equal(got[need], want[need])
        if prefill_nan:
            assert torch.isnan(got[~need]).all()                 # the attention wrote the listed pixels and nothing else
        z_got, z_want = (t.view(EB, 11, A, hw)[:, 6].permute(0, 2, 1).reshape(EB * hw, A) for t in (box, box_dense))
        assert torch.equal(z_got[need], z_want[need])
    ref = []
    for x in xs:
        d, c = detect_batch(net, x, conf)
        ref.append((d.clone(), c.clone()))
    assert sum(int(c.sum()) for _, c in ref) > 0
    if prefill_nan:
        gl.t.fill_(float("nan"))
    pipe = PipelinedDetector(net, conf, EB, *CROP, sparse_heads=True)
    assert pipe.sparse_heads
    got = []
    for x in xs:
        r = pipe.step(x)
        if r is not None:
            got.append((r[0].clone(), r[1].clone()))
    r = pipe.flush()
    got.append((r[0].clone(), r[1].clone()))
    assert len(got) == len(ref)
    for (gd, gc), (rd, rc) in zip(got, ref):
        assert torch.equal(gc, rc) and torch.equal(gd, rd)
