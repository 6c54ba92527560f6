"""GPU tests (-m gpu) of the box heads at the needed pixels only: ``m3d_need_rows`` against torch, the row-list form of the fused
head kernel (``m3d_head_mlp_forward_rows``) and the gated centre offsets (``m3d_align_offsets_gated``) against the library's dense
calls, and ``PipelinedDetector`` / ``FrameDetector`` with ``sparse_heads=True`` against the eager ``detect_batch``.  Every
comparison is ``torch.equal``: the references are torch and the unchanged dense path, so there are no tolerances in this file."""
import ctypes

import pytest
import torch

import poison
from gpu_common import _dev, _stream
from m3dssd_amd import _hip, synth

pytestmark = pytest.mark.gpu

B, A, HW = 2, 36, 640
SENT = -7.25                       # what the output planes hold before a row-list launch


# ------------------------------------------------------------------------------------ m3d_need_rows
def _keys(seed):
    """[B][A*HW] u32 keys (as int64) drawn from 160 values, so every value is held by ~140 rows and every rank falls into a tie:
    30 values that differ in the low 10 bits only, 30 that share the top 11 bits, 100 anywhere."""
    g = torch.Generator().manual_seed(seed)
    pool = torch.cat([0xBF7FFC00 + torch.randperm(1024, generator=g)[:30],
                      0xBF600000 + torch.randint(0, 1 << 20, (30,), generator=g),
                      torch.randint(0, 1 << 32, (100,), generator=g)])
    return pool[torch.randint(0, pool.numel(), (B, A * HW), generator=g)]


def _need_rows(keys_dev, k, ws_fill=None):
    L, dev = _hip.lib(), keys_dev.device
    nb = L.m3d_need_rows_workspace_bytes(B, HW)
    ws = torch.zeros(nb, device=dev, dtype=torch.uint8) if ws_fill is None else torch.full((nb,), ws_fill, device=dev, dtype=torch.uint8)
    thresh = torch.full((B,), 12345, device=dev, dtype=torch.int32)
    need = torch.full((B * HW,), 7, device=dev, dtype=torch.uint8)
    rows = torch.full((B * HW,), -1, device=dev, dtype=torch.int32)
    n_rows = torch.full((1,), -5, device=dev, dtype=torch.int32)
    _hip.check(L.m3d_need_rows(keys_dev.data_ptr(), B, A, HW, k, thresh.data_ptr(), need.data_ptr(), rows.data_ptr(),
                               n_rows.data_ptr(), ws.data_ptr(), nb, _stream()))
    torch.cuda.synchronize()
    return thresh.cpu(), need.cpu(), rows.cpu(), int(n_rows.item())


@pytest.mark.parametrize("k", [1, 100, 3000, A * HW])
def test_need_rows_matches_torch(k):
    keys = _keys(5)
    kd = (keys - (keys >= (1 << 31)) * (1 << 32)).to(torch.int32).to(_dev())
    kth = keys.sort(dim=1, descending=True).values[:, k - 1]                   # [B]
    if k < A * HW:
        assert ((keys >= kth[:, None]).sum(1) > k).all(), "the case is meant to have a tie at rank k"
    want_need = (keys.view(B, A, HW) >= kth[:, None, None]).any(1).reshape(-1)
    want_rows = torch.nonzero(want_need).reshape(-1).to(torch.int32)           # b * HW + pix, ascending
    if k == A * HW:
        assert want_need.all()
    for fill in (None, 0xFF):                                                   # 0xFF: a workspace of NaN bytes
        thresh, need, rows, n = _need_rows(kd, k, fill)
        assert torch.equal(thresh.to(torch.int64) & 0xFFFFFFFF, kth)
        assert torch.equal(need, want_need.to(torch.uint8))
        assert n == want_rows.numel()
        assert torch.equal(rows[:n], want_rows)
        assert (rows[n:] == -1).all()                                           # nothing written past the list


# ------------------------------------------------------------------------------------ row-list form of the fused head
def _head(seed, cin, dev, cout=36, h=20, w=32):
    """A three-layer head cin -> 256 -> 256 -> cout on an NHWC slice [B*h*w][cin + 8]: (MlpDesc, output planes, keep-alive)."""
    from m3dssd_amd.engine import pack_frag
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * h * w, cin + 8, generator=g).to(dev)
    d = _hip.MlpDesc()
    keep = [x]
    d.inp, d.in_cs, d.M, d.Cin = x.data_ptr(), cin + 8, B * h * w, cin
    chans = [cin, 256, 256, cout]
    for li, slot in enumerate("123"):
        ci, co = chans[li], chans[li + 1]
        wp = pack_frag(torch.randn(co, ci, generator=g) / ci ** 0.5, 64 if li == 2 else 256, dev)
        sc, sh = (torch.rand(co, generator=g) + 0.5).to(dev), (torch.randn(co, generator=g) * 0.2).to(dev)
        keep += [wp, sc, sh]
        setattr(d, "w" + slot, wp.data_ptr())
        setattr(d, "s" + slot, sc.data_ptr())
        setattr(d, "t" + slot, sh.data_ptr())
    out = torch.full((B, cout, h * w), SENT, device=dev)
    d.Cout, d.Cout_pad, d.out, d.out_img_stride, d.HW = cout, 64, out.data_ptr(), cout * h * w, h * w
    return d, out, keep


def _row_lists():
    g = torch.Generator().manual_seed(11)
    perm = torch.randperm(B * HW, generator=g)
    lists = {n: perm[:n].sort().values for n in (0, 1, 63, 64, 65)}
    lists["all"] = torch.arange(B * HW)
    lists["straddle"] = torch.arange(600, 700)            # its first tile holds pixels 600 .. 639 of image 0 and 0 .. 23 of image 1
    return lists


@pytest.mark.parametrize("cin", [128, 256])
def test_head_rows_equal_dense_at_listed_pixels_and_write_nothing_else(cin):
    L, dev = _hip.lib(), _dev()
    h0, h1 = _head(20 + cin, cin, dev), _head(21 + cin, cin, dev)
    arr = (_hip.MlpDesc * 2)(h0[0], h1[0])
    _hip.check(L.m3d_head_mlp_forward_batched(arr, 2, _stream()))
    torch.cuda.synchronize()
    dense = [h0[1].clone(), h1[1].clone()]
    assert not (dense[0] == SENT).any() and not (dense[1] == SENT).any()
    rows_buf = torch.full((B * HW,), 1 << 30, device=dev, dtype=torch.int32)     # entries past n_rows: out of every buffer if read
    n_rows = torch.zeros(1, device=dev, dtype=torch.int32)
    for name, rows in _row_lists().items():
        for mask in (0b11, 0b10):                          # both heads on the list; head 0 dense beside head 1 on the list
            rows_buf.fill_(1 << 30)
            rows_buf[:rows.numel()] = rows.to(dev, torch.int32)
            n_rows.fill_(rows.numel())
            for hd in (h0, h1):
                hd[1].fill_(SENT)
            _hip.check(L.m3d_head_mlp_forward_rows(arr, 2, rows_buf.data_ptr(), n_rows.data_ptr(), mask, _stream()))
            torch.cuda.synchronize()
            listed = torch.zeros(B * HW, dtype=torch.bool, device=dev)
            listed[rows.to(dev)] = True
            listed = listed.view(B, 1, HW).expand(B, 36, HW)
            for i, hd in enumerate((h0, h1)):
                if not (mask >> i) & 1:
                    assert torch.equal(hd[1], dense[i]), (name, mask, i)
                    continue
                want = torch.where(listed, dense[i], torch.full_like(dense[i], SENT))
                assert torch.equal(hd[1], want), (name, mask, i)


# ------------------------------------------------------------------------------------ gated centre offsets
def test_align_offsets_gated():
    L, dev = _hip.lib(), _dev()
    g = torch.Generator().manual_seed(3)
    sel_idx = torch.randint(0, A, (B * HW,), generator=g, dtype=torch.int32).to(dev)
    sel_prob = torch.rand(B * HW, generator=g).to(dev)
    box = torch.randn(B, 11, A, HW, generator=g).to(dev)
    wh = (torch.rand(A, 2, generator=g) * 4 + 0.5).to(dev)
    need = (torch.rand(B * HW, generator=g) < 0.4).to(torch.uint8).to(dev)
    assert 0 < int(need.sum()) < B * HW
    holes = box.clone()
    holes[(need == 0).view(B, 1, 1, HW).expand_as(box)] = float("nan")
    kx, ky, cs = 0, 1, 4
    args = (0.1, 0.9, -0.2, 1.1)

    def ptr(t, k):
        return t.data_ptr() + 4 * k * A * HW

    ref = torch.full((B * HW, cs), SENT, device=dev)
    _hip.check(L.m3d_align_offsets(1, sel_idx.data_ptr(), sel_prob.data_ptr(), 0.5, None, ptr(box, kx), ptr(box, ky), wh.data_ptr(),
                                   *args, ref.data_ptr(), cs, B, A, HW, 1, 11 * A * HW, _stream()))
    got = torch.full((B * HW, cs), SENT, device=dev)
    _hip.check(L.m3d_align_offsets_gated(sel_idx.data_ptr(), sel_prob.data_ptr(), 0.5, ptr(holes, kx), ptr(holes, ky), wh.data_ptr(),
                                         *args, need.data_ptr(), got.data_ptr(), cs, B, A, HW, 11 * A * HW, _stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    nd = need.bool()
    assert torch.equal(got[nd], ref[nd])
    assert (got[~nd][:, :2] == 0).all()
    assert torch.equal(got[~nd][:, 2], sel_prob[~nd])                     # the mask channel comes from sel_prob everywhere
    assert (got[:, 3] == SENT).all()                                       # the pad channel is not written


# ------------------------------------------------------------------------------------ end to end
CROP = (128, 320)
CASES = [("dla34", "base"), ("dla34", "anab"), ("dla34", "anab_fullalign"), ("dla102", "anab_fullalign")]


def _net(back_bone, config, k):
    from model.M3d_inference_align import build
    flags = synth.config_flags(config)
    conf = synth.synth_conf(CROP, 0, batch_size=B, device="cuda:0", back_bone=back_bone, **flags)
    conf.nms_topN_pre = k
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0, back_bone=back_bone, **flags), strict=True)
    return net.to(_dev()), conf


def _batches():
    return [synth.synth_frames(B, CROP, s).to(_dev()) for s in (1234, 3, 4, 5)]


def _run_detectors(net, conf, xs, crop=CROP, sparse_heads=True):
    """Detections of the batches xs from PipelinedDetector and FrameDetector with sparse heads (sparse_heads=False: dense), and
    the n_rows each left."""
    from m3dssd_amd.pipeline import FrameDetector, PipelinedDetector
    nb = xs[0].shape[0]
    plan = net.engine().plan_for(nb, *crop)
    pipe = PipelinedDetector(net, conf, nb, *crop, sparse_heads=sparse_heads)
    assert pipe.sparse_heads == sparse_heads
    got_p = []
    for x in xs:
        r = pipe.step(x)
        if r is not None:
            got_p.append((r[0].clone(), r[1].clone()))
    r = pipe.flush()
    got_p.append((r[0].clone(), r[1].clone()))
    n_p = int(plan.named["n_rows"].item())
    fd = FrameDetector(net, conf, *crop, batch=nb, sparse_heads=sparse_heads)
    assert fd.sparse_heads == sparse_heads
    got_f = []
    for x in xs:
        r = fd.detect(x)
        got_f.append((r[0].clone(), r[1].clone()))
    n_f = int(plan.named["n_rows"].item())
    return got_p, got_f, (n_p, n_f)


@pytest.mark.parametrize("k", [200, 3000])
@pytest.mark.parametrize("back_bone,config", CASES)
def test_detectors_with_sparse_heads_equal_detect_batch(back_bone, config, k):
    """Four different batches in a row: the staging rows that the previous batch left at pixels this batch does not need must not
    reach its detections."""
    from lib.rpn_util import detect_batch
    net, conf = _net(back_bone, config, k)
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


def test_sparse_detectors_do_not_depend_on_unwritten_memory():
    """The full configuration under the three fills of tests/poison.py: the box staging at the unneeded pixels and the selection
    workspace hold the fill; the three results are equal."""
    xs = _batches()
    results = []
    for fill in poison.FILLS:
        with poison.poisoned_allocations(fill) as stats:
            net, conf = _net("dla34", "anab_fullalign", 3000)
            got_p, got_f, _ = _run_detectors(net, conf, xs)
        assert stats.from_file("m3dssd_amd/engine.py") > 0
        results.append(got_p + got_f)
    for other in results[1:]:
        for (d0, c0), (d1, c1) in zip(results[0], other):
            assert torch.equal(c0, c1) and torch.equal(d0, d1)


def test_sparse_heads_none_follows_the_plan_rule():
    """Plan-level, no forward: 3000 rows can touch every one of the 640 pixels of a 128x320 crop (dense), but at most 3000 of the
    7680 pixels of 384x1280 (tail)."""
    net, conf = _net("dla34", "anab_fullalign", 3000)
    eng = net.engine()
    small, large = eng.plan_for(1, 128, 320), eng.plan_for(1, 384, 1280)
    assert small.tail is not None and large.tail is not None
    assert eng.sparse_heads_default(small, conf.nms_topN_pre) is False
    assert eng.sparse_heads_default(large, conf.nms_topN_pre) is True
    assert eng.sparse_heads_default(small, 200) is True
    # the tail replaces exactly the ops between anchor_select and bundle_outputs, one selection pass in front
    for plan in (small, large):
        assert plan.ops[plan.tail_start - 1][0] == "anchor_select" and plan.ops[-1][0] == "bundle_outputs"
        assert [op[0] for op in plan.tail] == ["need_rows"] + [op[0] for op in plan.ops[plan.tail_start:-1]]
