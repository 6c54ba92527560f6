"""GPU tests (-m gpu) of the 3-D size, depth and angle heads behind the NMS: ``m3d_post_rows`` against its numpy restatement
(tests/post_nms_ref.py), ``m3d_topk_decode_planar_2d`` against ``m3d_topk_decode_planar``, ``m3d_fill_post_3d`` against the
selection of the full decode, and ``PipelinedDetector(defer_3d=True)`` against ``defer_3d=False`` and the eager ``detect_batch``.
Every comparison is ``torch.equal`` / ``np.array_equal``: the references are numpy on integers and the unchanged full path, so
there are no tolerances in this file."""
import types

import numpy as np
import pytest
import torch

import poison
import post_nms_ref as R
from gpu_common import _dev, _sortable_bits, _stream
from m3dssd_amd import _hip, synth
from m3dssd_amd.host.detect import select_block

pytestmark = pytest.mark.gpu

SENT = -77


# ------------------------------------------------------------------------------------ m3d_post_rows
@pytest.mark.parametrize("post", [1, 5, 40])
def test_post_rows_matches_numpy(post):
    B, HW, A, n = 3, 128, 4, 100
    L, dev = _hip.lib(), _dev()
    rows_out, keep, num = R.post_rows_case(B, HW, A, n)
    want = R.post_rows_ref(rows_out, keep, num, post, HW)
    assert 0 < want.size < B * post + 1
    d_rows_out, d_keep, d_num = (torch.from_numpy(a).to(dev) for a in (rows_out, keep, num))
    rows = torch.full((B * HW,), SENT, device=dev, dtype=torch.int32)
    n_rows = torch.full((1,), SENT, device=dev, dtype=torch.int32)
    for _ in range(2):                                     # twice into the same buffers: nothing carries over between calls
        _hip.check(L.m3d_post_rows(d_rows_out.data_ptr(), d_keep.data_ptr(), d_num.data_ptr(), B, n, post, HW, rows.data_ptr(),
                                   n_rows.data_ptr(), _stream()))
        torch.cuda.synchronize()
        got_n, got = int(n_rows.item()), rows.cpu().numpy()
        assert got_n == want.size
        assert np.array_equal(got[:got_n], want)
        assert (got[got_n:] == SENT).all()                 # nothing written past the list


def test_post_rows_with_no_kept_row_at_all():
    B, HW, n = 3, 128, 100
    L, dev = _hip.lib(), _dev()
    rows_out, keep, _ = R.post_rows_case(B, HW, 4, n)
    d_rows_out, d_keep = torch.from_numpy(rows_out).to(dev), torch.from_numpy(keep).to(dev)
    num = torch.zeros(B, device=dev, dtype=torch.int32)
    rows = torch.full((B * HW,), SENT, device=dev, dtype=torch.int32)
    n_rows = torch.full((1,), SENT, device=dev, dtype=torch.int32)
    _hip.check(L.m3d_post_rows(d_rows_out.data_ptr(), d_keep.data_ptr(), num.data_ptr(), B, n, 40, HW, rows.data_ptr(),
                               n_rows.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert int(n_rows.item()) == 0 and (rows == SENT).all()


# ------------------------------------------------------------------------------------ the 2-D decode and the fill
TB, TA, THW, TK = 2, 4, 128, 100


def _staging(seed=9):
    """Inputs of the planar decode for B = 2, A = 4, HW = 128: keys with ties, logits, box staging, rois, anchors, means / stds."""
    g = torch.Generator().manual_seed(seed)
    dev, R_ = _dev(), TA * THW
    scores = (torch.randint(0, 300, (TB, R_), generator=g).float() / 300.0)               # ~1.7 rows per value: ties at the cut
    bits = _sortable_bits(scores)
    bits = (bits - (bits >= (1 << 31)) * (1 << 32)).to(torch.int32).to(dev)
    cls = torch.randn(TB, 4 * TA, THW, generator=g).to(dev)
    box = (torch.randn(TB, 11, R_, generator=g) * 0.3).to(dev)
    x1, y1 = torch.rand(R_, generator=g) * 1000, torch.rand(R_, generator=g) * 300
    rois = torch.stack([x1, y1, x1 + 20 + torch.rand(R_, generator=g) * 80, y1 + 20 + torch.rand(R_, generator=g) * 60,
                        torch.randint(0, TA, (R_,), generator=g).float()], 1).to(dev)
    anchors = (torch.rand(TA, 9, generator=g) * 10 + 1).to(dev)
    means, stds = (torch.randn(11, generator=g) * 0.1).to(dev), (torch.rand(11, generator=g) + 0.5).to(dev)
    return types.SimpleNamespace(bits=bits, cls=cls, box=box, rois=rois, anchors=anchors, means=means, stds=stds)


def _decode(s, box, scale, two_d):
    L, dev = _hip.lib(), _dev()
    nb = L.m3d_topk_decode_workspace_bytes(TB, TA * THW)
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    aboxes = torch.full((TB, TK, 14), float(SENT), device=dev)
    rows_out = torch.full((TB, TK), SENT, device=dev, dtype=torch.int32)
    fn = L.m3d_topk_decode_planar_2d if two_d else L.m3d_topk_decode_planar
    _hip.check(fn(s.bits.data_ptr(), s.cls.data_ptr(), box.data_ptr(), s.rois.data_ptr(), s.anchors.data_ptr(), s.means.data_ptr(),
                  s.stds.data_ptr(), None if scale is None else scale.data_ptr(), aboxes.data_ptr(), rows_out.data_ptr(),
                  ws.data_ptr(), nb, TB, TA, THW, TK, _stream()))
    torch.cuda.synchronize()
    return aboxes, rows_out


def _nan_planes(box, keep_pixels=None):
    """`box` with planes 6..10 NaN (tests/poison.py's fill), except -- keep_pixels [B][HW] bool -- at those pixels under every anchor."""
    out = poison.poison_(torch.empty_like(box), "nan")
    assert torch.isnan(out).all()
    out[:, :6] = box[:, :6]
    if keep_pixels is not None:
        m = keep_pixels.view(TB, 1, 1, THW).expand(TB, 5, TA, THW).reshape(TB, 5, TA * THW)
        out[:, 6:] = torch.where(m, box[:, 6:], out[:, 6:])
    return out


@pytest.mark.parametrize("scaled", [False, True])
def test_decode_2d_equals_the_full_decode_outside_the_deferred_columns(scaled):
    s = _staging()
    scale = torch.tensor([1.0, 0.8], device=_dev()) if scaled else None
    full, rows_full = _decode(s, s.box, scale, False)
    assert torch.isfinite(full).all() and (full[:, :, 8:13] != 0).any()
    for box in (s.box, _nan_planes(s.box)):
        got, rows = _decode(s, box, scale, True)
        assert torch.equal(rows, rows_full)
        assert torch.equal(got[:, :, :8], full[:, :, :8]) and torch.equal(got[:, :, 13], full[:, :, 13])
        z = got[:, :, 8:13]
        assert (z == 0).all() and not torch.signbit(z).any()                              # +0.0


@pytest.mark.parametrize("post", [5, 40])
def test_fill_completes_the_selected_rows_bit_for_bit(post):
    L, dev = _hip.lib(), _dev()
    s = _staging()
    scale = torch.tensor([1.0, 0.8], device=dev)
    conf = types.SimpleNamespace(nms_topN_post=post)
    full, _ = _decode(s, s.box, scale, False)
    two_d, rows_out = _decode(s, _nan_planes(s.box), scale, True)
    g = torch.Generator().manual_seed(post)
    keep = torch.full((TB, TK), 1 << 28, dtype=torch.int32)                               # entries past num: never read
    num = torch.tensor([50, 3], dtype=torch.int32)                                         # 50 > both posts; 3 < both
    for b in range(TB):
        keep[b, :int(num[b])] = torch.randperm(TK, generator=g)[:int(num[b])].sort().values.to(torch.int32)
    keep, num = keep.to(dev), num.to(dev)
    want, want_counts = select_block(full, keep, num, conf)
    block, counts = select_block(two_d, keep, num, conf)
    assert torch.equal(counts, want_counts) and counts.tolist() == [min(50, post), 3]
    assert not torch.equal(block, want)
    # the staging holds planes 6..10 at the survivors' pixels and NaN everywhere else
    surv = torch.zeros(TB, THW, dtype=torch.bool, device=dev)
    for b in range(TB):
        sel = rows_out[b, keep[b, :int(counts[b])].long()].long()
        surv[b, sel % THW] = True
    box = _nan_planes(s.box, surv)
    assert torch.isnan(box[:, 6:]).any()
    _hip.check(L.m3d_fill_post_3d(box.data_ptr(), s.rois.data_ptr(), s.anchors.data_ptr(), s.means.data_ptr(), s.stds.data_ptr(),
                                  rows_out.data_ptr(), keep.data_ptr(), counts.data_ptr(), TB, TA, THW, TK, post, block.data_ptr(),
                                  _stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(block).all()
    assert torch.equal(block, want)                        # rows past the counts and the count row included


# ------------------------------------------------------------------------------------ end to end
CROP = (128, 320)
B = 2
PRE = 200
# The cases need every image of a batch to fill its block (count == post, post up to 40).  With the synthetic weights the NMS at
# the configuration's nms_thres = 0.4 keeps 13 .. 18 of the 200 decoded rows of an image, at 0.8 it keeps 70 .. 75 (the CPU
# restatement, oracle/detect.py, on the batches below), and among the first 40 of them two or more share a pixel: both the cut
# at `post` and the repeated pixels of m3d_post_rows are exercised.
NMS_THRES = 0.8
p2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884],
               [0.0, 0.0, 0.0, 1.0]])


def _net(config, post, back_bone="dla34"):
    from model.M3d_inference_align import build
    flags = synth.config_flags(config)
    conf = synth.synth_conf(CROP, 0, batch_size=B, device="cuda:0", back_bone=back_bone, **flags)
    conf.nms_topN_pre, conf.nms_topN_post, conf.nms_thres = PRE, post, NMS_THRES
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0, back_bone=back_bone, **flags), strict=True)
    return net.to(_dev()), conf


def _batches():
    return [synth.synth_frames(B, CROP, s).to(_dev()) for s in (1234, 3, 4)]


def _metas():
    return [{"p2": np.stack([p2, p2 * np.array([[1.0 + 0.01 * i], [1.0], [1.0], [1.0]])]),
             "scale": np.array([1.0, 0.9 - 0.1 * i], np.float32), "clip_wh": np.array([[0, 0], [300, 100 + i]], np.float32)}
            for i in range(3)]


def _run_pipe(net, conf, xs, defer_3d, refine=False, want_defer=None):
    """as_block results (block, counts[, refined]) of the batches xs: every step's and flush()'s."""
    from m3dssd_amd.pipeline import PipelinedDetector
    pipe = PipelinedDetector(net, conf, B, *CROP, sparse_heads=True, defer_3d=defer_3d, refine=refine)
    assert pipe.sparse_heads
    assert pipe.defer_3d == (defer_3d if want_defer is None else want_defer)
    got = []
    for x, m in zip(xs, _metas()):
        r = pipe.step(x, as_block=True, meta=m) if refine else pipe.step(x, as_block=True)
        if r is not None:
            got.append(tuple(t.clone() for t in r))
    got.append(tuple(t.clone() for t in pipe.flush(as_block=True)))
    assert pipe.flush() is None and len(got) == len(xs)
    return got


def _assert_same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for a, b in zip(g, w):
            assert torch.equal(a, b)


def _assert_blocks_fill(got, post):
    """Fails unless every image of at least one batch has count == post, and at least one image has two rows or more."""
    counts = [c.tolist() for _, c, *_ in got]
    assert any(all(v == post for v in c) for c in counts), counts
    assert any(v >= 2 for c in counts for v in c), counts


@pytest.mark.parametrize("post", [5, 40])
def test_deferred_heads_equal_the_one_part_tail_and_detect_batch(post):
    from lib.rpn_util import detect_batch
    net, conf = _net("anab_fullalign", post)
    plan = net.engine().plan_for(B, *CROP)
    assert plan.post3d is not None and plan.tail_pre is not None
    xs = _batches()
    ref = []
    for x in xs:
        d, c = detect_batch(net, x, conf)
        ref.append((d.clone(), c.clone()))
    on = _run_pipe(net, conf, xs, True)
    n_post = int(plan.post_n_rows.item())
    assert 0 < n_post <= B * post                           # the deferred launches ran on the survivors' list
    off = _run_pipe(net, conf, xs, False)
    _assert_same(on, off)
    _assert_blocks_fill(on, post)
    for (blk, cnt), (rd, rc) in zip(on, ref):
        assert torch.equal(cnt, rc) and torch.equal(blk[:, :-1], rd)
        assert torch.equal(blk[:, -1, 0], rc.float()) and (blk[:, -1, 1:] == 0).all()
        assert (blk[:, :-1, 8:13] != 0).any(dim=2).sum() == int(rc.sum())       # every selected row got its 3-D columns


def test_deferred_heads_with_refinement_and_per_image_scale():
    from m3dssd_amd.host.detect import detect_batch
    post = 40
    net, conf = _net("anab_fullalign", post)
    xs = _batches()
    on = _run_pipe(net, conf, xs, True, refine=True)
    off = _run_pipe(net, conf, xs, False, refine=True)
    _assert_same(on, off)
    _assert_blocks_fill(on, post)
    for (blk, cnt, refined), x, m in zip(on, xs, _metas()):
        d, c = detect_batch(net, x, conf, scale=m["scale"])
        assert torch.equal(cnt, c) and torch.equal(blk[:, :-1], d)
        assert float(refined[:, :, 0].sum()) > 0            # some rows were refined


@pytest.mark.parametrize("config", ["base", "anab"])
def test_declining_configurations_keep_the_one_part_tail(config):
    """The heads (and the attention) of these configurations read feats0, which the backbone of the next batch writes in front
    of the join: the plan offers no split, and defer_3d=True is the one-part tail bit for bit."""
    net, conf = _net(config, 40)
    plan = net.engine().plan_for(B, *CROP)
    assert plan.tail is not None and plan.deferred                # forms were registered, the rule declined them
    assert plan.post3d is None and plan.tail_pre is None and plan.post_rows is None
    xs = _batches()
    _assert_same(_run_pipe(net, conf, xs, True, want_defer=False), _run_pipe(net, conf, xs, False))


def test_the_rule_reads_the_buffers_of_the_full_configuration():
    """Plan-level: every map the deferred launches read is first written at or behind planar_first_op, and the split tail is the
    one-part tail minus the deferred launches, with the two 2-D size heads in the six-head launch's place."""
    net, conf = _net("anab_fullalign", 40)
    plan = net.engine().plan_for(B, *CROP)
    join = int(plan.named["planar_first_op"])
    assert plan.post3d_reads and all(w >= join for _, w in plan.post3d_reads)
    named = {(v if torch.is_tensor(v) else v.t).data_ptr() for k, v in plan.named.items()
             if k in ("feats_align3d", "feats_gl", "anab.khat", "anab.vhatT")}
    assert len(named) == 4
    assert named <= {t.data_ptr() for t, _ in plan.post3d_reads}
    tail, pre, post3d = ([op[0] for op in ops] for ops in (plan.tail, plan.tail_pre, plan.post3d))
    assert post3d == ["bbox_w3d+bbox_h3d+bbox_l3d+bbox_rY3d.mlp", "anab.attend", "bbox_z3d.mlp"]
    assert "bbox_w+bbox_h.mlp" in pre and "anab.qkvs" in pre and not set(post3d) & set(pre)
    assert len(pre) == len(tail) - 2 and [n for n in pre if n in tail] == [n for n in tail if n in pre]


def test_deferred_heads_do_not_depend_on_unwritten_memory():
    """The full configuration under the three fills of tests/poison.py: every plan buffer (the box staging, which the split tail
    writes at the needed / surviving pixels only, the two lists, feats_gl) holds the fill before the first replay."""
    xs = _batches()
    results = []
    for fill in poison.FILLS:
        with poison.poisoned_allocations(fill) as stats:
            net, conf = _net("anab_fullalign", 40)
            results.append(_run_pipe(net, conf, xs, True))
        assert stats.from_file("m3dssd_amd/engine.py") > 0
    for got in results:
        for blk, cnt in got:
            assert torch.isfinite(blk).all()
    _assert_blocks_fill(results[0], 40)
    for other in results[1:]:
        _assert_same(results[0], other)
