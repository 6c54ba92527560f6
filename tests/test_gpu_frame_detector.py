"""GPU tests (-m gpu) of the single-frame mode: the multi-workgroup top-k + decode (``m3d_topk_decode_planar_mw``) against the
single-workgroup kernel it has to reproduce bit for bit, and ``m3dssd_amd.pipeline.FrameDetector`` (one hipGraph per frame) against
the eager ``detect_batch`` / ``refine_detections``.  Exact equality everywhere: there are no tolerances in this file."""

import numpy as np
import pytest
import torch

from m3dssd_amd import _hip, synth
from gpu_common import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu

SENT = -559038737          # 0xDEADBEEF as int32
GUARD = 64                 # 4-byte elements on each side of every output


class Guarded:
    """n 4-byte elements on the device between two sentinel-filled guard regions."""

    def __init__(self, n, dtype=torch.float32):
        self.n = int(n)
        self.raw = torch.full((GUARD + self.n + GUARD,), SENT, dtype=torch.int32, device=_dev())
        self.t = self.raw[GUARD:GUARD + self.n].view(dtype)
        self.ptr = self.t.data_ptr()

    def check(self):
        raw = self.raw.cpu().numpy()
        assert (raw[:GUARD] == SENT).all(), "write below the buffer"
        assert (raw[GUARD + self.n:] == SENT).all(), "write beyond the buffer"


DISTS = ("all_equal", "16_levels", "ties_at_cut", "negative_and_zero", "skewed")
# (R, k): R = 1, 5, one not divisible by 4, 46 080, 276 480; k = 1, R (R <= 16384), 3000, 16 384
RK = [(1, 1), (5, 1), (5, 5), (10007, 1), (10007, 3000), (10007, 10007), (46080, 1), (46080, 3000), (46080, 16384),
      (276480, 3000), (276480, 16384)]
WGS = (1, 2, 7, 64, 0)     # R = 5: single keys, 7 slices -> a slice smaller than a workgroup and empty last slices
N_ANCH = 36


def _scores(name, B, R, k, g):
    if name == "all_equal":
        return torch.full((B, R), 0.731)
    if name == "16_levels":
        return torch.randint(0, 16, (B, R), generator=g).float() / 16.0
    if name == "ties_at_cut":
        s = torch.rand(B, R, generator=g)
        n_tie = min(R, max(2, min(8000, 2 * k)))               # a block of equal scores that the cut at k falls into
        for b in range(B):
            s[b, torch.randperm(R, generator=g)[:n_tie]] = 0.95
        return s
    if name == "negative_and_zero":
        s = torch.randn(B, R, generator=g)
        s[:, ::7] = 0.0
        s[:, 3::11] = -0.0
        return s
    return torch.rand(B, R, generator=g) ** 6                  # most rows near 0 like real fg probabilities


def _planar_inputs(B, R, g):
    """Planar staging with A = 1 (row = pixel): cls [B][4][R] logits, box [B][11][R]; rois / anchors / means / stds as the decode
    reads them.  The sort keys are given separately: the selection does not look at the logits."""
    dev = _dev()
    cls_pl = torch.randn(B, 4, R, generator=g)
    box_pl = torch.randn(B, 11, R, generator=g) * 0.3
    x1 = torch.rand(R, generator=g) * 1000
    y1 = torch.rand(R, generator=g) * 300
    rois = torch.stack([x1, y1, x1 + 20 + torch.rand(R, generator=g) * 80, y1 + 20 + torch.rand(R, generator=g) * 60,
                        torch.randint(0, N_ANCH, (R,), generator=g).float()], 1)
    anchors = torch.rand(N_ANCH, 9, generator=g) * 10 + 1
    means, stds = torch.randn(11, generator=g) * 0.1, torch.rand(11, generator=g) + 0.5
    return [t.to(dev).contiguous() for t in (cls_pl, box_pl, rois, anchors, means, stds)]


@pytest.mark.parametrize("R,k", RK)
@pytest.mark.parametrize("name", DISTS)
def test_topk_mw_equals_single_workgroup_kernel_and_stable_sort(name, R, k):
    """aboxes and rows_out of m3d_topk_decode_planar_mw == those of m3d_topk_decode_planar (torch.equal) for every workgroup count,
    rows == np.lexsort((row, -key))[:k]; with test-time scale factors at B = 3; a second call on the same workspace gives the
    same bits; every output and the workspace sit between sentinel-filled guards."""
    L = _hip.lib()
    dev = _dev()
    for B in (1, 3):
        g = torch.Generator().manual_seed(DISTS.index(name) * 100003 + R * 7 + k + B)
        scores = _scores(name, B, R, k, g)
        bits64 = _sortable_bits(scores)
        bits = torch.from_numpy(bits64.numpy().astype(np.uint32).view(np.int32)).to(dev)
        d = _planar_inputs(B, R, g)
        scale = torch.tensor([1.0, 0.75, 1.3][:B], device=dev) if B == 3 else None
        sp = None if scale is None else scale.data_ptr()
        # the single-workgroup kernel: the reference of the bits
        ab0 = torch.empty(B, k, 14, device=dev)
        rows0 = torch.empty(B, k, device=dev, dtype=torch.int32)
        nb0 = L.m3d_topk_decode_workspace_bytes(B, R)
        ws0 = torch.empty(nb0, device=dev, dtype=torch.uint8)
        _hip.check(L.m3d_topk_decode_planar(bits.data_ptr(), *[t.data_ptr() for t in d], sp, ab0.data_ptr(), rows0.data_ptr(),
                                            ws0.data_ptr(), nb0, B, 1, R, k, _stream()))
        torch.cuda.synchronize()
        key = bits64.numpy().astype(np.int64)
        for b in range(B):
            order = np.lexsort((np.arange(R), -key[b]))[:k]
            assert np.array_equal(rows0[b].cpu().numpy().astype(np.int64), order), (name, B, b)
        nb = L.m3d_topk_decode_mw_workspace_bytes(B, R, k)
        assert nb > nb0
        for wgs in WGS:
            ab, rows, ws = Guarded(B * k * 14), Guarded(B * k, torch.int32), Guarded((nb + 3) // 4, torch.int32)
            _hip.check(L.m3d_topk_decode_planar_mw(bits.data_ptr(), *[t.data_ptr() for t in d], sp, ab.ptr, rows.ptr, ws.ptr, nb,
                                                   B, 1, R, k, wgs, _stream()))
            torch.cuda.synchronize()
            for t in (ab, rows, ws):
                t.check()
            assert torch.equal(rows.t.view(B, k), rows0), (name, B, wgs)
            assert torch.equal(ab.t.view(B, k, 14), ab0), (name, B, wgs)
            # second call on the same workspace (what it left behind must not matter), without rows_out
            ab2 = Guarded(B * k * 14)
            _hip.check(L.m3d_topk_decode_planar_mw(bits.data_ptr(), *[t.data_ptr() for t in d], sp, ab2.ptr, None, ws.ptr, nb,
                                                   B, 1, R, k, wgs, _stream()))
            torch.cuda.synchronize()
            ab2.check()
            ws.check()
            assert torch.equal(ab2.t.view(B, k, 14), ab0), (name, B, wgs)


def test_topk_mw_with_36_anchor_planes_and_argument_checks():
    """A = 36 planes (row = a * HW + p, the layout the heads write) at R = 46 080, and the stated error codes."""
    L = _hip.lib()
    dev = _dev()
    B, A, HW, k = 2, 36, 1280, 3000
    R = A * HW
    g = torch.Generator().manual_seed(11)
    scores = torch.rand(B, R, generator=g) ** 6
    bits = torch.from_numpy(_sortable_bits(scores).numpy().astype(np.uint32).view(np.int32)).to(dev)
    d = _planar_inputs(B, R, g)
    d[0] = d[0].view(B, 4, A, HW).contiguous().view(B, 4 * A, HW)      # [B][4A][HW]: class-major planes
    nb0, nb = L.m3d_topk_decode_workspace_bytes(B, R), L.m3d_topk_decode_mw_workspace_bytes(B, R, k)
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    ab0, ab1 = torch.empty(B, k, 14, device=dev), torch.empty(B, k, 14, device=dev)
    r0, r1 = (torch.empty(B, k, device=dev, dtype=torch.int32) for _ in range(2))
    ptrs = [bits.data_ptr(), *[t.data_ptr() for t in d], None]
    _hip.check(L.m3d_topk_decode_planar(*ptrs, ab0.data_ptr(), r0.data_ptr(), ws.data_ptr(), nb0, B, A, HW, k, _stream()))
    for wgs in (0, 3, 256):
        ab1.fill_(float("nan"))
        _hip.check(L.m3d_topk_decode_planar_mw(*ptrs, ab1.data_ptr(), r1.data_ptr(), ws.data_ptr(), nb, B, A, HW, k, wgs,
                                               _stream()))
        torch.cuda.synchronize()
        assert torch.equal(r0, r1) and torch.equal(ab0, ab1)
    args = [*ptrs, ab1.data_ptr(), None, ws.data_ptr()]
    st = _stream()
    assert L.m3d_topk_decode_planar_mw(*args, nb, B, A, HW, 16385, 0, st) == -1        # k > 16384
    assert L.m3d_topk_decode_planar_mw(*args, nb, B, 1, 100, 101, 0, st) == -1         # k > R
    assert L.m3d_topk_decode_planar_mw(*args, nb, B, A, HW, 0, 0, st) == -1            # k < 1
    assert L.m3d_topk_decode_planar_mw(*args, nb, B, A, HW, k, -1, st) == -1           # wgs_per_image < 0
    assert L.m3d_topk_decode_planar_mw(*args, nb, B, A, HW, k, 257, st) == -1          # above the cap of 256
    assert b"wgs_per_image" in L.m3d_last_error()
    assert L.m3d_topk_decode_planar_mw(*args, nb - 8, B, A, HW, k, 0, st) == -3        # workspace too small
    assert b"workspace" in L.m3d_last_error()
    assert L.m3d_topk_decode_planar_mw(None, *args[1:], nb, B, A, HW, k, 0, st) == -1  # null pointer
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ FrameDetector
def _clone(r):
    return tuple(t.clone() for t in r)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_frame_detector_equals_detect_batch_on_every_frame(dtype, B):
    """Four different frames: detect(x) == detect_batch(net, x, conf) of the SAME x, counts and rows; the same frame twice and
    topk_wgs = 1 / 7 / default give the same bits; 20 replays of one frame are bitwise equal."""
    from lib.rpn_util import detect_batch
    from m3dssd_amd.pipeline import FrameDetector
    dev = _dev()
    net, conf = _net_dt((128, 320), B, dtype)
    xs = [synth.synth_frames(B, (128, 320), 40 + i).to(dev) for i in range(4)]
    ref = [_clone(detect_batch(net, x, conf)) for x in xs]
    assert all(int(c.sum()) > 0 for _, c in ref)
    assert any(not torch.equal(ref[0][0], r[0]) for r in ref[1:])          # the frames do differ
    dets = {w: FrameDetector(net, conf, 128, 320, batch=B, topk_wgs=w) for w in (None, 1, 7)}
    assert dets[1].topk_wgs == 1 and dets[7].topk_wgs == 7
    for w, det in dets.items():
        for x, (rd, rc) in zip(xs, ref):
            gd, gc = det.detect(x)
            assert gd.shape == rd.shape and torch.equal(gc, rc) and torch.equal(gd, rd), (w, dtype, B)
        a = _clone(det.detect(xs[1]))
        b = _clone(det.detect(xs[1]))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], ref[1][0])
        blk, cnt = det.detect(xs[2], as_block=True)
        assert blk.shape[1] == conf.nms_topN_post + 1 and torch.equal(blk[:, :-1], ref[2][0])
        assert torch.equal(blk[:, -1, 0].to(torch.int32), cnt)
    det = dets[None]
    first = _clone(det.detect(xs[3]))
    for _ in range(20):
        again = det.detect(xs[3])
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    # the eager route still runs next to the graph on the same plan
    d, c = detect_batch(net, xs[0], conf)
    assert torch.equal(d, ref[0][0]) and torch.equal(c, ref[0][1])
    # refusals
    with pytest.raises(RuntimeError, match=r"\(%d, 3, 128, 320\)" % B):
        det.detect(xs[0][:, :, :64])
    with pytest.raises(RuntimeError, match="float32"):
        det.detect(xs[0].to(torch.float64))


def test_frame_detector_full_size_single_frame():
    from lib.rpn_util import detect_batch
    from m3dssd_amd.pipeline import FrameDetector
    dev = _dev()
    crop = (384, 1280)
    net, conf = _net_dt(crop, 1, "f32")
    det = FrameDetector(net, conf, crop[0], crop[1])
    assert det.batch == 1
    for seed in (5, 6):
        x = synth.synth_frames(1, crop, seed).to(dev)
        rd, rc = _clone(detect_batch(net, x, conf))
        gd, gc = det.detect(x)
        assert torch.equal(gc, rc) and torch.equal(gd, rd)


def test_frame_detector_refine_equals_detect_batch_and_refine_detections():
    """refine=True with p2 / scale / clip_wh changing per frame == detect_batch(..., scale=) + refine_detections of the same frame."""
    from m3dssd_amd.host import refine as HR
    from m3dssd_amd.host.detect import detect_batch
    from m3dssd_amd.pipeline import FrameDetector
    dev = _dev()
    B = 2
    net, conf = _net_dt((128, 320), B, "f32")
    xs = [synth.synth_frames(B, (128, 320), 20 + i).to(dev) for i in range(3)]
    p2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884],
                   [0.0, 0.0, 0.0, 1.0]])
    metas = [{"p2": np.stack([p2, p2 * np.array([[1.0 + 0.01 * i], [1.0], [1.0], [1.0]])]),
              "scale": np.array([1.0, 0.9 - 0.1 * i], np.float32), "clip_wh": np.array([[0, 0], [300, 100 + i]], np.float32)}
             for i in range(3)]
    det = FrameDetector(net, conf, 128, 320, batch=B, refine=True)
    with pytest.raises(RuntimeError, match="meta"):
        det.detect(xs[0])
    for x, m in zip(xs, metas):
        gd, gc, gr = _clone(det.detect(x, meta=m))
        sd, sc = _clone(detect_batch(net, x, conf, scale=m["scale"]))
        assert torch.equal(gc, sc) and torch.equal(gd, sd)
        want = HR.refine_detections(sd, sc, m["p2"], hill_climbing=bool(getattr(conf, "hill_climbing", True)), scale=None,
                                    clip_wh=m["clip_wh"])
        assert gr.shape == want.shape and torch.equal(gr, want)
        assert float(gr[:, :, 0].sum()) > 0                # some rows were refined


def test_frame_detector_uint8_frames_device_and_pinned():
    from lib.rpn_util import detect_batch
    from m3dssd_amd.pipeline import FrameDetector
    dev = _dev()
    B, fh, fw = 2, 120, 310                                 # frames smaller than the crop: the stem pads them (Preprocess)
    net, conf = _net_dt((128, 320), B, "f32")
    rng = np.random.RandomState(3)
    sets = [torch.from_numpy(rng.randint(0, 256, size=(B, fh, fw, 3)).astype(np.uint8)).pin_memory() for _ in range(3)]
    det = FrameDetector(net, conf, 128, 320, batch=B, u8_frame=(fh, fw))
    for i, fr in enumerate(sets):
        rd, rc = _clone(detect_batch(net, fr.to(dev), conf))
        gd, gc = det.detect(fr if i % 2 == 0 else fr.to(dev))          # pinned host, device, pinned host
        assert torch.equal(gc, rc) and torch.equal(gd, rd)
        assert int(rc.sum()) > 0
    with pytest.raises(RuntimeError, match="uint8"):
        det.detect(sets[0].to(torch.float32))
    with pytest.raises(RuntimeError, match="pinned"):
        det.detect(sets[0].clone())                        # pageable host memory
    with pytest.raises(RuntimeError, match="does not fit"):
        FrameDetector(net, conf, 128, 320, batch=B, u8_frame=(129, 320))


def test_frame_detector_dla102_single_frame():
    from lib.rpn_util import detect_batch
    from m3dssd_amd.pipeline import FrameDetector
    from model.M3d_inference_align import build
    dev = _dev()
    crop = (128, 320)
    flags = synth.config_flags("anab_fullalign")
    conf = synth.synth_conf(crop, 0, batch_size=1, device="cuda:0", back_bone="dla102", **flags)
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0, back_bone="dla102", **flags), strict=True)
    net = net.to(dev)
    det = FrameDetector(net, conf, crop[0], crop[1])
    for seed in (40, 41):
        x = synth.synth_frames(1, crop, seed).to(dev)
        rd, rc = _clone(detect_batch(net, x, conf))
        gd, gc = det.detect(x)
        assert torch.equal(gc, rc) and torch.equal(gd, rd)
