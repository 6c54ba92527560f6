"""KITTI AP evaluator.

CPU: the oracle restatement (oracle/kitti_eval.py) against the vectors the REFERENCE's own lib/eval produced
(tests/golden/kitti_eval.npz, tools/gen_golden_eval.py), and the host natives of libm3dssd_hip.so (2-D overlaps, 3-D height
intersection, greedy matching) against the oracle -- none of them touches the device.
GPU: the rotated-IoU HIP kernel and the whole product evaluator / test_kitti_3d against the golden.
"""
import ctypes
import functools
import os
import tempfile

import numpy as np
import pytest

from oracle import kitti_eval as OK

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_eval.npz")


def _annos(tmp_path, reader):
    g = np.load(GOLDEN)
    for nm, texts in (("gt", g["gt_texts"]), ("dt", g["dt_texts"])):
        os.makedirs(os.path.join(str(tmp_path), nm), exist_ok=True)
        for i, t in enumerate(texts):
            with open(os.path.join(str(tmp_path), nm, "%06d.txt" % i), "w") as f:
                f.write(str(t))
    return g, reader(os.path.join(str(tmp_path), "gt")), reader(os.path.join(str(tmp_path), "dt"))


# ------------------------------------------------------------------------------------ oracle vs the reference's numbers
def test_oracle_rotated_iou_and_3d_overlap_match_reference():
    g = np.load(GOLDEN)
    for c in (-1, 0, 1, 2):
        assert np.abs(OK.rotate_iou_eval(g["rb"], g["qb"], c) - g["riou_%d" % (c + 1)]).max() < 5e-6, c
    assert np.abs(OK.d3_box_overlap(g["b7"], g["q7"]) - g["d3"]).max() < 5e-6
    # identical boxes: IoU 1 (the corner / edge coincidences that overflow the reference's scratch are handled)
    b = np.array([[1.0, 2.0, 4.0, 2.0, 0.7]])
    assert abs(OK.rotate_iou_eval(b, b, -1)[0, 0] - 1.0) < 1e-5
    assert OK.rotate_iou_eval(b, b + np.array([100.0, 0, 0, 0, 0]), -1)[0, 0] == 0.0
    assert OK.rotate_iou_eval(np.zeros((0, 5)), b).shape == (0, 1)
    # ... but NOT for every box: the reference's float32 edge / corner tests are data dependent, and
    # devRotateIoUEval(b, b) of lib/eval/rotate_iou.py returns 0.0 for these two rotated boxes against THEMSELVES (run in the build
    # container through tools/gen_golden_eval.py's loader, round 6).  The restatement reproduces that; a tool that scores a
    # detector against its own output must not feed bit-identical boxes (tools/bf16_ap_agreement.py shifts them by 1 mm).
    deg = np.array([[10.0, 20.0, 3.9, 1.6, 0.3], [5.0, 30.0, 3.5, 1.5, -1.2]])
    assert OK.rotate_iou_eval(deg, deg, -1)[0, 0] == 0.0 and OK.rotate_iou_eval(deg, deg, -1)[1, 1] == 0.0
    shifted = deg + np.array([1e-3, 5e-4, 0, 0, 0])
    assert np.diag(OK.rotate_iou_eval(deg, shifted, -1)).min() > 0.998


def test_oracle_official_result_matches_reference(tmp_path):
    g, gt, dt = _annos(tmp_path, OK.get_label_annos)
    assert len(gt) == len(dt) == len(g["gt_texts"])
    assert gt[5]["name"].shape[0] == 0 and dt[7]["bbox"].shape == (0, 4)          # the empty label / result files
    assert dt[0]["score"].shape[0] == dt[0]["bbox"].shape[0] and gt[0]["score"].sum() == 0
    ret = OK.eval_class(gt, dt, [0, 1, 2], [0, 1, 2], 1, np.array([[0.7, 0.5, 0.5]] * 3)[np.newaxis], compute_aos=False)
    assert np.allclose(ret["precision"], g["bev_precision"], rtol=0, atol=1e-12, equal_nan=True)
    assert np.allclose(ret["recall"], g["bev_recall"], rtol=0, atol=1e-12, equal_nan=True)
    text, stats = OK.get_official_eval_result(gt, dt, [0, 1, 2])
    assert text == str(g["result_text"])
    for k, v in zip(g["stat_keys"], g["stat_vals"]):
        assert abs(stats[str(k)] - v) < 1e-9, k


def test_oracle_get_thresholds_and_filters():
    # 10 true-positive scores, 10 valid ground truths, 41 sample points -> every score is a threshold
    s = np.linspace(0.95, 0.05, 10)
    assert np.allclose(OK.get_thresholds(s.copy(), 10), s)
    assert len(OK.get_thresholds(np.linspace(1, 0, 500), 500)) == 41
    gt = dict(name=np.array(["Car", "Van", "Pedestrian", "DontCare", "Car"]), occluded=np.array([0, 0, 0, -1, 2]),
              truncated=np.array([0.0, 0.0, 0.0, -1.0, 0.0]), bbox=np.array([[0, 0, 50, 50], [0, 0, 50, 60], [0, 0, 20, 50],
                                                                             [5, 5, 60, 60], [0, 0, 30, 30.0]]))
    dt = dict(name=np.array(["Car", "Cyclist", "Car"]), bbox=np.array([[0, 0, 40, 45.0], [0, 0, 10, 60], [0, 0, 10, 20]]))
    n, ig, idt, dc = OK.clean_data(gt, dt, 0, 0)
    assert n == 1 and ig == [0, 1, -1, -1, 1] and idt == [0, -1, 1] and len(dc) == 1


# ------------------------------------------------------------------------------------ host natives vs the oracle (no GPU)
def _lib():
    from m3dssd_amd import _hip
    return _hip, _hip.lib()


def _dp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_native_overlaps_match_oracle():
    _hip, L = _lib()
    rng = np.random.default_rng(3)
    b = np.sort(rng.uniform(0, 100, (13, 2, 2)), axis=1).reshape(13, 4)[:, [0, 1, 2, 3]]
    b = np.stack([b[:, 0], b[:, 1], b[:, 2], b[:, 3]], 1)
    q = b[::-1][:7] + rng.normal(0, 3, (7, 4))
    for c in (-1, 0, 1, 2):
        out = np.zeros((13, 7))
        _hip.check(L.m3d_eval_image_box_overlap(_dp(np.ascontiguousarray(b)), 13, _dp(np.ascontiguousarray(q)), 7, c, _dp(out)))
        assert np.array_equal(out, OK.image_box_overlap(b, q, c)), c
    g = np.load(GOLDEN)
    b7, q7 = np.ascontiguousarray(g["b7"]), np.ascontiguousarray(g["q7"])
    rinc = OK.rotate_iou_eval(b7[:, [0, 2, 3, 5, 6]], q7[:, [0, 2, 3, 5, 6]], 2).astype(np.float64)
    r = np.ascontiguousarray(rinc)
    _hip.check(L.m3d_eval_d3_overlap(_dp(b7), b7.shape[0], _dp(q7), q7.shape[0], _dp(r), -1))
    assert np.abs(r - g["d3"]).max() < 5e-6


def test_native_statistics_match_oracle(tmp_path):
    _hip, L = _lib()
    g, gt, dt = _annos(tmp_path, OK.get_label_annos)
    overlaps, parted, total_dt, total_gt = OK.calculate_iou_partly(dt, gt, 0, 50)
    for cls, diff in ((0, 0), (0, 2), (1, 1), (2, 2)):
        gds, dds, igs, ids_, dcs, dcn, nvalid = OK._prepare_data(gt, dt, cls, diff)
        for i in range(len(gt)):
            for compute_fp, thresh, aos in ((False, 0.0, False), (True, 0.3, True), (True, 0.6, False)):
                want = OK.compute_statistics(overlaps[i], gds[i], dds[i], igs[i], ids_[i], dcs[i], 0, 0.5, thresh, compute_fp, aos)
                ov = np.ascontiguousarray(overlaps[i], dtype=np.float64)
                st, thr, nthr = np.zeros(4), np.zeros(max(1, gds[i].shape[0])), ctypes.c_int(0)
                gd, dd = np.ascontiguousarray(gds[i], dtype=np.float64), np.ascontiguousarray(dds[i], dtype=np.float64)
                _hip.check(L.m3d_eval_statistics(_dp(ov), ov.shape[1] if ov.ndim == 2 and ov.size else 1, _dp(gd), gd.shape[0],
                                                 _dp(dd), dd.shape[0], _dp(igs[i]), _dp(ids_[i]), _dp(dcs[i]), dcs[i].shape[0], 0, 0.5,
                                                 thresh, int(compute_fp), int(aos), _dp(st), _dp(thr), ctypes.byref(nthr)))
                assert (st[0], st[1], st[2]) == (want[0], want[1], want[2]), (cls, diff, i)
                assert abs(st[3] - want[3]) < 1e-12
                assert np.array_equal(thr[:nthr.value], want[4])


# ------------------------------------------------------------------------------------ partitions (no GPU at metric 0)
# A real evaluation always takes the multi-part path (3769 validation images: 50 parts of 75 and one of 19); the 40 golden images
# with the default num_parts = 50 form ONE part.  The parts only batch the overlap computation, so no value may depend on them.
MIN_OVERLAPS = np.array([[0.7, 0.5, 0.5]] * 3)[np.newaxis]
NUM_PARTS = (1, 2, 3, 7, 13, 40)         # parts of 40 | 20, 20 | 13, 13, 13, 1 | 5 x 7, 5 | 3 x 13, 1 | 1 x 40


@functools.lru_cache(maxsize=None)
def _golden_annos():
    """(gt, dt) of the golden fixture, read by the oracle's reader (the product's reader is compared with it further down)."""
    with tempfile.TemporaryDirectory() as d:
        _, gt, dt = _annos(d, OK.get_label_annos)
    return gt, dt


@functools.lru_cache(maxsize=None)
def _oracle_eval_class(metric, num_parts):
    gt, dt = _golden_annos()
    return OK.eval_class(gt, dt, [0, 1, 2], [0, 1, 2], metric, MIN_OVERLAPS, compute_aos=(metric == 0), num_parts=num_parts)


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("recall", "precision", "orientation"))


def test_get_split_parts_of_the_partition_cases():
    from m3dssd_amd.eval.eval import get_split_parts
    assert get_split_parts(40, 50) == [40] and get_split_parts(3769, 50) == [75] * 50 + [19]
    want = {1: [40], 2: [20, 20], 3: [13, 13, 13, 1], 7: [5] * 7 + [5], 13: [3] * 13 + [1], 40: [1] * 40}
    for n in NUM_PARTS:
        assert get_split_parts(40, n) == want[n] == OK.get_split_parts(40, n) and sum(want[n]) == 40


@pytest.mark.parametrize("num_parts", NUM_PARTS)
def test_eval_class_bbox_aos_does_not_depend_on_the_partition(num_parts):
    """Product eval_class at metric 0 (2-D boxes + AOS: host natives only) over several parts == the oracle over one part: the
    running gt / dt / dontcare offsets of m3d_eval_fused_statistics and the slicing of the parted overlaps."""
    from m3dssd_amd.eval.eval import eval_class
    gt, dt = _golden_annos()
    want = _oracle_eval_class(0, 50)
    assert np.nanmax(want["precision"]) > 0.5 and np.nanmax(want["orientation"]) > 0.3          # not a comparison of zeros
    got = eval_class(gt, dt, [0, 1, 2], [0, 1, 2], 0, MIN_OVERLAPS, compute_aos=True, num_parts=num_parts)
    for k in ("recall", "precision", "orientation"):
        assert np.array_equal(got[k], want[k], equal_nan=True), (k, num_parts)


def test_eval_class_of_empty_images_in_two_parts():
    """Four images made of the fixture's empty label file and its empty result file, two parts of two."""
    from m3dssd_amd.eval.eval import eval_class
    gt, dt = _golden_annos()
    assert len(gt[5]["name"]) == 0 and len(dt[7]["name"]) == 0
    e_gt, e_dt = [gt[5]] * 4, [dt[7]] * 4
    want = OK.eval_class(e_gt, e_dt, [0, 1, 2], [0, 1, 2], 0, MIN_OVERLAPS, compute_aos=True, num_parts=2)
    got = eval_class(e_gt, e_dt, [0, 1, 2], [0, 1, 2], 0, MIN_OVERLAPS, compute_aos=True, num_parts=2)
    assert _same(got, want) and got["precision"].shape == (3, 3, 1, 41)


@pytest.mark.parametrize("cls,diff,min_overlap", [(0, 1, 0.7), (0, 2, 0.5), (1, 0, 0.5), (2, 2, 0.5)])
def test_native_fused_statistics_over_hand_built_parts(cls, diff, min_overlap):
    """m3d_eval_fused_statistics called directly on two parts built by hand from golden images: one [sum dt][sum gt] overlap matrix
    per part (ov_stride = sum gt), unequal gt / dt counts per image, an image without detections and one without labels.
    Expected: the sum of the oracle's per-image compute_statistics over the same images; pr compared exactly."""
    _hip, L = _lib()
    gt, dt = _golden_annos()
    parts = ([8, 7, 6, 5], [3, 19, 13])
    assert len(dt[7]["name"]) == 0 and len(gt[5]["name"]) == 0
    assert all(len(gt[i]["name"]) != len(dt[i]["name"]) for i in (8, 7, 5, 3, 19, 13))
    thresholds = np.array([0.0, 0.2, 0.45, 0.7, 0.9])
    pr, want = np.zeros((len(thresholds), 4)), np.zeros((len(thresholds), 4))
    for idxs in parts:
        g, d = [gt[i] for i in idxs], [dt[i] for i in idxs]
        gds, dds, igs, ids_, dcs, dcn, _ = OK._prepare_data(g, d, cls, diff)
        ov = np.ascontiguousarray(OK.image_box_overlap(np.concatenate([a["bbox"] for a in d]), np.concatenate([a["bbox"] for a in g])))
        gn, dn = np.array([x.shape[0] for x in gds], dtype=np.int64), np.array([x.shape[0] for x in dds], dtype=np.int64)
        assert ov.shape == (dn.sum(), gn.sum())
        gi = di = 0
        for i in range(len(idxs)):
            for t, thresh in enumerate(thresholds):
                tp, fp, fn, sim, _ = OK.compute_statistics(ov[di:di + dn[i], gi:gi + gn[i]], gds[i], dds[i], igs[i], ids_[i], dcs[i], 0,
                                                           min_overlap, thresh, True, True)
                want[t, :3] += (tp, fp, fn)
                if sim != -1:
                    want[t, 3] += sim
            gi, di = gi + gn[i], di + dn[i]
        cat = [np.ascontiguousarray(np.concatenate(x, 0), dtype=np.float64) for x in (gds, dds, dcs)]
        ig, idt = (np.ascontiguousarray(np.concatenate(x, 0), dtype=np.int64) for x in (igs, ids_))
        dcn = np.ascontiguousarray(dcn, dtype=np.int64)
        _hip.check(L.m3d_eval_fused_statistics(_dp(ov), int(gn.sum()), _dp(pr), _dp(gn), _dp(dn), _dp(dcn), len(idxs), _dp(cat[0]),
                                               _dp(cat[1]), _dp(cat[2]), _dp(ig), _dp(idt), 0, min_overlap, _dp(thresholds),
                                               len(thresholds), 1))
    assert want[:, :3].sum() > 0
    assert np.array_equal(pr, want), (pr, want)


# ------------------------------------------------------------------------------------ rotated IoU: seeded boxes and an exact lattice
ROT_SHAPES = [(1, 1), (1, 53), (37, 1), (37, 53), (128, 3)]      # N*K below, at and across the 128-thread block; 2436 pairs


@functools.lru_cache(maxsize=None)
def _rot_case(N, K):
    """Seeded boxes; about half of the query boxes are perturbed copies of boxes, so that overlaps of every size occur.
    -> (boxes [N, 5] float64, qboxes [K, 5] float64, {criterion: oracle matrix}).

    The ranges follow from the tolerance, not the other way round.  The oracle's cosf / sinf are numpy's and the kernel's are the
    device library's: where they differ in the last place, a float32 corner coordinate may land on the neighbouring float32, and
    the intersection area moves by up to (coordinate ulp) x (edge length) per corner.  With centres within +-2.5 and sizes of
    1.0 .. 2.4 by 0.8 .. 1.6 every corner coordinate is below 4 (ulp 2.4e-7), so four moved corners change an area by at most
    4 x 2.4e-7 x 2.4 = 2.3e-6 (criterion 2) and a ratio by at most that over the smallest area 0.8 = 2.9e-6 -- inside the project's
    5e-6.  (Boxes of 0.5 x 0.5 at a coordinate of 12, ulp 9.5e-7, would allow 4 x 9.5e-7 x 0.5 / 0.25 = 7.6e-6: a tolerance of
    5e-6 cannot be asked of such a pair.)"""
    rng = np.random.default_rng(1000 * N + K)
    lo, hi = np.array([-2.5, -2.5, 1.0, 0.8, -3.2]), np.array([2.5, 2.5, 2.4, 1.6, 3.2])
    b = rng.uniform(lo, hi, (N, 5))
    q = rng.uniform(lo, hi, (K, 5))
    for k in range(0, K, 2):
        q[k] = b[rng.integers(0, N)] + rng.normal(0, 1.0, 5) * [0.2, 0.2, 0.15, 0.15, 0.2]
    q[:, :4] = np.clip(q[:, :4], lo[:4], hi[:4])
    return b, q, {c: OK.rotate_iou_eval(b, q, c) for c in (-1, 0, 1, 2)}


def _eighths(b):
    """Edge coordinates (x_lo, x_hi, y_lo, y_hi) of axis-aligned lattice boxes in units of 1/8, as exact integers."""
    e = np.stack([b[:, 0] - b[:, 2] / 2, b[:, 0] + b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 1] + b[:, 3] / 2], 1) * 8
    assert np.array_equal(e, np.round(e))
    return e.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _lattice():
    """Axis-aligned boxes (angle 0) whose centres and sizes are multiples of 1/4: corners are multiples of 1/8 below 16, so every
    float32 sum, product and quotient of the rotated-intersection code is exact (products of three such values need 9 fraction bits
    and stay below 2^12; cos 0 = 1 and sin 0 = 0 exactly).
    -> (boxes [n, 5], kind [n, n]: 0 disjoint, 1 contained, 2 overlapping (0..2 in general position: no two edge coordinates
    equal along either axis), 3 coincident edge or corner, 4 identical; closed-form intersection areas [n, n] float64)."""
    rng = np.random.default_rng(77)
    hand = [[0, 0, 4, 2], [0, 0, 4, 2], [4, 0, 4, 2], [0, 2, 4, 2], [4, 2, 4, 2], [0, 0, 2, 1], [1, 0.5, 2, 1], [0.25, 0.25, 1, 0.5],
            [0, 0, 8, 6], [9, 9, 1, 1], [0.5, 0.25, 4.5, 0.5], [0.25, 0, 0.5, 5.5]]
    rand = np.concatenate([rng.integers(-24, 25, (14, 2)) / 4.0, rng.integers(1, 25, (14, 2)) / 4.0], 1)
    b = np.concatenate([np.array(hand, dtype=np.float64), rand])
    b = np.concatenate([b, np.zeros((b.shape[0], 1))], 1)
    e = _eighths(b)
    n = b.shape[0]
    kind, area = np.zeros((n, n), dtype=np.int64), np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            iw = min(e[i, 1], e[j, 1]) - max(e[i, 0], e[j, 0])
            ih = min(e[i, 3], e[j, 3]) - max(e[i, 2], e[j, 2])
            area[i, j] = (max(iw, 0) / 8.0) * (max(ih, 0) / 8.0)
            if np.array_equal(e[i], e[j]):
                kind[i, j] = 4
            elif len({e[i, 0], e[i, 1], e[j, 0], e[j, 1]}) < 4 or len({e[i, 2], e[i, 3], e[j, 2], e[j, 3]}) < 4:
                kind[i, j] = 3
            elif iw <= 0 or ih <= 0:
                kind[i, j] = 0
            else:
                inside = lambda a, c: e[a, 0] > e[c, 0] and e[a, 1] < e[c, 1] and e[a, 2] > e[c, 2] and e[a, 3] < e[c, 3]
                kind[i, j] = 1 if inside(i, j) or inside(j, i) else 2
    return b, kind, area


def _lattice_closed_form(b, area, criterion):
    """What devRotateIoUEval(query j, box i) yields when its intersection area is exact: float32 areas, float64 ratio, float32."""
    a = (b[:, 2].astype(np.float32) * b[:, 3].astype(np.float32))
    a_box, a_query = a[:, None], a[None, :]                       # iou[n, k]: box n, query k
    if criterion == -1:
        v = area / ((a_query + a_box).astype(np.float32).astype(np.float64) - area)
    elif criterion == 0:
        v = area / a_query.astype(np.float64)
    elif criterion == 1:
        v = area / a_box.astype(np.float64)
    else:
        v = area
    return np.broadcast_to(v, area.shape).astype(np.float32)


def test_lattice_holds_every_kind_of_pair_and_the_oracle_agrees_with_the_closed_form():
    b, kind, area = _lattice()
    counts = [int((kind == k).sum()) for k in range(5)]
    print("lattice pairs: disjoint %d, contained %d, overlapping %d, coincident %d, identical %d" % tuple(counts))
    assert counts[0] >= 100 and counts[1] >= 10 and counts[2] >= 50 and counts[3] >= 40 and counts[4] == b.shape[0] + 2
    e = _eighths(b)
    assert any(kind[i, j] == 3 and (e[i, 1] == e[j, 0] or e[i, 3] == e[j, 2]) and area[i, j] == 0 for i in range(len(b))
               for j in range(len(b)))                            # boxes that only share an edge
    general = kind <= 2
    for c in (-1, 0, 1, 2):
        want = _lattice_closed_form(b, area, c)
        assert np.array_equal(OK.rotate_iou_eval(b, b, c)[general], want[general]), c


# ------------------------------------------------------------------------------------ GPU: kernel + whole evaluator
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N,K", ROT_SHAPES)
def test_rotate_iou_kernel_whole_matrix_all_criteria(N, K, dtype):
    """The WHOLE [N, K] matrix of lib.eval.rotate_iou.rotate_iou_gpu_eval against the oracle for all four criteria at the project's
    5e-6, with float32 and float64 inputs (the result takes the dtype of `boxes`)."""
    from gpu_common import _log
    from lib.eval.rotate_iou import rotate_iou_gpu_eval
    b, q, want = _rot_case(N, K)
    assert want[-1].max() > 0.3 or N * K == 1
    for c in (-1, 0, 1, 2):
        got = rotate_iou_gpu_eval(b.astype(dtype), q.astype(dtype), c)
        assert got.shape == (N, K) and got.dtype == dtype
        err = float(np.abs(got.astype(np.float64) - want[c].astype(np.float64)).max())
        _log("rotate_iou_whole", {"N": N, "K": K, "dtype": np.dtype(dtype).name, "criterion": c, "max_err": err})
        print("rotate_iou %dx%d %s criterion %d: max err %.3e" % (N, K, np.dtype(dtype).name, c, err))
        assert err < 5e-6, (N, K, c, err)


@pytest.mark.gpu
def test_rotate_iou_kernel_is_exact_on_a_lattice():
    """Axis-aligned lattice boxes: pairs in general position equal the closed-form axis-aligned intersection (float64, rounded to
    float32) exactly; pairs with coincident edges or corners, and identical boxes, follow the reference's data-dependent rule and
    equal the oracle bit for bit."""
    from lib.eval.rotate_iou import rotate_iou_gpu_eval
    b, kind, area = _lattice()
    general = kind <= 2
    for c in (-1, 0, 1, 2):
        got = rotate_iou_gpu_eval(b.astype(np.float32), b.astype(np.float32), c)
        want = _lattice_closed_form(b, area, c)
        assert np.array_equal(got[general].view(np.uint32), want[general].view(np.uint32)), (c, np.argwhere(general & (got != want))[:5])
        orc = OK.rotate_iou_eval(b, b, c)
        assert np.array_equal(got[~general].view(np.uint32), orc[~general].view(np.uint32)), (c, np.argwhere(~general & (got != orc))[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [1, 2])
def test_eval_class_bev_3d_does_not_depend_on_the_partition(metric):
    """Product eval_class at metrics 1 (BEV) and 2 (3-D), whose overlaps come from the device: every partition gives the bits of
    the single part, and those agree with the oracle within the 1e-9 of test_product_evaluator_matches_reference."""
    from lib.eval.eval import eval_class
    gt, dt = _golden_annos()
    one = eval_class(gt, dt, [0, 1, 2], [0, 1, 2], metric, MIN_OVERLAPS, num_parts=50)
    for n in NUM_PARTS:
        got = eval_class(gt, dt, [0, 1, 2], [0, 1, 2], metric, MIN_OVERLAPS, num_parts=n)
        assert _same(got, one), (metric, n)
    want = _oracle_eval_class(metric, 40)                         # the oracle is per image: its parts only batch the IoU loop
    assert np.nanmax(want["precision"]) > 0.5
    for k in ("precision", "recall"):
        assert np.allclose(one[k], want[k], rtol=0, atol=1e-9, equal_nan=True), (metric, k)
    if metric == 1:
        g = np.load(GOLDEN)
        assert np.allclose(one["precision"], g["bev_precision"], rtol=0, atol=1e-9, equal_nan=True)


@pytest.mark.gpu
def test_rotate_iou_kernel_matches_reference_and_oracle():
    from lib.eval.rotate_iou import rotate_iou_gpu_eval
    g = np.load(GOLDEN)
    for c in (-1, 0, 1, 2):
        got = rotate_iou_gpu_eval(g["rb"], g["qb"], c)
        assert got.dtype == g["rb"].dtype and np.abs(got - g["riou_%d" % (c + 1)]).max() < 5e-6, c
    rng = np.random.default_rng(5)
    b = rng.uniform([-20, -20, 0.5, 0.5, -3.2], [20, 20, 6, 3, 3.2], (300, 5))
    q = np.concatenate([b[:150] + rng.normal(0, 0.3, (150, 5)), rng.uniform([-20, -20, 0.5, 0.5, -3.2], [20, 20, 6, 3, 3.2], (57, 5))])
    got = rotate_iou_gpu_eval(b, q, -1)
    sub = OK.rotate_iou_eval(b[:40], q[:60], -1)
    assert np.abs(got[:40, :60] - sub).max() < 5e-6
    assert got.min() >= 0 and got.max() <= 1.0 + 1e-5 and (got > 0.3).sum() > 50
    bb = np.array([[1.0, 2.0, 4.0, 2.0, 0.7]])
    assert abs(rotate_iou_gpu_eval(bb, bb, -1)[0, 0] - 1.0) < 1e-5
    assert rotate_iou_gpu_eval(np.zeros((0, 5)), bb).shape == (0, 1)
    # the reference's data-dependent self-IoU degeneracy (see the oracle test above) is reproduced by the kernel, bit for bit
    deg = np.array([[10.0, 20.0, 3.9, 1.6, 0.3], [5.0, 30.0, 3.5, 1.5, -1.2], [0.0, 10.0, 4.0, 2.0, 0.0]])
    assert np.array_equal(rotate_iou_gpu_eval(deg, deg, -1), OK.rotate_iou_eval(deg, deg, -1).astype(deg.dtype))


@pytest.mark.gpu
def test_product_evaluator_matches_reference(tmp_path):
    from lib.eval.eval import eval_class, get_official_eval_result
    from lib.eval.kitti_common import get_label_annos
    g, gt, dt = _annos(tmp_path, get_label_annos)
    o_gt = OK.get_label_annos(os.path.join(str(tmp_path), "gt"))
    for a, b in zip(gt, o_gt):
        for k in b:
            assert np.array_equal(a[k], b[k]), k
    ret = eval_class(gt, dt, [0, 1, 2], [0, 1, 2], 1, np.array([[0.7, 0.5, 0.5]] * 3)[np.newaxis], compute_aos=False)
    assert np.allclose(ret["precision"], g["bev_precision"], rtol=0, atol=1e-9, equal_nan=True)
    assert np.allclose(ret["recall"], g["bev_recall"], rtol=0, atol=1e-9, equal_nan=True)
    pr = {}
    text, stats = get_official_eval_result(gt, dt, [0, 1, 2], PR_detail_dict=pr)
    assert text == str(g["result_text"])
    for k, v in zip(g["stat_keys"], g["stat_vals"]):
        assert abs(stats[str(k)] - v) < 1e-9, k
    assert set(pr) == {"bbox", "aos", "bev", "3d"}
    # class names instead of ids, a single class
    t1, s1 = get_official_eval_result(gt, dt, "Car")
    assert t1 == "".join(l + "\n" for l in text.split("\n")[:10]) and s1["Car_3d_moderate_R40"] == stats["Car_3d_moderate_R40"]


@pytest.mark.gpu
def test_test_kitti_3d_writes_results_and_evaluates(tmp_path):
    """lib.rpn_util.test_kitti_3d with the reference's signature: detect (batched) -> refine on the device -> '<id>.txt'
    (identical to the per-image reference-style path) -> AP against a label folder."""
    import torch
    from lib.rpn_util import im_detect_3d, test_kitti_3d
    from m3dssd_amd import synth
    from m3dssd_amd.config import Conf
    from m3dssd_amd.host import refine as R
    from model.M3d_inference_align import build
    dev = torch.device("cuda:0")
    crop = (128, 320)
    conf = synth.synth_conf(crop, 0, batch_size=3, device="cuda:0")
    conf.datasets_validation = [Conf(name="kitti_synth")]
    conf.hill_climbing = True
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0))
    net = net.to(dev)
    p2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884],
                   [0.0, 0.0, 0.0, 1.0]])
    frames = synth.synth_frames(7, crop, 77)
    dataset = [(frames[i:i + 1], Conf(id="%06d" % i, p2=p2, scale_factor=1.0)) for i in range(7)]
    label_dir = tmp_path / "kitti_synth" / "validation" / "label_2"
    os.makedirs(label_dir)
    # labels = the detector's own output of a first pass with alpha jittered -> a non-trivial AP
    res_dir = tmp_path / "results" / "data"
    with pytest.raises(FileNotFoundError):                           # like the reference: a missing label folder is an error ...
        test_kitti_3d(dataset, net, conf, str(res_dir), str(tmp_path), use_log=False, phase="train")
    text, stats = test_kitti_3d(dataset, net, conf, str(res_dir), str(tmp_path), use_log=False, phase="train", require_labels=False)
    assert text is None                                              # ... unless the caller asks for the result files only
    files = sorted(os.listdir(res_dir))
    assert files == ["%06d.txt" % i for i in range(7)]
    from lib.rpn_util import detect_batch
    for lo, hi in ((0, 3), (3, 6), (6, 7)):                          # the batches the wrapper formed (batch_size 3, 7 frames)
        dets, counts = detect_batch(net, frames[lo:hi].to(dev), conf)
        ref = R.refine_detections(dets.clone(), counts, np.stack([p2] * (hi - lo))).cpu().numpy()
        for b in range(hi - lo):
            assert open(res_dir / ("%06d.txt" % (lo + b))).read() == R.kitti_text(ref[b], conf.lbls)
    # scale_factor != 1 (lib/rpn_util.py:1506-1507: BEFORE the sort and the NMS, inside m3d_topk_decode_scaled) and clip_boxes
    # (:1557-1561, inside m3d_refine_3d_ex; full batches: both in the captured graph) == the eager detection with the same factors
    # followed by the float32 clip and the plain refinement
    conf.clip_boxes = True
    scales = [0.8 + 0.05 * i for i in range(7)]
    dataset2 = [(frames[i:i + 1], Conf(id="%06d" % i, p2=p2, scale_factor=scales[i], imW=300, imH=110)) for i in range(7)]
    res2 = tmp_path / "results2" / "data"
    test_kitti_3d(dataset2, net, conf, str(res2), str(tmp_path), use_log=False, phase="train", require_labels=False)
    from oracle import refine as OR
    n_clipped = n_oracle_lines = 0
    for lo, hi in ((0, 3), (3, 6), (6, 7)):
        dets, counts = detect_batch(net, frames[lo:hi].to(dev), conf, scale=scales[lo:hi])
        d = dets.clone()
        # the scaled rows are the unscaled decode divided in float32 -- for the rows both detections keep
        un, _ = detect_batch(net, frames[lo:hi].to(dev), conf)
        un = un.clone()
        sc = torch.tensor(scales[lo:hi], device=dev, dtype=torch.float32)
        un[:, :, 0:4] /= sc[:, None, None]
        un[:, :, 6:8] /= sc[:, None, None]
        same = (un[:, :, 13] == d[:, :, 13]) & (un[:, :, 4] == d[:, :, 4])
        assert same.float().mean() > 0.5 and torch.equal(un[same], d[same])
        n_clipped += int((d[:, :, 2] > 299).sum()) + int((d[:, :, 3] > 109).sum())
        d[:, :, 0].clamp_(0, 299); d[:, :, 2].clamp_(0, 299); d[:, :, 1].clamp_(0, 109); d[:, :, 3].clamp_(0, 109)
        ref = R.refine_detections(d, counts, np.stack([p2] * (hi - lo))).cpu().numpy()
        for b in range(hi - lo):
            assert open(res2 / ("%06d.txt" % (lo + b))).read() == R.kitti_text(ref[b], conf.lbls), (lo, b)
        # ... and an expectation that does not come from the product's own refinement: the oracle's text of the same scaled and
        # clipped rows (the clamps above are the float32 np.clip of lib/rpn_util.py:1557-1561)
        rows, cnt = d.cpu().numpy(), counts.cpu().numpy()
        for b in range(hi - lo):
            want = OR.kitti_text(rows[b, :int(cnt[b])], p2, conf.lbls, nms_topn_post=conf.nms_topN_post)
            assert open(res2 / ("%06d.txt" % (lo + b))).read() == want, (lo, b)
            n_oracle_lines += len(want.splitlines())
    assert n_oracle_lines > 0
    assert n_clipped > 0                                             # the clip really acted on some box
    conf.clip_boxes = False
    ab = im_detect_3d(frames[6], net, conf)                          # and the reference-style single-image entry (same batch of 1)
    assert np.array_equal(ab[:conf.nms_topN_post], detect_batch(net, frames[6:7].to(dev), conf)[0][0, :len(ab)].cpu().numpy())
    n_lines = 0
    for f in files:
        lines = open(res_dir / f).read().splitlines()
        n_lines += len(lines)
        with open(label_dir / f, "w") as out:
            for ln in lines[::2]:                                    # every second detection becomes a ground-truth object
                p = ln.split(" ")
                out.write(" ".join([p[0], "0.00", "0"] + p[3:15]) + "\n")
    assert n_lines > 0
    text, stats = test_kitti_3d(dataset, net, conf, str(res_dir), str(tmp_path), use_log=False, phase="validation")
    assert "Car AP@0.70, 0.70, 0.70:" in text and "Cyclist AP_R40@0.50, 0.50, 0.50:" in text
    assert all(np.isfinite(v) or np.isnan(v) for v in stats.values()) and len(stats) >= 36
    assert max(stats["%s_3d_easy_R40" % c] for c in conf.lbls if np.isfinite(stats["%s_3d_easy_R40" % c])) > 10.0
