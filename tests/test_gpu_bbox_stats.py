"""GPU tests (-m gpu) of the dataset statistics on the device: m3d_rpn_target_stats (launches 1-3 of csrc/rpn_loss.hip on float64
rois with the reducing form of launch 3, plus its finish launch) behind ops.rpn_target_stats and
m3dssd_amd.host.dataset_stats.compute_bbox_stats.

Yardstick: the reference's own per-image sums, means and stds (tests/golden/bbox_stats.npz; tests/test_bbox_stats_host.py pins
the numpy restatement to them bit for bit and shows that float32 rois miss the first bound below by > 1e3).

Bounds, per image with n fg rows, per column, against the golden's longdouble sums:
  columns without a logarithm (dx dy x3d y3d z ry): n * 2^-53 * sum |t|.  Every operation up to the float32 transform is exact
      IEEE float64 on both sides, so the summands are the same numbers; only the order of n float64 additions differs.
  columns with a logarithm (dw dh w3d h3d l3d): n * 2^-23 * max |t|.  The device's float64 log may differ from numpy's by a
      float64 ulp, which can move the float32 rounding of t by one float32 ulp of t (the argument of rpn_loss_ref.target_tolerance).
End to end: means within 2^-23 * max |t| per column, stds within 2^-22 * max |t| (max over the images).  (The reference itself
adds each image's float32 transforms in float32 before it widens; the device never does.)"""
import os

import numpy as np
import pytest
import torch

from m3dssd_amd import _hip
from m3dssd_amd.host import dataset_stats as ds
from m3dssd_amd.host import loss as hl
from m3dssd_amd.host import ops
from gpu_common import _dev, _stream
import bbox_stats_ref as BR
import poison

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PLAIN_COLS, LOG_COLS = (0, 1, 4, 5, 6, 10), (2, 3, 7, 8, 9)
NC = hl.TARGET_STATS_COLS


@pytest.fixture(scope="module")
def G():
    return dict(np.load(os.path.join(GOLDEN, "bbox_stats.npz")))


@pytest.fixture(scope="module")
def case(G):
    conf, imdb = BR.conf_from_arrays(G), BR.imdb_from_arrays(G)
    conf.anchors = np.array(G["anchors"])
    conf.device = "cuda:0"
    return conf, imdb


@pytest.fixture(scope="module")
def rows(case):
    """Pass 1 of every image through the host layer, computed once: float64 [8, 23]."""
    _dev()
    conf, imdb = case
    return ds.image_target_stats(conf, imdb)


def test_n_fg_and_the_sums_of_every_image_against_the_reference(G, rows):
    fig = {"plain": 0.0, "log": 0.0}
    for i in range(len(rows)):
        n = int(G["n_fg"][i])
        assert rows[i, 0] == n, (i, rows[i, 0], n)
        if n == 0:
            assert not rows[i].any() and rows[i].tobytes() == np.zeros(NC).tobytes()          # no gts (4), all ignored (6): +0.0
            continue
        err = np.abs(rows[i, 1:12] - G["sum_t"][i])
        for c in PLAIN_COLS:
            bound = n * 2.0 ** -53 * G["sum_abs_t"][i, c]
            fig["plain"] = max(fig["plain"], err[c] / bound)
        for c in LOG_COLS:
            bound = n * 2.0 ** -23 * G["max_abs_t"][i, c]
            fig["log"] = max(fig["log"], err[c] / bound)
    print("device sums vs reference, worst error / bound: %s" % fig)
    assert fig["plain"] <= 1.0 and fig["log"] <= 1.0, fig
    assert int(G["n_fg"].sum()) > 40 and (G["n_fg"] == 0).sum() == 2


def test_compute_bbox_stats_end_to_end_against_the_reference(G, case):
    conf, imdb = case
    conf = conf.copy()
    ds.compute_bbox_stats(conf, imdb, None)
    assert conf.bbox_means.shape == conf.bbox_stds.shape == (1, 11) and conf.bbox_means.dtype == conf.bbox_stds.dtype == np.float64
    mx = G["max_abs_t"].max(axis=0)
    em, es = np.abs(conf.bbox_means - G["bbox_means"])[0], np.abs(conf.bbox_stds - G["bbox_stds"])[0]
    print("means: worst error / bound %.3g; stds: %.3g" % ((em / (2.0 ** -23 * mx)).max(), (es / (2.0 ** -22 * mx)).max()))
    assert (em <= 2.0 ** -23 * mx).all(), em / (2.0 ** -23 * mx)
    assert (es <= 2.0 ** -22 * mx).all(), es / (2.0 ** -22 * mx)


def test_second_pass_squares_around_the_means(G, case, rows):
    """sum (t - c) and sum (t - c)^2 with c = the reference's means, against the restatement's float32 transforms in longdouble.
    Bound: a log column's t may sit one float32 ulp off (delta), which moves (t - c)^2 by 2 |t - c| delta + delta^2; on top,
    the float64 roundings of the difference, the square and the n additions."""
    conf, imdb = case
    c = G["bbox_means"][0]
    got = ds.image_target_stats(conf, imdb, c)
    cols = [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11]
    for i, im in enumerate(imdb):
        assert got[i, 0] == rows[i, 0]
        p = BR.image_transforms(conf, im)
        n = int(G["n_fg"][i])
        if n == 0:
            assert not got[i].any()
            continue
        t = p[0][p[0][:, 4] > 0][:, cols].astype(np.longdouble)
        d = t - c.astype(np.longdouble)
        want = (d * d).sum(axis=0)
        delta = 2.0 ** -23 * G["max_abs_t"][i]                  # one float32 ulp of t, log columns only
        delta[list(PLAIN_COLS)] = 0.0
        exact = (n + 4) * 2.0 ** -52                             # t - c, its square and n additions, each rounded to float64
        slack = 2 * np.abs(d).sum(axis=0) * delta + n * delta * delta + exact * want
        assert (np.abs(got[i, 12:23] - want) <= slack).all(), (i, np.abs(got[i, 12:23] - want) / slack)
        assert (np.abs(got[i, 1:12] - d.sum(axis=0)) <= n * delta + exact * np.abs(d).sum(axis=0)).all()


GUARD = 256


def _raw_call(conf, imdb, idx, fs, center=None, fill=None):
    """m3d_rpn_target_stats through the C ABI on caller-made buffers: `out` and the workspace pre-filled with `fill`, a guard
    pattern behind each.  Returns the rows as bytes per image and checks the guards."""
    L, dev = _hip.lib(), _dev()
    table = ds.pack_gts_scaled(conf, [imdb[i] for i in idx])
    B, A = len(idx), conf.anchors.shape[0]
    R = A * fs[0] * fs[1]
    nbytes = L.m3d_rpn_target_stats_workspace_bytes(B, R)
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.empty(256 + nbytes + GUARD, device=dev, dtype=torch.uint8)
    off = (-ws.data_ptr()) % 256
    out = torch.empty(B * NC + 32, device=dev, dtype=torch.float64)
    if fill is not None:
        poison.poison_(out, fill)
        ws.fill_({"zero": 0x00, "nan": 0xFF, "huge": 0x7F}[fill])
    ws[off + nbytes:off + nbytes + GUARD] = 0xA5
    out[B * NC:] = -7.25
    anc = torch.from_numpy(np.ascontiguousarray(conf.anchors)).to(dev)
    gt = torch.from_numpy(table).to(dev)
    cen = torch.from_numpy(np.zeros(11) if center is None else np.ascontiguousarray(center, dtype=np.float64)).to(dev)
    vec = ds.stats_conf_vec(conf)
    _hip.check(L.m3d_rpn_target_stats(anc.data_ptr(), A, fs[0], fs[1], vec.ctypes.data, int(vec.size), gt.data_ptr(), B, table.shape[1] - 1,
                                      cen.data_ptr(), out.data_ptr(), ws.data_ptr() + off, nbytes, _stream()))
    torch.cuda.synchronize()
    assert bool((ws[off + nbytes:off + nbytes + GUARD] == 0xA5).all()), "the guard behind the workspace was written"
    assert bool((out[B * NC:] == -7.25).all()), "the guard behind `out` was written"
    # short of the full size by one byte: refused, nothing launched
    assert L.m3d_rpn_target_stats(anc.data_ptr(), A, fs[0], fs[1], vec.ctypes.data, int(vec.size), gt.data_ptr(), B, table.shape[1] - 1,
                                  cen.data_ptr(), out.data_ptr(), ws.data_ptr() + off, nbytes - 1, _stream()) == -3
    o = out[:B * NC].view(B, NC).cpu().numpy()
    return [o[k].tobytes() for k in range(B)]


def test_a_row_has_the_same_bits_alone_in_a_batch_in_another_slot_and_over_poison(G, case, rows):
    conf, imdb = case
    fs = (4, 159)
    idx = [i for i in range(len(imdb)) if tuple(G["feat_sizes"][i]) == fs]
    assert idx == [1, 4, 7]                                  # 12 fg rows, no gts, 4 fg rows
    want = {i: rows[i].tobytes() for i in idx}               # through the host layer, grouped as compute_bbox_stats groups them
    for i in idx:
        assert _raw_call(conf, imdb, [i], fs) == [want[i]]
    for order in ([1, 4, 7], [7, 1, 4], [4, 7, 1, 1]):
        for fill in ("zero", "nan", "huge"):
            got = _raw_call(conf, imdb, order, fs, fill=fill)
            assert got == [want[i] for i in order], (order, fill)
    c = G["bbox_means"][0]
    a = _raw_call(conf, imdb, [1], fs, center=c, fill="nan")
    b = _raw_call(conf, imdb, [7, 4, 1], fs, center=c, fill="huge")
    assert a[0] == b[2] and a[0] != want[1]


def test_the_host_layer_over_poisoned_allocations(case, rows, monkeypatch):
    conf, imdb = case
    for fill in ("nan", "huge"):
        with poison.poisoned_allocations(fill, monkeypatch=monkeypatch) as st:
            got = ds.image_target_stats(conf, imdb)
        assert st.from_file("m3dssd_amd/host/loss.py") >= 2 * 4          # out + workspace of each of the four feature sizes
        assert got.tobytes() == rows.tobytes(), fill


def test_the_operator_refuses_what_it_cannot_compute(case):
    conf, imdb = case
    dev = _dev()
    vec, table = ds.stats_conf_vec(conf), ds.pack_gts_scaled(conf, imdb[:1])
    out = ops.rpn_target_stats(conf.anchors, vec, table, (4, 160))
    assert out.dtype == torch.float64 and tuple(out.shape) == (1, NC) and out.is_cuda
    with pytest.raises(RuntimeError, match="center must hold 11"):
        ops.rpn_target_stats(conf.anchors, vec, table, (4, 160), center=np.zeros(4))
    with pytest.raises(RuntimeError, match="anchors must be float64"):
        ops.rpn_target_stats(torch.zeros(12, 9, device=dev), vec, table, (4, 160))
    big = np.zeros((1, hl.MAX_GT + 2, hl.GT_COLS))
    with pytest.raises(RuntimeError, match="M3D_RPN_MAX_GT"):
        ops.rpn_target_stats(conf.anchors, vec, big, (4, 160))
    with pytest.raises(RuntimeError, match="M3D_RPN_CONF_COUNT"):
        ops.rpn_target_stats(conf.anchors, vec[:-1], table, (4, 160))
    ones = vec.copy()
    ones[:22] = 0.0                                          # means and stds of the conf vector are not read: zero stds are fine
    assert ops.rpn_target_stats(conf.anchors, ones, table, (4, 160)).cpu().numpy().tobytes() == out.cpu().numpy().tobytes()


def test_the_float_path_is_untouched():
    """m3d_rpn_precompute_targets gives the bits the library built from the commit before the roi arithmetic became generic gave
    (tests/golden/rpn_precompute_bits.npz, tools/gen_golden_rpn_precompute_bits.py)."""
    from tools import gen_golden_rpn_precompute_bits as PB
    _dev()
    P = np.load(os.path.join(GOLDEN, "rpn_precompute_bits.npz"))
    for name in PB.CASES:
        bits = PB.precompute_bits(name)
        for k in PB.KEYS:
            if name == "odd":
                assert bits[k].dtype == P["odd_" + k].dtype and np.array_equal(bits[k].view(np.uint8), P["odd_" + k].view(np.uint8)), k
            assert PB.digest(bits[k]) == str(P["%s_%s_sha256" % (name, k)]), (name, k)
