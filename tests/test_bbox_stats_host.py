"""CPU checks of generate_anchors / compute_bbox_stats (m3dssd_amd/host/dataset_stats.py): the yardstick of the GPU tests
(tests/bbox_stats_ref.py) is pinned bit for bit against the reference's own numbers (tests/golden/bbox_stats.npz,
tools/gen_golden_bbox_stats.py), and the host layer is checked: the anchors, the packed gt tables, the grouping, the caches, the
refusals, the shim and the C ABI's new names."""
import os
import pickle
import re

import numpy as np
import pytest

from m3dssd_amd import _hip
from m3dssd_amd.host import dataset_stats as ds
from m3dssd_amd.host import loss as hl

import bbox_stats_ref as BR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bbox_stats.npz")


@pytest.fixture(scope="module")
def G():
    return dict(np.load(GOLDEN))


def _case(G, anchors=True):
    conf, imdb = BR.conf_from_arrays(G), BR.imdb_from_arrays(G)
    if anchors:
        conf.anchors = np.array(G["anchors"])
    return conf, imdb


def test_restatement_equals_the_reference_bit_for_bit(G):
    conf, imdb = _case(G, anchors=False)
    assert float(G["threshold_gap"]) > 1e-9
    anchors, _ = BR.generate_anchors(conf, imdb)
    assert anchors.dtype == np.float64 and anchors.tobytes() == G["anchors"].tobytes()
    conf.anchors = anchors
    means, stds = BR.compute_bbox_stats(conf, imdb)
    assert means.shape == stds.shape == (1, 11) and means.dtype == stds.dtype == np.float64
    assert means.tobytes() == G["bbox_means"].tobytes() and stds.tobytes() == G["bbox_stds"].tobytes()
    for i, im in enumerate(imdb):
        p = BR.image_transforms(conf, im)
        n, s, sa, mx = BR.image_sums(None if p is None else p[0])
        assert n == int(G["n_fg"][i])
        assert s.tobytes() == G["sum_t"][i].tobytes() and sa.tobytes() == G["sum_abs_t"][i].tobytes() and mx.tobytes() == G["max_abs_t"][i].tobytes()


def test_float32_rois_are_told_apart_by_the_bound_of_the_device_test(G):
    """The fixture is worth its width: with the loss path's float32 rois the sums of the columns without a logarithm miss the
    bound the device test holds the float64 kernel to (n_fg * 2^-53 * sum |t|), in some image, by orders of magnitude."""
    conf, imdb = _case(G)
    worst = 0.0
    for i, im in enumerate(imdb):
        n = int(G["n_fg"][i])
        if n == 0:
            continue
        n32, s32, _, _ = BR.image_sums(BR.image_transforms(conf, im, rois_dtype=np.float32)[0])
        assert n32 == n
        for c in (0, 1, 4, 5):
            worst = max(worst, abs(s32[c] - G["sum_t"][i, c]) / (n * 2.0 ** -53 * G["sum_abs_t"][i, c]))
    assert worst > 1e3, worst


def test_generate_anchors_equals_the_reference_bit_for_bit(G):
    conf, imdb = _case(G, anchors=False)
    ds.generate_anchors(conf, imdb, None)
    assert conf.anchors.dtype == np.float64 and conf.anchors.shape == (12, 9)
    assert conf.anchors.tobytes() == G["anchors"].tobytes()
    conf.has_3d = False                                   # 2-D only: the float32 anchors of scales x ratios
    ds.generate_anchors(conf, imdb, None)
    assert conf.anchors.dtype == np.float32 and conf.anchors.shape == (12, 4)
    assert np.array_equal(conf.anchors.astype(np.float64), G["anchors"][:, :4])


def test_packed_tables_equal_what_the_restatement_feeds_compute_targets(G):
    conf, imdb = _case(G)
    table = ds.pack_gts_scaled(conf, imdb)
    assert table.dtype == np.float64 and table.shape[0] == len(imdb) and table.shape[2] == hl.GT_COLS
    seen_ign = seen_val = 0
    for b, im in enumerate(imdb):
        nv, ni = int(table[b, 0, 0]), int(table[b, 0, 1])
        if len(im.gts) == 0:
            assert nv == ni == 0 and not table[b].any()
            continue
        fs, val, ign, lbls, g3 = BR.image_inputs(conf, im)
        assert tuple(int(v) for v in fs) == ds.image_feat_size(conf, im) == tuple(int(v) for v in G["feat_sizes"][b])
        assert (nv, ni) == (len(val), len(ign))
        assert table[b, 1:1 + nv, 0:4].tobytes() == val.tobytes()
        assert np.array_equal(table[b, 1:1 + nv, 4], lbls.astype(np.float64))
        assert table[b, 1:1 + nv, 5:12].tobytes() == np.ascontiguousarray(g3[:, :7]).tobytes()
        assert table[b, 1 + nv:1 + nv + ni, 0:4].tobytes() == ign.tobytes()
        assert not table[b, 1 + nv + ni:].any()
        seen_val, seen_ign = seen_val + nv, seen_ign + ni
    assert seen_val > 0 and seen_ign > 0
    assert int(table[4, 0, 0]) == 0 and int(table[6, 0, 0]) == 0 and int(table[6, 0, 1]) > 0      # no gts; all ignored
    # the loss path's packing is another function with another result (no scale factor): untouched
    assert hl.pack_gts(imdb[1:2], conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h).tobytes() != ds.pack_gts_scaled(conf, imdb[1:2]).tobytes()


def test_more_than_128_ground_truths_in_an_image_is_an_error(G):
    conf, imdb = _case(G)
    im = imdb[0].copy()
    im.gts = [imdb[0].gts[0]] * (hl.MAX_GT + 1)
    with pytest.raises(RuntimeError, match="exceed the kernel's cap of 128"):
        ds.pack_gts_scaled(conf, [im])


def test_grouping_by_feature_size_covers_every_image_once(G):
    conf, imdb = _case(G)
    plan = ds.group_by_feat_size(conf, imdb, chunk=2)
    idx = [i for _fs, part in plan for i in part]
    assert sorted(idx) == list(range(len(imdb)))
    assert len({fs for fs, _ in plan}) == len({tuple(f) for f in G["feat_sizes"].tolist()}) >= 3
    for fs, part in plan:
        assert 1 <= len(part) <= 2 and all(tuple(G["feat_sizes"][i]) == fs for i in part)
    assert len(ds.group_by_feat_size(conf, imdb)) == len({fs for fs, _ in plan})


def test_cache_round_trip_and_a_hit_needs_no_device(G, tmp_path, monkeypatch):
    conf, imdb = _case(G, anchors=False)
    folder = str(tmp_path)
    ds.generate_anchors(conf, imdb, folder)
    with open(os.path.join(folder, "anchors.pkl"), "rb") as f:
        assert pickle.load(f).tobytes() == G["anchors"].tobytes()                    # a plain pickle under the reference's name
    conf2, _ = _case(G, anchors=False)
    ds.generate_anchors(conf2, [], folder)                                           # a hit reads no imdb
    assert conf2.anchors.tobytes() == G["anchors"].tobytes()
    for name, arr in (("bbox_means.pkl", G["bbox_means"]), ("bbox_stds.pkl", G["bbox_stds"])):      # as the reference writes them
        with open(os.path.join(folder, name), "wb") as f:
            pickle.dump(arr, f)
    monkeypatch.setattr(hl, "rpn_target_stats", lambda *a, **k: pytest.fail("a cache hit touched the device"))
    conf2.device = "cpu"
    ds.compute_bbox_stats(conf2, imdb, folder)
    assert conf2.bbox_means.tobytes() == G["bbox_means"].tobytes() and conf2.bbox_stds.tobytes() == G["bbox_stds"].tobytes()
    os.remove(os.path.join(folder, "bbox_stds.pkl"))                                  # both files make a hit, one does not
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ds.compute_bbox_stats(conf2, imdb, folder)


def test_cluster_anchors_is_refused(G):
    conf, imdb = _case(G, anchors=False)
    conf.cluster_anchors = 1
    with pytest.raises(NotImplementedError, match="cluster_anchors"):
        ds.generate_anchors(conf, imdb, None)


def test_an_unused_anchor_raises_like_the_reference(G):
    conf, imdb = _case(G, anchors=False)
    conf.anchor_scales = np.concatenate([conf.anchor_scales, [200.0]])            # no ground truth is that large: anchors 12-14
    with pytest.raises(ValueError, match=r"Non-used anchor #12 found"):
        ds.generate_anchors(conf, imdb, None)
    with pytest.raises(ValueError, match=r"Non-used anchor #12 found"):
        BR.generate_anchors(conf, imdb)


def test_no_device_and_no_cache_is_refused(G):
    conf, imdb = _case(G)
    conf.device = "cpu"
    with pytest.raises(NotImplementedError, match="no cache and no ROCm device"):
        ds.compute_bbox_stats(conf, imdb, None)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        hl.rpn_target_stats(conf.anchors, ds.stats_conf_vec(conf), ds.pack_gts_scaled(conf, imdb[:1]), (4, 160), device="cpu")
    conf.has_3d = False
    with pytest.raises(NotImplementedError, match="has_3d"):
        ds.compute_bbox_stats(conf, imdb, None)


def test_the_shim_exposes_both_names():
    import lib.rpn_util as shim
    from lib.rpn_util import compute_bbox_stats, generate_anchors
    assert shim.generate_anchors is ds.generate_anchors is generate_anchors
    assert shim.compute_bbox_stats is ds.compute_bbox_stats is compute_bbox_stats


def test_header_signature_table_and_library_agree_on_the_new_names():
    L = _hip.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(_hip.HEADER).read(), flags=re.S)
    for name, nargs in (("m3d_rpn_target_stats_workspace_bytes", 2), ("m3d_rpn_target_stats", 14)):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs
        assert hasattr(L, name) and name in _hip.SIGNATURES
        assert len(_hip.SIGNATURES[name][1]) == nargs
    assert L.m3d_abi_version() == 5                                 # additive: the number does not move
    assert int(re.search(r"M3D_RPN_TARGET_STATS_COLS\s+(\d+)", hdr).group(1)) == hl.TARGET_STATS_COLS == 23
    f = L.m3d_rpn_target_stats_workspace_bytes
    assert f(0, 100) == -1 and f(1, 0) == -1
    one, two = f(1, 7680), f(2, 7680)
    assert 0 < one < two and f(1, 7681) > one                        # 30 -> 31 workgroups
