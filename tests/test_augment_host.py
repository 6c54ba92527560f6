"""CPU tests of the training augmentation's host side (m3dssd_amd/host/augment.py) against tests/golden/augment.npz, which
tools/gen_golden_augment.py wrote by running the reference's own ``Augmentation(conf)`` from seeds: the random draws and the
label rewrite must be the reference's bit for bit, the float32 restatement of the image path (tests/augment_ref.py) driven by
``draw_params`` must reproduce the golden images."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from m3dssd_amd import _hip
from m3dssd_amd.host import augment as A

import augment_cases as AC
import augment_ref as AR

CASES = AR.golden_cases()
IDS = [c[0] for c in CASES]


def _sizes(frames):
    return [f.shape[:2] for f in frames]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_labels_from_the_seed_are_the_references_bit_for_bit(case):
    name, conf, seed, frames, imobjs, size, images, want, scale_factors = case
    params = A.draw_params(conf, _sizes(frames), np.random.RandomState(seed))
    for i, (imobj, p) in enumerate(zip(imobjs, params)):
        before = copy.deepcopy(imobj)
        got = A.transform_labels(imobj, p)
        fields = AR.label_fields(got)
        for k in AR.GT_FIELDS:
            assert _same_bits(fields[k], want[i][k]), (name, i, k, fields[k], want[i][k])
        assert float(got.scale_factor) == scale_factors[i]
        assert float(p["scale"]) == scale_factors[i]
        for k in AR.GT_FIELDS:                                           # a deep copy: the input is untouched
            assert _same_bits(AR.label_fields(imobj)[k], AR.label_fields(before)[k])


def test_the_global_numpy_rng_is_drawn_like_a_random_state():
    name, conf, seed, frames = CASES[IDS.index("photo_half")][:4]
    want = A.draw_params(conf, _sizes(frames), np.random.RandomState(seed))
    state = np.random.get_state()
    try:
        np.random.seed(seed)
        got = A.draw_params(conf, _sizes(frames))
    finally:
        np.random.set_state(state)
    assert [A.pack_params([p]).tobytes() for p in got] == [A.pack_params([p]).tobytes() for p in want]


def test_the_golden_covers_what_it_was_built_for():
    modes, scales, mirrors, warps = set(), set(), set(), set()
    for name, conf, seed, frames, imobjs, size, images, want, sf in CASES:
        for p in A.draw_params(conf, _sizes(frames), np.random.RandomState(seed)):
            modes.add(p["mode"])
            scales.add(float(p["scale"]))
            mirrors.add(p["mirror"])
            warps.add(p["warped"])
    assert modes == {0, 1, 2} and {0.6, 1.4, 1.0} <= scales and mirrors == {False, True} and warps == {False, True}
    assert any(s not in (0.6, 1.0, 1.4) for s in scales)


def test_neutral_parameters_and_the_folded_matrix():
    p = A.make_params(13, 37)
    assert (p["mode"], p["delta"], p["alpha"], p["sat"], p["hue"]) == (0, 0.0, 1.0, 1.0, 0.0)
    assert np.array_equal(p["M"], [[1, 0, 0], [0, 1, 0]]) and np.array_equal(p["Minv"], [[1, 0, 0], [0, 1, 0]])
    m = A.make_params(13, 37, mirror=True)
    assert np.array_equal(m["Minv"], [[-1, 0, 36], [0, 1, 0]])
    q = A.make_params(20, 36, scale=1.4, centre=(20.0, 9.0), warped=True, mirror=True)
    fwd = AR.get_rotation_matrix_2d((20.0, 9.0), 0, 1.4)
    assert np.array_equal(q["M"], fwd)
    inv = AR.invert_affine(fwd)
    assert np.array_equal(q["Minv"][1], inv[1]) and np.array_equal(q["Minv"][0], [-inv[0, 0], -inv[0, 1], 35 - inv[0, 2]])
    rows = A.pack_params([p, q])
    assert rows.shape == (2, A.PARAM_COLS) and rows.dtype == np.float64
    assert rows[1, :3].tolist() == [20, 36, 0] and np.array_equal(rows[1, 8:], q["Minv"].reshape(6))


def test_images_from_the_seed_match_the_golden():
    # measured: max |float32 restatement - float64 restatement| over the golden cases = 2.2e-6 (normalised units, values up
    # to 2.6; the photometric cases set it); two correct float32 evaluations differ by operation order, 4x covers
    # a few reorderings.  A wrong draw order moves pixels by whole grey levels (1 / 255 / 0.229 = 1.7e-2).
    gap = AC.golden_gap()
    bound = 4 * gap
    worst = 0.0
    for name, conf, seed, frames, imobjs, size, images, want, sf in CASES:
        params = A.draw_params(conf, _sizes(frames), np.random.RandomState(seed))
        got = np.stack([AR.augment_image(f, p, size, dtype=np.float32) for f, p in zip(frames, params)])
        assert got.shape == images.shape and got.dtype == np.float32
        err = float(np.abs(got.astype(np.float64) - images).max())
        print("augment golden", name, "max err %.3e" % err)
        worst = max(worst, err)
        assert err <= bound, (name, err, bound)
    print("augment: float32-float64 restatement gap %.3e, bound %.3e, worst golden error %.3e" % (gap, bound, worst))
    assert 0 < gap < 1e-3


def test_the_border_is_a_normalised_zero_not_a_distorted_zero():
    rng = np.random.RandomState(3)
    frame = rng.randint(40, 216, size=(13, 37, 3)).astype(np.uint8)
    p = A.make_params(13, 37, mode=A.MODE_CONTRAST_FIRST, delta=20.0, alpha=1.3, sat=1.2, hue=10.0, scale=0.6, centre=(18.5, 6.5), warped=True)
    mask = AR.border_mask(p["Minv"], 13, 37, 16, 38)
    assert mask.any() and not mask.all()
    mean, stds = np.asarray(AR.MEAN, np.float32), np.asarray(AR.STDS, np.float32)
    zero = ((np.float32(0) / np.float32(255) - mean) / stds)[::-1]                                   # RGB plane order
    distorted = (((np.float32(20.0) * np.float32(1.3)) / np.float32(255) - mean) / stds)[::-1]
    for dtype in (np.float32, np.float64):
        out = AR.augment_image(frame, p, (16, 38), dtype=dtype)
        want = ((dtype(0) / dtype(255) - mean.astype(dtype)) / stds.astype(dtype))[::-1]
        for c in range(3):
            assert (out[c][mask] == want[c]).all()
            assert not np.isclose(out[c][mask], distorted[c]).any()
    # a source smaller than the destination without a warp: the padding at the bottom / right is the same zero
    q = A.make_params(13, 37)
    out = AR.augment_image(frame, q, (16, 38))
    assert (out[:, 13:, :] == zero[:, None, None]).all() and (out[:, :, 37:] == zero[:, None, None]).all()
    assert np.array_equal(out[:, :13, :37], AR.normalise(frame.astype(np.float32), AR.MEAN, AR.STDS)[:, :, ::-1].transpose(2, 0, 1))


def test_host_side_errors():
    p = [A.make_params(13, 37)]
    frames = torch.zeros(1, 13, 37, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="uint8"):
        A.augment_batch(frames.float(), p, (16, 38), AR.MEAN, AR.STDS)
    with pytest.raises(RuntimeError, match="uint8"):
        A.augment_batch(frames[0], p, (16, 38), AR.MEAN, AR.STDS)
    with pytest.raises(RuntimeError, match="uint8"):
        A.augment_batch(torch.zeros(1, 13, 37, 4, dtype=torch.uint8), p, (16, 38), AR.MEAN, AR.STDS)
    with pytest.raises(RuntimeError, match="parameter sets"):
        A.augment_batch(frames, p + p, (16, 38), AR.MEAN, AR.STDS)
    with pytest.raises(RuntimeError, match="does not fit"):
        A.augment_batch(frames, [A.make_params(14, 37)], (16, 38), AR.MEAN, AR.STDS)
    bad = A.make_params(13, 37)
    bad["Minv"] = np.zeros((2, 3))
    with pytest.raises(RuntimeError, match="singular"):
        A.augment_batch(frames, [bad], (16, 38), AR.MEAN, AR.STDS)
    bad["Minv"] = np.array([[1.0, 0.0, np.nan], [0.0, 1.0, 0.0]])
    with pytest.raises(RuntimeError, match="finite"):
        A.augment_batch(frames, [bad], (16, 38), AR.MEAN, AR.STDS)
    with pytest.raises(NotImplementedError):
        A.augment_batch(frames, p, (16, 38), AR.MEAN, AR.STDS, device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(NotImplementedError):
            A.augment_batch(frames, p, (16, 38), AR.MEAN, AR.STDS)
        conf = AR.AttrDict(crop_size=[16, 38], image_means=AR.MEAN, image_stds=AR.STDS, distort_prob=-1, mirror_prob=0.5, trans_prob=0.7,
                           shift=0.1, scale_trans=0.4)
        with pytest.raises(NotImplementedError):
            A.TrainAugmentation(conf)(frames, [AR.AttrDict(gts=[], p2_inv=np.eye(4))])


@pytest.mark.parametrize("photo,mirror_first,dest", AC.PARITY_IDS)
def test_the_float32_restatement_stays_inside_the_device_bound(photo, mirror_first, dest):
    """The device test allows 4x the float32-float64 restatement gap of these cases (measured: 2.3e-6 in normalised units): the
    float32 restatement itself must sit inside it, every photometric input must stay positive (a well-conditioned HSV step), and
    every case must have border pixels and interior pixels."""
    buf, params, r32, r64, masks = AC.parity_case(photo, mirror_first, dest)
    gap = AC.parity_gap()
    print("augment parity gap %.3e" % gap)
    assert 0 < gap < 1e-4
    assert np.abs(r32 - r64).max() <= 4 * gap
    for f, p in zip(buf, params):
        lo = (float(f[:p["h"], :p["w"]].min()) + p["delta"]) * (p["alpha"] if p["mode"] == 1 else 1.0)
        assert lo > 0
    assert masks.any() and not masks.all()
    zero = AC.border_value()
    for c in range(3):
        assert ((r32[:, c] == zero[c]) == masks).all()


def _call(frames, N, hmax, wmax, rows, stride, out, H, W, mean=AR.MEAN, stds=AR.STDS):
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*stds)
    ptr = None if rows is None else rows.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    return _hip.lib().m3d_augment_u8(frames, N, hmax, wmax, ptr, stride, m3, s3, out, H, W, None)


def test_the_library_rejects_bad_arguments_before_it_touches_the_device():
    """Every check of m3d_augment_u8 runs before its first launch, so the error paths need no device: the pointers given here
    are never dereferenced."""
    frames, out = 0x1000, 0x2000
    good = A.pack_params([A.make_params(13, 37)])

    def rc(**kw):
        a = dict(frames=frames, N=1, hmax=13, wmax=37, rows=good, stride=A.PARAM_COLS, out=out, H=16, W=38)
        a.update(kw)
        code = _call(**a)
        return code, _hip.lib().m3d_last_error().decode()

    for kw, text in ((dict(frames=None), "null"), (dict(out=None), "null"), (dict(rows=None), "null"), (dict(N=0), "bad sizes"),
                     (dict(N=-3), "bad sizes"), (dict(stride=13), "bad sizes"), (dict(H=0), "bad sizes"),
                     (dict(hmax=12), "does not fit"), (dict(wmax=36), "does not fit")):
        code, msg = rc(**kw)
        assert code != 0 and text in msg, (kw, code, msg)
    for col, val, text in ((8, 0.0, "singular"), (12, 0.0, "singular"), (10, np.nan, "not finite"), (9, np.inf, "not finite"),
                           (0, 0.0, "does not fit"), (1, 37.5, "does not fit"), (2, 3.0, "mode"), (6, 400.0, "hue")):
        rows = good.copy()
        rows[0, col] = val
        code, msg = rc(rows=rows)
        assert code != 0 and text in msg, (col, val, code, msg)
    two = np.concatenate([good, good])              # the second image is checked before the first is launched
    two[1, 0] = 14
    code, msg = rc(rows=two, N=2)
    assert code != 0 and "image 1" in msg
    code, msg = rc(stds=[0.229, 0.0, 0.225])
    assert code != 0 and "std" in msg
