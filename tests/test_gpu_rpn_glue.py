"""GPU tests (-m gpu; every call goes through the C ABI of libm3dssd_hip.so) of the small kernels between the heavy ones: anchor
selection, fg top-1, alignment offsets, row softmax, output bundling / sort keys (csrc/rpn_kernels.hip) and max-pool, layout
changes, weight packing (csrc/backbone_kernels.hip).  They take the model's discrete decisions (foreground anchor of a pixel,
hard mask at the threshold) and move data between layouts; the whole-network tests forgive exactly those decisions at near-ties.

References are numpy / torch in float64, written here from the formulas the kernel comments cite (M3d_inference_align.py:229-234,
feturealign_mgpu.py:58-89,160-183, attention.py:208).  Three comparisons carry a derived bound, everything else is equality:
  * class softmax (fg_all, prob, keys) and row softmax: |err| <= 1e-6.  Every intermediate lies in [0, 1]; expf is within 1 ulp,
    then at most 8 additions (row softmax: a 6-level tree over per-lane sums), one division and one subtraction -> about
    12 * 2^-24 = 7e-7; the same expressions in numpy float32 differ from float64 by 2.0e-7 / 3.6e-7 on these inputs.
  * center_align offsets: |err| <= 4 * 2^-24 * (|b * std| + |mean|) * |anchor| (three fp32 roundings, 2^-24 relative each, on
    terms bounded by (|b * std| + |mean|) * |anchor|; the fourth unit covers the products of the (1 + eps) factors).
Every output buffer has a guard region on both sides (and its pad columns, where it has any) pre-filled with a sentinel bit
pattern; every test asserts that they are untouched.  Measured on the MI355X (logged through gpu_common._log): fg_all 3.1e-7,
keys 2.0e-7, bundled prob 1.8e-7, row softmax 2.8e-7, center_align 0.48 of its bound; 99.97 % of the pixels of the std-10 case tie."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from m3dssd_amd import _hip
from gpu_common import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu

SENT = -559038737          # 0xDEADBEEF as int32 (as a float: -6.26e18, finite, never a result of these kernels)
GUARD = 64                 # 4-byte elements on each side: 256 bytes, so the payload keeps the allocation's alignment
HW_EDGES = (1, 63, 64, 65, 257)


class Guarded:
    """n 4-byte elements on the device between two sentinel-filled guard regions; `shift` moves the payload by that many
    elements (shift = 1: a base that is 4-byte but not 16-byte aligned)."""

    def __init__(self, n, dtype=torch.float32, shift=0):
        self.n, self.lo = int(n), GUARD + shift
        self.raw = torch.full((self.lo + self.n + GUARD,), SENT, dtype=torch.int32, device=_dev())
        self.t = self.raw[self.lo:self.lo + self.n].view(dtype)
        self.ptr = self.t.data_ptr()
        assert self.ptr % 16 == (4 * shift) % 16

    def put(self, arr):
        a = np.ascontiguousarray(arr)
        assert a.size == self.n and a.dtype.itemsize == 4
        self.t.copy_(torch.from_numpy(a.reshape(-1).view(np.int32)).to(self.t.device).view(self.t.dtype))
        return self

    def get(self, dtype=np.float32):
        """Payload as a numpy array (synchronises), after asserting that both guards still hold the sentinel."""
        raw = self.raw.cpu().numpy()
        assert (raw[:self.lo] == SENT).all(), "write below the buffer"
        assert (raw[self.lo + self.n:] == SENT).all(), "write beyond the buffer"
        return raw[self.lo:self.lo + self.n].view(dtype).copy()

    def untouched(self):
        return bool((self.get(np.int32) == SENT).all())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _f32(x):
    return float(np.float32(x))


def _sortable(f):
    """The documented key of a float32 (common.h f32_sortable; gpu_common._sortable_bits): monotone unsigned image."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    return _sortable_bits(torch.from_numpy(f)).numpy().astype(np.uint32).reshape(f.shape)


def _unsortable(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _softmax64(x, axis):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


# ======================================================================================== 1. anchor selection
def _logits(B, A, NC, HW, std, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, NC, A, HW)) * std).astype(np.float32)      # channel = cls * A + a


def _select(l, fg=True, keys=False):
    """One launch of m3d_anchor_select (fg_all written or NULL) or m3d_anchor_select_keys on logits [B][NC][A][HW]."""
    L = _hip.lib()
    B, NC, A, HW = l.shape
    d = Guarded(l.size).put(l)
    idx, prob = Guarded(B * HW, torch.int32), Guarded(B * HW)
    extra = Guarded(B * A * HW) if (fg or keys) else None
    if keys:
        assert NC == 4
        _hip.check(L.m3d_anchor_select_keys(d.ptr, B, A, HW, idx.ptr, prob.ptr, extra.ptr, _stream()))
    else:
        _hip.check(L.m3d_anchor_select(d.ptr, B, A, NC, HW, idx.ptr, prob.ptr, extra.ptr if fg else None, _stream()))
    i, p = idx.get(np.int32).reshape(B, HW), prob.get().reshape(B, HW)
    e = None if extra is None else extra.get(np.uint32 if keys else np.float32).reshape(B, A, HW)
    assert np.array_equal(_bits(d.get()), _bits(l).reshape(-1)), "input modified"
    return i, p, e


def _keys_planar(l):
    L = _hip.lib()
    B, NC, A, HW = l.shape
    d, k = Guarded(l.size).put(l), Guarded(B * A * HW, torch.int32)
    _hip.check(L.m3d_score_keys_planar(d.ptr, k.ptr, B, A, HW, _stream()))
    return k.get(np.uint32).reshape(B, A, HW)


def _bundle(l, box):
    """m3d_bundle_outputs on planar logits [B][4][A][HW] and boxes [B][11][A][HW] -> cls, prob, bbox_2d, bbox_3d, keys."""
    L = _hip.lib()
    B, NC, A, HW = l.shape
    R = A * HW
    d, bx = Guarded(l.size).put(l), Guarded(box.size).put(box)
    o = [Guarded(B * R * 4), Guarded(B * R * 4), Guarded(B * R * 4), Guarded(B * R * 7), Guarded(B * R, torch.int32)]
    _hip.check(L.m3d_bundle_outputs(d.ptr, bx.ptr, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, o[4].ptr, B, A, HW, _stream()))
    return (o[0].get().reshape(B, R, 4), o[1].get().reshape(B, R, 4), o[2].get().reshape(B, R, 4), o[3].get().reshape(B, R, 7),
            o[4].get(np.uint32).reshape(B, R))


def _check_keys(name, keys, l):
    """keys [B][A][HW] against float64 max(softmax[1:]) (<= 1e-6) and their unsigned order against the float order."""
    score = _unsortable(keys)
    err = float(np.abs(score.astype(np.float64) - _softmax64(l, 1)[:, 1:].max(axis=1)).max())
    assert err <= 1e-6, (name, err)
    assert np.array_equal(_sortable(score), keys)
    k, f = keys.reshape(-1), score.reshape(-1)
    order = np.argsort(k, kind="stable")
    ks, fs = k[order], f[order]
    assert (np.diff(fs) >= 0).all() and np.array_equal(np.diff(ks.astype(np.int64)) == 0, np.diff(fs) == 0), name
    return err


def _check_select_case(B, A, NC, HW, std, seed):
    name = "B%d A%d NC%d HW%d std%g" % (B, A, NC, HW, std)
    l = _logits(B, A, NC, HW, std, seed)
    idx, prob, fg = _select(l, fg=True)
    # fg_all against float64
    ref = 1.0 - _softmax64(l, 1)[:, 0]
    err = float(np.abs(fg.astype(np.float64) - ref).max())
    print("anchor_select %s: max|fg_all - f64| = %.3e" % (name, err))
    assert err <= 1e-6, (name, err)
    # the selection: first maximum of the kernel's own fg_all, bit for bit, at every pixel
    assert not np.isnan(fg).any()
    assert np.array_equal(idx, np.argmax(fg, axis=1)), name
    assert np.array_equal(_bits(prob), _bits(fg.max(axis=1))), name
    # production form: fg_all = NULL, and the keys entry point
    i2, p2, _ = _select(l, fg=False)
    assert np.array_equal(i2, idx) and np.array_equal(_bits(p2), _bits(prob)), name
    kerr = 0.0
    if NC == 4 and A >= 4:
        i3, p3, keys = _select(l, keys=True)
        assert np.array_equal(i3, idx) and np.array_equal(_bits(p3), _bits(prob)), name
        kerr = _check_keys(name, keys, l)
        if HW % 4 == 0:
            assert np.array_equal(_keys_planar(l), keys), name
        box = np.random.default_rng(seed + 1).standard_normal((B, 11, A, HW)).astype(np.float32)
        assert np.array_equal(_bundle(l, box)[4].reshape(B, A, HW), keys), name
    ties = float(((fg == fg.max(axis=1, keepdims=True)).sum(axis=1) >= 2).mean())
    return err, kerr, ties


def test_anchor_select_shipped_shape_saturated():
    """A = 36, NC = 4, HW = 48 * 160, B = 3, logits of standard deviation 10: saturated probabilities, exact ties the common case."""
    err, kerr, ties = _check_select_case(3, 36, 4, 48 * 160, 10.0, 100)
    _log("rpn_glue.anchor_select_shipped", {"fg_err": err, "key_err": kerr, "tie_fraction": ties})
    assert ties >= 0.5, "the std = 10 case no longer exercises the tie rule (%.3f of the pixels tie)" % ties


@pytest.mark.parametrize("A,NC", [(36, 4), (4, 4), (5, 4), (6, 4), (7, 4), (9, 4), (13, 4), (3, 4), (5, 2), (7, 3), (36, 8), (1, 4)])
def test_anchor_select_matches_float64_and_own_argmax(A, NC):
    """Wave kernel (NC = 4, A >= 4: empty wave groups, ranges shorter than the unroll, tails of 1 and 2) and generic kernel;
    HW around the 64-pixel block and the 256-thread block; logit scales 1, 3, 10."""
    worst, worst_k = 0.0, 0.0
    for hi, HW in enumerate(HW_EDGES + (256, 60)):
        for si, std in enumerate((1.0, 3.0, 10.0)):
            err, kerr, _ = _check_select_case(2, A, NC, HW, std, 1000 * A + 100 * NC + 10 * hi + si)
            worst, worst_k = max(worst, err), max(worst_k, kerr)
    _log("rpn_glue.anchor_select", {"A": A, "NC": NC, "fg_err": worst, "key_err": worst_k})


def _tie_logits(NC, fgclass):
    """Two logit vectors: `low` (background 2 above the rest: fg = (NC-1) / (e^2 + NC-1)) and `high` (one foreground class 1
    above the rest).  Identical logits give bit-identical fg, whatever the rounding."""
    low, high = np.zeros(NC, np.float32), np.zeros(NC, np.float32)
    low[0] = 2.0
    high[fgclass] = 1.0
    return low, high


@pytest.mark.parametrize("A,NC", [(36, 4), (4, 4), (5, 4), (6, 4), (7, 4), (9, 4), (13, 4), (18, 4), (3, 4), (5, 2), (7, 3), (9, 8)])
def test_anchor_select_constructed_ties(A, NC):
    """One pixel per pair i < j of anchors with identical, maximal logits -> index i.  All pairs: both in one unrolled triple, one
    in the unrolled part and one in the tail of a group, and in different groups for every pair of groups.  Plus: identical logits
    on all anchors -> 0; a unique maximum on the last anchor -> A - 1; a unique maximum on every single anchor."""
    pairs = [(i, j) for i in range(A) for j in range(i + 1, A)]
    if NC == 4 and A >= 4:      # the cases the comment promises are present in the pair list (groups of the wave kernel)
        per = (A + 3) >> 2
        grp = lambda a: a // per
        unrolled = lambda a: (a - grp(a) * per) < 3 * ((min(A, (grp(a) + 1) * per) - grp(a) * per) // 3)
        kinds = set()
        for i, j in pairs:
            if grp(i) != grp(j):
                kinds.add((grp(i), grp(j)))
            elif unrolled(i) and unrolled(j) and (i - grp(i) * per) // 3 == (j - grp(j) * per) // 3:
                kinds.add("triple")
            elif unrolled(i) != unrolled(j):
                kinds.add("tail")
        ngroups = (A + per - 1) // per
        assert all((g, h) in kinds for g in range(ngroups) for h in range(g + 1, ngroups))
        if A in (13, 18, 36):
            assert "triple" in kinds
        if A in (13, 18):
            assert "tail" in kinds
    low, high = _tie_logits(NC, NC - 1)
    expect = [i for i, _ in pairs] + [0, A - 1] + list(range(A))
    HW, B = len(expect), 2
    l = np.empty((B, NC, A, HW), np.float32)
    l[:] = low[None, :, None, None]
    for p, (i, j) in enumerate(pairs):
        l[:, :, i, p] = high[None]
        l[:, :, j, p] = high[None]
    p0 = len(pairs)
    l[:, :, :, p0] = high[None, :, None]                  # every anchor identical
    l[:, :, A - 1, p0 + 1] = high[None]                   # unique maximum on the last anchor
    for a in range(A):
        l[:, :, a, p0 + 2 + a] = high[None]
    l[1] = l[1, :, :, ::-1].copy()                               # image 1: the same pixels in reverse order (other lanes, other blocks)
    want = np.stack([np.array(expect), np.array(expect)[::-1]]).astype(np.int32)
    runs = [_select(l, fg=True), _select(l, fg=False)] + ([_select(l, keys=True)] if NC == 4 and A >= 4 else [])
    fg = runs[0][2]
    hi_fg = fg[0, expect[0], 0]
    for idx, prob, _ in runs:
        assert np.array_equal(idx, want), (A, NC, np.nonzero(idx != want))
        assert (_bits(prob) == _bits(np.float32(hi_fg))).all()
    assert np.array_equal(np.argmax(fg, axis=1), want)
    assert abs(float(hi_fg) - (1.0 - 1.0 / (np.e + NC - 1))) <= 1e-6


@pytest.mark.parametrize("A,NC", [(36, 4), (5, 4), (3, 4), (5, 2), (7, 3), (9, 8)])
def test_anchor_select_known_values(A, NC):
    """All logits equal -> fg = 1 - 1/NC exactly (0.75 for 4 classes, 0.5 for 2); background 200 below the others -> exactly 1.0;
    background 200 above -> exactly 0.0 and index 0."""
    B, HW = 2, 65
    rng = np.random.default_rng(A * 10 + NC)
    level = rng.standard_normal((B, 1, A, HW)).astype(np.float32) * 5
    l = np.repeat(level, NC, axis=1)
    equal = {2: 0.5, 4: 0.75, 8: 0.875}.get(NC, float(np.float32(1) - np.float32(1) / np.float32(NC)))
    for fg_on in (True, False):
        idx, prob, fg = _select(l, fg=fg_on)
        assert (prob == np.float32(equal)).all() and (idx == 0).all()
        assert fg is None or (fg == np.float32(equal)).all()
    below, above = l.copy(), l.copy()
    below[:, 0] -= 200.0
    above[:, 0] += 200.0
    for fg_on in (True, False):
        idx, prob, fg = _select(below, fg=fg_on)
        assert (prob == 1.0).all() and (idx == 0).all() and (fg is None or (fg == 1.0).all())
        idx, prob, fg = _select(above, fg=fg_on)
        assert (_bits(prob) == 0).all() and (idx == 0).all() and (fg is None or (_bits(fg) == 0).all())
    # one saturated anchor among unsaturated ones: found wherever it is
    for a in (0, A // 2, A - 1):
        one = l.copy()
        one[:, 0, a] -= 200.0
        idx, prob, _ = _select(one, fg=False)
        assert (idx == a).all() and (prob == 1.0).all()


@pytest.mark.parametrize("A,NC", [(36, 4), (13, 4), (5, 3)])
def test_anchor_select_non_finite_logits_stay_in_range(A, NC):
    """NaN, +inf and -inf logits at a handful of pixels: sel_idx stays inside [0, A) everywhere (it indexes the offset table next)
    and every other pixel is bit-equal to the run on the clean input."""
    B, HW = 2, 257
    l = _logits(B, A, NC, HW, 3.0, 77 + A)
    dirty = l.copy()
    rng = np.random.default_rng(5)
    pix = rng.choice(HW, 12, replace=False)
    for n, p in enumerate(pix):
        v = (np.nan, np.inf, -np.inf)[n % 3]
        if n < 9:
            dirty[n % B, rng.integers(NC), rng.integers(A), p] = v
        elif n < 11:
            dirty[n % B, :, rng.integers(A), p] = v              # every class of one anchor
        else:
            dirty[:, :, :, p] = np.nan                           # a whole pixel
    clean_pix = np.isfinite(dirty).all(axis=(1, 2))              # [B][HW]
    assert (~clean_pix).sum() >= 12
    for kw in ({"fg": True}, {"fg": False}) + (({"keys": True},) if NC == 4 else ()):
        i0, p0, _ = _select(l, **kw)
        i1, p1, _ = _select(dirty, **kw)
        assert ((i1 >= 0) & (i1 < A)).all()
        assert np.array_equal(i1[clean_pix], i0[clean_pix]) and np.array_equal(_bits(p1)[clean_pix], _bits(p0)[clean_pix])


# ======================================================================================== 2. fg top-1
def _fg_top1(prob):
    L = _hip.lib()
    B, A, HW = prob.shape
    d, idx, val = Guarded(prob.size).put(prob), Guarded(B * HW, torch.int32), Guarded(B * HW)
    _hip.check(L.m3d_fg_top1(d.ptr, B, A, HW, idx.ptr, val.ptr, _stream()))
    return idx.get(np.int32).reshape(B, HW), val.get().reshape(B, HW)


@pytest.mark.parametrize("A", [1, 2, 36])
def test_fg_top1_exact(A):
    B = 2
    for hi, HW in enumerate(HW_EDGES + (48 * 160,) * (A == 36)):
        rng = np.random.default_rng(31 * A + hi)
        u = rng.random((B, A, HW)).astype(np.float32)
        maps = {"uniform": u, "all_negative": -1.0 - u, "eighths": np.round(u * 8) / 8, "negative_eighths": -np.round(u * 8) / 8 - 1,
                "constant": np.full_like(u, 0.25)}
        for name, m in maps.items():
            m = m.astype(np.float32)
            idx, val = _fg_top1(m)
            want = np.argmax(m, axis=1)
            assert np.array_equal(idx, want), (A, HW, name)
            assert np.array_equal(_bits(val), _bits(np.take_along_axis(m, want[:, None], 1)[:, 0])), (A, HW, name)
            assert np.array_equal(val, m.max(axis=1))
        if A >= 2:
            # -0.0 beside +0.0 compare equal: the lower index wins whichever zero it holds
            for first, second in ((-0.0, 0.0), (0.0, -0.0)):
                z = (-1.0 - u).astype(np.float32)
                a0 = rng.integers(0, A - 1, size=(B, HW))
                a1 = a0 + 1 + (rng.random(a0.shape) * (A - 1 - a0)).astype(np.int64)
                np.put_along_axis(z, a0[:, None], np.float32(first), 1)
                np.put_along_axis(z, a1[:, None], np.float32(second), 1)
                idx, val = _fg_top1(z)
                assert np.array_equal(idx, a0) and np.array_equal(idx, np.argmax(z, axis=1)) and (val == 0).all()
                assert (np.signbit(val) == np.signbit(np.float32(first))).all()


# ======================================================================================== 3. alignment offsets
def _sel_inputs(B, A, HW, thresh, seed):
    """Random indices in [0, A) and probabilities that include the threshold, its two neighbours, 0, 1 and -1."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, A, size=(B, HW)).astype(np.int32)
    prob = rng.random((B, HW)).astype(np.float32)
    t = np.float32(thresh)
    special = np.array([t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0)), 0.0, 1.0, -1.0], np.float32)
    flat = prob.reshape(-1)
    where = rng.permutation(flat.size)[:max(1, flat.size // 3)]
    flat[where] = special[np.arange(where.size) % 6]
    if where.size >= 6:
        assert all((flat == s).any() for s in special)
    return idx, prob


def _align0(idx, prob, thresh, table, kk, om_cs, shift=0):
    L = _hip.lib()
    B, HW = idx.shape
    A = table.shape[0]
    di, dp, dt = Guarded(idx.size, torch.int32).put(idx), Guarded(prob.size).put(prob), Guarded(table.size).put(table)
    om = Guarded(B * HW * om_cs, shift=shift)
    _hip.check(L.m3d_align_offsets(0, di.ptr, dp.ptr, _f32(thresh), dt.ptr, None, None, None, 0.0, 1.0, 0.0, 1.0, om.ptr, om_cs,
                                   B, A, HW, kk, 0, _stream()))
    return om.get().reshape(B, HW, om_cs)


def _check_align0(idx, prob, thresh, table, kk, om_cs, shift, vector):
    got = _align0(idx, prob, thresh, table, kk, om_cs, shift)
    hard = (prob > np.float32(thresh)).astype(np.float32)                    # strict
    want = table[idx] * hard[..., None]                                      # exact: a product with 0 or 1
    tag = (idx.shape, kk, om_cs, shift)
    assert np.array_equal(got[..., :2 * kk], want), tag
    assert (got[..., :2 * kk][hard == 0] == 0).all(), tag
    assert np.array_equal(_bits(got[..., 2 * kk:3 * kk]), np.repeat(_bits(prob)[..., None], kk, axis=2)), tag
    if vector:
        assert om_cs == 28 and (_bits(got[..., 27]) == 0).all(), tag
    else:
        assert (_bits(got[..., 3 * kk:]) == SENT).all(), tag                 # pad columns untouched
    return got


def _engine_table():
    net, _ = _net_dev()
    eng = net.engine()
    tab = eng.P["shape.table"].cpu().numpy()
    assert tab.shape == (eng.A, 18) and tab.dtype == np.float32
    return tab


def test_align_offsets_mode0_exact():
    """shape_align: columns [0, 2kk) = table[idx] * (prob > thresh), columns [2kk, 3kk) = prob; the 16-byte-store path (kk = 9,
    om_cs = 28, aligned base: pad column written as 0) and the scalar path (pad columns untouched) give the same 27 columns."""
    rng = np.random.default_rng(11)
    tables = [(rng.standard_normal((36, 18)) * 3).astype(np.float32), _engine_table(), (rng.standard_normal((5, 18)) * 3).astype(np.float32)]
    for ti, table in enumerate(tables):
        A = table.shape[0]
        for B in (1, 3):
            for hi, HW in enumerate((1, 255, 256, 257, 7680)):
                if HW == 7680 and (B, ti) not in ((3, 0), (1, 1)):
                    continue                                   # the large shape once per table of the shipped A
                thresh = 0.5 if (hi + B) % 2 else 0.3
                idx, prob = _sel_inputs(B, A, HW, thresh, 100 * ti + 10 * B + hi)
                vec = _check_align0(idx, prob, thresh, table, 9, 28, 0, True)
                for om_cs, shift in ((28, 1), (27, 0), (32, 0), (32, 1)):
                    sc = _check_align0(idx, prob, thresh, table, 9, om_cs, shift, False)
                    assert np.array_equal(_bits(sc[..., :27]), _bits(vec[..., :27]))
    table1 = (rng.standard_normal((36, 2)) * 3).astype(np.float32)
    for B in (1, 3):
        for hi, HW in enumerate((1, 255, 256, 257)):
            idx, prob = _sel_inputs(B, 36, HW, 0.5, 900 + 10 * B + hi)
            for om_cs in (3, 4):
                _check_align0(idx, prob, 0.5, table1, 1, om_cs, 0, False)


def test_align_offsets_mode1_matches_float64():
    """center_align, called as the engine calls it: bbox_x / bbox_y are two planes of one [B][11][A][HW] tensor.  Column 0 is
    off_y, column 1 off_x, column 2 prob (exact); offsets are 0 where prob <= thresh."""
    L = _hip.lib()
    worst = 0.0
    for B in (1, 3):
        for hi, HW in enumerate((1, 255, 256, 257, 7680)):
            for A, (kx, ky), om_cs in ((36, (0, 1), 4), (36, (4, 5), 3), (5, (5, 0), 4)):
                if HW == 7680 and (B, A, kx) != (3, 36, 0):
                    continue
                rng = np.random.default_rng(7000 + 100 * B + 10 * hi + kx)
                idx, prob = _sel_inputs(B, A, HW, 0.5, 300 + 10 * B + hi + kx)
                box = rng.standard_normal((B, 11, A, HW)).astype(np.float32)
                wh = (rng.random((A, 2)) * 20 + 0.5).astype(np.float32)
                wh[:, 1] *= 3.0
                mean_x, std_x, mean_y, std_y = (np.float32(v) for v in (0.37, 1.9, -41.5, 23.0))   # four distinct constants
                di, dp = Guarded(idx.size, torch.int32).put(idx), Guarded(prob.size).put(prob)
                db, dw = Guarded(box.size).put(box), Guarded(wh.size).put(wh)
                om = Guarded(B * HW * om_cs)
                _hip.check(L.m3d_align_offsets(1, di.ptr, dp.ptr, 0.5, None, db.ptr + 4 * kx * A * HW, db.ptr + 4 * ky * A * HW,
                                               dw.ptr, float(mean_x), float(std_x), float(mean_y), float(std_y), om.ptr, om_cs,
                                               B, A, HW, 1, 11 * A * HW, _stream()))
                got = om.get().reshape(B, HW, om_cs)
                hard = prob > np.float32(0.5)
                bx = np.take_along_axis(box[:, kx], idx[:, None], 1)[:, 0].astype(np.float64)
                by = np.take_along_axis(box[:, ky], idx[:, None], 1)[:, 0].astype(np.float64)
                aw, ah = wh[idx, 0].astype(np.float64), wh[idx, 1].astype(np.float64)
                off_x = (bx * float(std_x) + float(mean_x)) * aw * hard
                off_y = (by * float(std_y) + float(mean_y)) * ah * hard
                tol_x = 4 * 2.0 ** -24 * (np.abs(bx * float(std_x)) + abs(float(mean_x))) * np.abs(aw)
                tol_y = 4 * 2.0 ** -24 * (np.abs(by * float(std_y)) + abs(float(mean_y))) * np.abs(ah)
                tag = (B, HW, A, kx, ky, om_cs)
                ey, ex = np.abs(got[..., 0] - off_y), np.abs(got[..., 1] - off_x)
                assert (ey <= tol_y).all() and (ex <= tol_x).all(), tag
                assert (got[..., :2][~hard] == 0).all(), tag
                assert np.array_equal(_bits(got[..., 2]), _bits(prob)), tag
                assert (_bits(got[..., 3:]) == SENT).all(), tag
                if hard.any():
                    worst = max(worst, float((ey[hard] / tol_y[hard]).max()), float((ex[hard] / tol_x[hard]).max()))
    print("align_offsets mode 1: max err / bound = %.3f" % worst)
    _log("rpn_glue.align_mode1", {"max_err_over_bound": worst})


def test_align_offsets_argument_checks_launch_nothing():
    L = _hip.lib()
    B, A, HW = 1, 36, 64
    idx, prob = _sel_inputs(B, A, HW, 0.5, 1)
    di, dp = Guarded(idx.size, torch.int32).put(idx), Guarded(prob.size).put(prob)
    tab, box, wh = Guarded(A * 18).put(np.ones((A, 18), np.float32)), Guarded(B * 11 * A * HW).put(np.ones(B * 11 * A * HW, np.float32)), \
        Guarded(A * 2).put(np.ones((A, 2), np.float32))
    om = Guarded(B * HW * 32)
    bad = [
        (0, tab.ptr, None, None, None, 26, 9),               # om_cs < 3 * kk
        (0, tab.ptr, None, None, None, 2, 1),
        (1, None, box.ptr, box.ptr, wh.ptr, 2, 1),
        (1, None, box.ptr, box.ptr, wh.ptr, 28, 9),          # mode 1 with kk != 1
        (0, None, None, None, None, 28, 9),                  # mode 0 without a table
        (0, None, box.ptr, box.ptr, wh.ptr, 4, 1),
    ]
    for mode, t, bx, by, w, om_cs, kk in bad:
        rc = L.m3d_align_offsets(mode, di.ptr, dp.ptr, 0.5, t, bx, by, w, 0.0, 1.0, 0.0, 1.0, om.ptr, om_cs, B, A, HW, kk,
                                 11 * A * HW, _stream())
        assert rc != 0 and b"align_offsets" in L.m3d_last_error(), (mode, om_cs, kk)
    assert om.untouched()


# ======================================================================================== 4. row softmax
def _softmax_rows(x, valid, shift=0):
    L = _hip.lib()
    rows, cs = x.shape
    d = Guarded(x.size, shift=shift).put(x)
    _hip.check(L.m3d_softmax_rows(d.ptr, rows, valid, cs, _stream()))
    return d.get().reshape(rows, cs)


# cs, valid, shift (4-byte elements): reg<1> (cs <= 256), reg<2> (cs <= 512), three-pass (cs % 4 != 0, cs > 512, unaligned base)
SOFTMAX_CASES = [(352, 337, 0), (384, 337, 0), (128, 110, 0), (256, 256, 0), (260, 260, 0), (260, 257, 0), (512, 500, 0), (516, 516, 0),
                 (516, 513, 0), (130, 130, 0), (130, 127, 0), (1000, 999, 0), (128, 110, 1), (128, 128, 1), (4, 3, 0), (64, 1, 0)]


@pytest.mark.parametrize("cs,valid,shift", SOFTMAX_CASES)
def test_softmax_rows_matches_float64(cs, valid, shift):
    worst = 0.0
    big = (cs, valid, shift) in ((352, 337, 0), (128, 110, 0), (130, 127, 0), (128, 110, 1))   # one large run per kernel (+ the shifted base)
    for ri, rows in enumerate((1, 3, 4, 5) + ((7681,) if big else ())):
        g = torch.Generator().manual_seed(cs * 7 + valid + ri)
        x = (torch.randn(rows, cs, generator=g) * (1.0, 3.0, 10.0)[ri % 3]).numpy()
        got = _softmax_rows(x, valid, shift)
        ref = torch.softmax(torch.from_numpy(x[:, :valid]).double(), -1).numpy()
        err = float(np.abs(got[:, :valid].astype(np.float64) - ref).max())
        worst = max(worst, err)
        assert err <= 1e-6, (rows, cs, valid, shift, err)
        assert (_bits(got[:, valid:]) == 0).all(), (rows, cs, valid, shift)
    print("softmax_rows cs %d valid %d shift %d: max|err| = %.3e" % (cs, valid, shift, worst))
    _log("rpn_glue.softmax_rows", {"cs": cs, "valid": valid, "shift": shift, "err": worst})


@pytest.mark.parametrize("cs,valid,shift", [(128, 110, 0), (384, 337, 0), (130, 127, 0), (1000, 999, 0), (128, 110, 1)])
def test_softmax_rows_known_values(cs, valid, shift):
    rows = 5
    rng = np.random.default_rng(cs + valid)
    # valid = 1 -> exactly 1.0 (whatever the logit)
    x = (rng.standard_normal((rows, cs)) * 50).astype(np.float32)
    got = _softmax_rows(x, 1, shift)
    assert (got[:, 0] == 1.0).all() and (_bits(got[:, 1:]) == 0).all()
    # a constant row -> 1 / valid
    x = np.repeat((rng.standard_normal((rows, 1)) * 50).astype(np.float32), cs, axis=1)
    got = _softmax_rows(x, valid, shift)
    assert (got[:, :valid] == np.float32(1) / np.float32(valid)).all() and (_bits(got[:, valid:]) == 0).all()
    # one -inf entry -> exactly 0 there, the rest still the softmax of the others
    x = (rng.standard_normal((rows, cs)) * 3).astype(np.float32)
    hole = rng.integers(0, valid, size=rows)
    x[np.arange(rows), hole] = -np.inf
    got = _softmax_rows(x, valid, shift)
    assert (_bits(got[np.arange(rows), hole]) == 0).all()
    ref = torch.softmax(torch.from_numpy(x[:, :valid]).double(), -1).numpy()
    assert np.abs(got[:, :valid] - ref).max() <= 1e-6 and (_bits(got[:, valid:]) == 0).all()
    # logits of spread 1e4: finite, sum to 1
    x = (rng.standard_normal((rows, cs)) * 1e4).astype(np.float32)
    got = _softmax_rows(x, valid, shift)
    assert np.isfinite(got).all() and (got >= 0).all()
    assert np.abs(got[:, :valid].astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-5
    ref = torch.softmax(torch.from_numpy(x[:, :valid]).double(), -1).numpy()
    assert np.abs(got[:, :valid] - ref).max() <= 1e-6 and (_bits(got[:, valid:]) == 0).all()


# ======================================================================================== 5. bundling and sort keys
@pytest.mark.parametrize("A,HW", [(36, 4), (36, 60), (36, 48 * 160), (36, 61), (5, 4), (5, 60), (5, 257), (5, 7680)])
def test_bundle_outputs_and_score_keys(A, HW):
    B = 2
    rng = np.random.default_rng(A * 1000 + HW)
    std = (1.0, 3.0, 10.0)[HW % 3]
    l = (rng.standard_normal((B, 4, A, HW)) * std).astype(np.float32)
    box = rng.standard_normal((B, 11, A, HW)).astype(np.float32)
    cls, prob, b2, b3, keys = _bundle(l, box)
    R = A * HW
    flat = lambda t: t.reshape(B, t.shape[1], R).transpose(0, 2, 1)          # row = a * HW + p
    assert np.array_equal(_bits(cls), _bits(flat(l)))
    assert np.array_equal(_bits(b2), _bits(flat(box[:, :4])))
    assert np.array_equal(_bits(b3), _bits(flat(box[:, 4:])))
    err = float(np.abs(prob.astype(np.float64) - _softmax64(flat(l), 2)).max())
    print("bundle_outputs A %d HW %d std %g: max|prob - f64| = %.3e" % (A, HW, std, err))
    _log("rpn_glue.bundle_prob", {"A": A, "HW": HW, "err": err})
    assert err <= 1e-6
    assert np.array_equal(keys, _sortable(prob[..., 1:].max(axis=2)))
    _check_keys((A, HW), keys.reshape(B, A, HW), l)
    if HW % 4 == 0:
        assert np.array_equal(_keys_planar(l).reshape(B, R), keys)
    # score_bits is optional
    L = _hip.lib()
    d, bx = Guarded(l.size).put(l), Guarded(box.size).put(box)
    o = [Guarded(B * R * 4), Guarded(B * R * 4), Guarded(B * R * 4), Guarded(B * R * 7)]
    _hip.check(L.m3d_bundle_outputs(d.ptr, bx.ptr, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, None, B, A, HW, _stream()))
    for buf, want in zip(o, (cls, prob, b2, b3)):
        assert np.array_equal(_bits(buf.get()), _bits(want).reshape(-1))


def test_score_keys_planar_argument_checks():
    L = _hip.lib()
    l = _logits(1, 5, 4, 8, 1.0, 3)
    d, k = Guarded(l.size).put(l), Guarded(5 * 8, torch.int32)
    assert L.m3d_score_keys_planar(d.ptr, k.ptr, 1, 5, 6, _stream()) != 0 and b"score_keys_planar" in L.m3d_last_error()
    assert L.m3d_score_keys_planar(d.ptr + 4, k.ptr, 1, 5, 4, _stream()) != 0
    assert L.m3d_score_keys_planar(d.ptr, k.ptr + 4, 1, 5, 4, _stream()) != 0
    assert k.untouched()


# ======================================================================================== 6. max-pool, layouts, weight packing
def _maxpool(x, C, c_in0, out_cs, c_out0):
    """x: NHWC [N][H][W][in_cs] (numpy or torch); pools channels [c_in0, c_in0 + C) into channels [c_out0, c_out0 + C) of an
    [N][H/2][W/2][out_cs] buffer.  Returns the whole output buffer as int32 bits."""
    L = _hip.lib()
    x = torch.as_tensor(x)
    N, H, W, in_cs = x.shape
    d = Guarded(x.numel())
    d.t.copy_(x.reshape(-1))
    out = Guarded(N * (H // 2) * (W // 2) * out_cs)
    _hip.check(L.m3d_maxpool2x2(d.ptr + 4 * c_in0, in_cs, out.ptr + 4 * c_out0, out_cs, N, H, W, C, _stream()))
    return out.get(np.int32).reshape(N, H // 2, W // 2, out_cs)


@pytest.mark.parametrize("C,in_cs,c_in0,out_cs,c_out0", [(4, 4, 0, 4, 0), (16, 16, 0, 16, 0), (64, 64, 0, 64, 0), (16, 32, 8, 16, 0), (16, 16, 0, 24, 4),
                                                         (4, 12, 4, 20, 12), (64, 72, 8, 80, 0)])
def test_maxpool2x2_exact(C, in_cs, c_in0, out_cs, c_out0):
    for si, (N, H, W) in enumerate(((2, 8, 12), (1, 7, 12), (2, 8, 13), (3, 9, 11), (1, 2, 2), (1, 3, 3), (2, 40, 72))):
        g = torch.Generator().manual_seed(C * 100 + in_cs + si)
        for negative in (False, True):
            x = torch.randn(N, H, W, in_cs, generator=g)
            if negative:
                x = -x.abs() - 0.5
            got = _maxpool(x, C, c_in0, out_cs, c_out0)
            ref = F.max_pool2d(x[..., c_in0:c_in0 + C].permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous().numpy()
            tag = (N, H, W, negative)
            assert np.array_equal(got[..., c_out0:c_out0 + C], _bits(ref)), tag
            assert (got[..., :c_out0] == SENT).all() and (got[..., c_out0 + C:] == SENT).all(), tag


def test_maxpool2x2_batch8_level_shape_beyond_grid_cap():
    """N = 8, 384 x 1280, C = 16: 3.9 M work items against a grid cap of 8192 workgroups x 256 threads (the grid-stride loop)."""
    L = _hip.lib()
    N, H, W, C = 8, 384, 1280, 16
    assert N * (H // 2) * (W // 2) * (C // 4) > 8192 * 256
    g = torch.Generator().manual_seed(2)
    x = torch.randn(N, H, W, C, generator=g)
    d = Guarded(x.numel())
    d.t.copy_(x.reshape(-1))
    out = Guarded(N * (H // 2) * (W // 2) * C)
    _hip.check(L.m3d_maxpool2x2(d.ptr, C, out.ptr, C, N, H, W, C, _stream()))
    got = out.get(np.int32).reshape(N, H // 2, W // 2, C)
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous().numpy()
    assert np.array_equal(got, _bits(ref))


def test_maxpool2x2_argument_checks():
    L = _hip.lib()
    d, out = Guarded(2 * 4 * 4 * 8), Guarded(2 * 2 * 2 * 8)
    for C, in_cs, out_cs in ((6, 8, 8), (4, 6, 8), (4, 8, 6)):
        assert L.m3d_maxpool2x2(d.ptr, in_cs, out.ptr, out_cs, 2, 4, 4, C, _stream()) != 0 and b"maxpool" in L.m3d_last_error()
    assert out.untouched()


@pytest.mark.parametrize("C", [1, 3, 27, 32, 33, 168])
def test_layout_changes_exact(C):
    """m3d_nchw_to_nhwc / m3d_nhwc_to_nchw against permute, tile edges of the 32 x 32 LDS transpose on both axes, channel
    strides wider than C (pads untouched), and the round trip."""
    L = _hip.lib()
    N = 3
    for hi, (H, W) in enumerate(((1, 1), (1, 31), (4, 8), (3, 11), (48, 160))):
        HW = H * W
        rng = np.random.default_rng(C * 10 + hi)
        x = rng.standard_normal((N, C, H, W)).astype(np.float32)
        for cs in (C, C + 5):
            d, o = Guarded(x.size).put(x), Guarded(N * HW * cs)
            _hip.check(L.m3d_nchw_to_nhwc(d.ptr, o.ptr, N, C, H, W, cs, _stream()))
            nhwc = o.get(np.int32).reshape(N, HW, cs)
            assert np.array_equal(nhwc[..., :C], _bits(x.reshape(N, C, HW).transpose(0, 2, 1))), (C, HW, cs)
            assert (nhwc[..., C:] == SENT).all(), (C, HW, cs)
            # back, from the strided buffer the first call wrote (pads hold the sentinel: read, never used)
            back = Guarded(x.size)
            _hip.check(L.m3d_nhwc_to_nchw(o.ptr, cs, back.ptr, N, C, H, W, _stream()))
            assert np.array_equal(back.get(np.int32), _bits(x).reshape(-1)), (C, HW, cs)
            # nhwc_to_nchw on an input of its own
            y = rng.standard_normal((N, HW, cs)).astype(np.float32)
            dy, oy = Guarded(y.size).put(y), Guarded(N * C * HW)
            _hip.check(L.m3d_nhwc_to_nchw(dy.ptr, cs, oy.ptr, N, C, H, W, _stream()))
            assert np.array_equal(oy.get(np.int32).reshape(N, C, HW), _bits(y[..., :C].transpose(0, 2, 1))), (C, HW, cs)
    assert L.m3d_nchw_to_nhwc(d.ptr, o.ptr, N, C, 1, 1, C - 1, _stream()) != 0 and b"nchw_to_nhwc" in L.m3d_last_error()
    assert L.m3d_nhwc_to_nchw(d.ptr, C - 1, o.ptr, N, C, 1, 1, _stream()) != 0 and b"nhwc_to_nchw" in L.m3d_last_error()


@pytest.mark.parametrize("Cout,Cout_pad,Cin,Cin_pad,k", [(27, 32, 3, 4, 1), (27, 32, 3, 4, 3), (16, 16, 3, 4, 7), (27, 32, 128, 128, 3), (32, 32, 16, 16, 3),
                                                         (5, 5, 7, 7, 1), (1, 64, 1, 8, 3), (512, 512, 512, 512, 3)])
def test_pack_conv_weight_exact(Cout, Cout_pad, Cin, Cin_pad, k):
    """[Cout][Cin][kh][kw] -> [Cout_pad][(i * kw + j) * Cin_pad + c], zero rows >= Cout and channels >= Cin; 512 x 512 x 3 x 3 has
    more elements than the grid cap of 4096 workgroups x 256 threads covers in one pass."""
    L = _hip.lib()
    for kh, kw in ((k, k),) + (((1, 3), (3, 1)) if k == 3 and Cout <= 32 else ()):
        if Cout == 512:
            assert Cout_pad * kh * kw * Cin_pad > 4096 * 256
        rng = np.random.default_rng(Cout + Cin + kh)
        w = rng.standard_normal((Cout, Cin, kh, kw)).astype(np.float32)
        d, p = Guarded(w.size).put(w), Guarded(Cout_pad * kh * kw * Cin_pad)
        _hip.check(L.m3d_pack_conv_weight(d.ptr, p.ptr, Cout, Cout_pad, Cin, Cin_pad, kh, kw, _stream()))
        want = np.zeros((Cout_pad, kh * kw, Cin_pad), np.float32)
        want[:Cout, :, :Cin] = w.reshape(Cout, Cin, kh * kw).transpose(0, 2, 1)
        assert np.array_equal(p.get(np.int32), _bits(want).reshape(-1)), (kh, kw)
    assert L.m3d_pack_conv_weight(d.ptr, p.ptr, Cout, Cout - 1, Cin, Cin_pad, 1, 1, _stream()) != 0
    assert b"pack_conv_weight" in L.m3d_last_error()
    assert L.m3d_pack_conv_weight(d.ptr, p.ptr, Cout, Cout_pad, Cin, Cin - 1, 1, 1, _stream()) != 0
