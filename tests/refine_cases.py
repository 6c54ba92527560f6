"""Seeded cases of the post-NMS 3-D refinement, shared by tests/test_refine_host.py (the host twin m3d_refine_3d_host) and
tests/test_gpu_refine.py (the kernel).  Nothing here touches the product: inputs are numpy, expected values come from
oracle/refine.py -- ``refine_row`` for the default arguments, ``hill_climb`` directly when hill_climbing / step_r_init / r_lim are
not the defaults -- applied to the row AFTER the test-time scale and clip were applied to it in numpy float32, which is what the
reference does before its per-box loop:

    aboxes[:, 0:4] /= s; aboxes[:, 6:8] /= s                      (reference lib/rpn_util.py:1506-1507)
    np.clip(column, 0, imW - 1 / imH - 1) on x1, y1, x2, y2       (reference lib/rpn_util.py:1557-1561)

Every case has B = 3 images with a DIFFERENT p2 each (focal length, principal point and p2[0, 3] of the KITTI matrix perturbed;
the inverse is np.linalg.inv of each), counts = (K, 0, a value strictly between) in an order that rotates with the case so that
every image index carries rows somewhere, rows past the count filled with 123 / NaN / inf, scores drawn across the 0.75 threshold
with an exact 0.75 (kept), nextafter(0.75, 0) (dropped) and a NaN (dropped) planted, depths from 0.3 to 60 and negative, 2-D boxes
partly outside the image, alpha up to +-100 rad, and rows whose initial projection is invalid (a corner at or behind the camera),
for which the reference skips the hill climb.

A hill climb takes discrete decisions (ol_pos - ol_best > 0, ol_neg - ol_best > 0, ol_pos > ol_neg, rz <= 0, and the angle
wraps a > pi / a < -pi).  ``expected`` measures, from the oracle's own values, the smallest margin of any of them and the smallest
|rz| over every projection of every kept row; tests/test_refine_host.py asserts both stay above 1e-7 (a hundred times the value
tolerance of 1e-9), so no row is excluded anywhere.
"""
import collections
import contextlib
import functools
import math

import numpy as np

from oracle import refine as R

F = np.float32
B = 3
SCORE_THRESH = 0.75
STEP_R_DEFAULT, R_LIM_DEFAULT = 0.3 * math.pi, 0.01
LBLS = ["Car", "Pedestrian", "Cyclist"]
SENTINEL = -7.25                       # what an output buffer holds before the call: an unwritten row shows
TOL = 1e-9                             # |got - want| on columns 2..14 (the project's refinement tolerance)
MARGIN_MIN = 1e-7                      # required of every oracle decision margin and |rz|: 100 x TOL
KITTI_P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884],
                     [0.0, 0.0, 0.0, 1.0]])

Case = collections.namedtuple("Case", "name K seed scale clip hill_climbing step_r_init r_lim")
CASES = [
    Case("k1", 1, 11, False, False, True, STEP_R_DEFAULT, R_LIM_DEFAULT),             # one thread per image
    Case("k40", 40, 12, False, False, True, STEP_R_DEFAULT, R_LIM_DEFAULT),           # B*K = 120: not a multiple of 64
    Case("k40_scale", 40, 13, True, False, True, STEP_R_DEFAULT, R_LIM_DEFAULT),
    Case("k64_clip", 64, 14, False, True, True, STEP_R_DEFAULT, R_LIM_DEFAULT),       # an image fills a 64-thread block exactly
    Case("k65_scale_clip", 65, 15, True, True, True, STEP_R_DEFAULT, R_LIM_DEFAULT),  # one row over: images straddle blocks
    Case("k130", 130, 16, False, False, True, STEP_R_DEFAULT, R_LIM_DEFAULT),         # 390 rows, 7 blocks
    Case("k40_no_climb", 40, 17, False, False, False, STEP_R_DEFAULT, R_LIM_DEFAULT),
    Case("k65_step0", 65, 18, False, False, True, 0.0, R_LIM_DEFAULT),                # no loop iteration runs
    Case("k40_rlim", 40, 19, True, False, True, 0.2 * math.pi, 0.05),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
MIN_INVALID = 10                       # kept rows with an invalid initial projection, per case with K >= 40 (K = 1: one)

Inputs = collections.namedtuple("Inputs", "dets counts p2 p2_inv scale clip_wh")
Expected = collections.namedtuple("Expected", "want kept n_invalid margin min_rz")


def _p2s(rng):
    out = []
    for _ in range(B):
        m = KITTI_P2.copy()
        f = 721.5377 * rng.uniform(0.9, 1.1)
        m[0, 0] = m[1, 1] = f
        m[0, 2] += rng.uniform(-25, 25)
        m[1, 2] += rng.uniform(-15, 15)
        m[0, 3] *= rng.uniform(0.6, 1.4)
        out.append(m)
    p2 = np.stack(out)
    return p2, np.stack([np.linalg.inv(m) for m in p2])


def _row(rng, p2, near):
    """One detection row in ORIGINAL image coordinates.  near: a depth at which a corner of the 3 .. 5 m long box may lie at or
    behind the camera -- always below 0.7 and for a negative depth (no yaw helps: every candidate of a climb is invalid too), for
    some yaws between 0.7 and 2.4 (a climb that wrongly started would find valid candidates and move) -> most of these rows
    start from an invalid projection."""
    w3d, h3d, l3d = rng.uniform(1.4, 2.0), rng.uniform(1.3, 1.9), rng.uniform(3.0, 5.0)
    if near:
        u = rng.random()
        z = rng.uniform(0.3, 0.7) if u < 0.25 else (rng.uniform(0.7, 2.4) if u < 0.75 else -rng.uniform(0.3, 30.0))
    else:
        z = math.exp(rng.uniform(math.log(4.0), math.log(60.0)))
    x = rng.uniform(-1.0, 1.0) * abs(z) * 0.9                       # up to ~650 px off the principal point: boxes leave the image
    y = rng.uniform(0.8, 2.2)
    ry = rng.uniform(-math.pi, math.pi)
    c2 = p2.dot(np.array([x, y, z, 1.0]))
    u, v = c2[0] / c2[2], c2[1] / c2[2]
    if near:
        x1, y1 = rng.uniform(-200, 1100), rng.uniform(-80, 300)
        box = [x1, y1, x1 + rng.uniform(5, 400), y1 + rng.uniform(5, 200)]
    else:
        verts, _ = R.project_3d(p2, x, y, z, w3d, h3d, l3d, ry)
        box = [verts[:, 0].min(), verts[:, 1].min(), verts[:, 0].max(), verts[:, 1].max()]
        box = [b + rng.normal(0, 2.0) for b in box]
    alpha = ry - math.atan2(-z, x) - 0.5 * math.pi + rng.normal(0, 0.4)
    alpha = math.remainder(alpha, 2 * math.pi)
    if rng.random() < 0.3:                                          # whole turns on top: up to +-100 rad, <= 16 wrap iterations
        alpha += 2 * math.pi * rng.integers(-15, 16)
        alpha = max(-100.0, min(100.0, alpha))
    return box + [rng.uniform(0.68, 1.0), float(rng.integers(1, 4)), u, v, z, w3d, h3d, l3d, alpha, float(rng.integers(0, 36))]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> Inputs(dets [3, K, 14] float32, counts [3] int32, p2 / p2_inv [3, 4, 4] float64, scale [3] float32 or None,
    clip_wh [3, 2] float32 or None).  Shared between tests: treat as read-only."""
    c = BY_NAME[name]
    rng = np.random.default_rng(c.seed)
    K = c.K
    p2, p2_inv = _p2s(rng)
    mid = K // 2 - 3 if K > 2 else 1                                # strictly between 0 and K (K = 1 has no such value: 1)
    rot = c.seed % 3
    counts = np.roll(np.array([K, 0, mid], dtype=np.int32), rot)
    scale = np.roll(np.array([0.8, 1.25, 2.0 / 3.0], dtype=F), rot) if c.scale else None
    clip = None
    if c.clip:
        # (imW, imH): the full image is a small one, where whole boxes lie outside and clip to zero width; the image with `mid`
        # rows has cw <= 0 (x is not clipped, y is); the empty image is not clipped at all
        order = [int(i) for i in np.argsort(-counts)]
        clip = np.zeros((B, 2), dtype=F)
        clip[order[0]] = (600.0, 200.0)
        clip[order[1]] = (0.0, 375.0)
        clip[order[2]] = (0.0, -1.0)
    dets = np.zeros((B, K, 14), dtype=F)
    for b in range(B):
        n = int(counts[b])
        for k in range(n):
            near = (k % 3 == 1) or K == 1 and b == int(np.argmax(counts))
            dets[b, k] = np.array(_row(rng, p2[b], near), dtype=F)
        if n >= 8:                                                  # the score boundary, on far and on near rows
            dets[b, 0, 4] = F(0.75)
            dets[b, 1, 4] = F(0.75)
            dets[b, 2, 4] = np.nextafter(F(0.75), F(0))
            dets[b, 3, 4] = np.nan
            dets[b, 4, 4] = F(0.76)
            dets[b, 7, 4] = np.nextafter(F(0.75), F(0))
        elif K == 1 and n:
            dets[b, 0, 4] = F(0.75) if b == int(np.argmax(counts)) else F(0.9)
        if scale is not None:                                       # the detector's rows live in the scaled image
            dets[b, :n, 0:4] *= scale[b]
            dets[b, :n, 6:8] *= scale[b]
        for k in range(n, K):                                       # past the count: garbage that must not be read as a row
            dets[b, k] = (F(123.0), F(np.nan), F(np.inf))[k % 3]
    for a in (dets, counts, p2, p2_inv, scale, clip):
        if a is not None:
            a.setflags(write=False)
    return Inputs(dets, counts, p2, p2_inv, scale, clip)


def prepared_rows(inp):
    """The rows as the reference's per-box loop sees them: divided back to the original image scale, then clipped, in float32."""
    rows = np.array(inp.dets, dtype=F)
    for b in range(B):
        if inp.scale is not None:
            rows[b, :, 0:4] /= inp.scale[b]
            rows[b, :, 6:8] /= inp.scale[b]
        if inp.clip_wh is not None:
            cw, ch = inp.clip_wh[b]
            with np.errstate(invalid="ignore"):
                if cw > 0:
                    rows[b, :, 0] = np.clip(rows[b, :, 0], F(0), F(cw - F(1)))
                    rows[b, :, 2] = np.clip(rows[b, :, 2], F(0), F(cw - F(1)))
                if ch > 0:
                    rows[b, :, 1] = np.clip(rows[b, :, 1], F(0), F(ch - F(1)))
                    rows[b, :, 3] = np.clip(rows[b, :, 3], F(0), F(ch - F(1)))
    return rows


def kept_mask(inp):
    """[3, K] bool: rows inside the count whose float32 score is >= 0.75 (NaN is not)."""
    k = np.arange(inp.dets.shape[1])[None, :] < inp.counts[:, None]
    with np.errstate(invalid="ignore"):
        return k & (inp.dets[:, :, 4].astype(np.float64) >= SCORE_THRESH)


def _pieces(row, p2_inv):
    b = [F(v) for v in row]
    x3d, y3d, z3d = b[6], b[7], b[8]
    c3 = p2_inv.dot(np.array([float(F(x3d * z3d)), float(F(y3d * z3d)), float(z3d), 1.0]))
    ry3d = R.convert_alpha2rot(float(b[12]), c3[2], c3[0])
    box_2d = np.array([b[0], b[1], F(F(b[2] - b[0]) + F(1)), F(F(b[3] - b[1]) + F(1))], dtype=F)
    return b, ry3d, box_2d


def initial_invalid(row, p2, p2_inv):
    """Whether the reference's first test_projection of this row reports a corner with rz <= 0 (then hill_climb returns at once)."""
    b, ry3d, box_2d = _pieces(row, p2_inv)
    return R.test_projection(p2, p2_inv, box_2d, b[6], b[7], b[8], b[9], b[10], b[11], ry3d)[2]


def oracle_row(row, p2, p2_inv, hill_climbing, step_r_init, r_lim):
    """The 13 values of the result line for one prepared row."""
    if not hill_climbing or (step_r_init == STEP_R_DEFAULT and r_lim == R_LIM_DEFAULT):
        return R.refine_row(row, p2, p2_inv, hill_climbing)
    # refine_row with the step / limit passed on to hill_climb (rpn_util.py:1813-1849 around the call at :1833)
    b, ry3d, box_2d = _pieces(row, p2_inv)
    z3d, ry3d, _ = R.hill_climb(p2, p2_inv, box_2d, b[6], b[7], b[8], b[9], b[10], b[11], ry3d, step_r_init=step_r_init, r_lim=r_lim)
    assert isinstance(z3d, np.float32)                              # the depth step is 0: z3d is still the row's float32
    c3 = p2_inv.dot(np.array([float(F(b[6] * z3d)), float(F(b[7] * z3d)), float(z3d), 1.0]))
    alpha = R.convert_rot2alpha(ry3d, c3[2], c3[0])
    return [alpha] + [float(b[i]) for i in (0, 1, 2, 3, 10, 9, 11)] + [c3[0], c3[1] + float(b[10]) / 2, c3[2], ry3d, float(b[4])]


@contextlib.contextmanager
def _recording(rec):
    """Wraps the oracle's own functions while one row runs: every overlap score with its invalid flag, every corner depth, and
    every wrapped angle are noted in rec."""
    o_tp, o_p3, o_wr = R.test_projection, R.project_3d, R._wrap

    def tp(*a, **k):
        r = o_tp(*a, **k)
        rec["ol"].append((r[0], r[2]))
        return r

    def p3(*a, **k):
        r = o_p3(*a, **k)
        rec["rz"] = min(rec["rz"], float(np.abs(r[1][2]).min()))
        return r

    def wr(a):
        r = o_wr(a)
        rec["wrap"] = min(rec["wrap"], math.pi - abs(r))
        return r

    R.test_projection, R.project_3d, R._wrap = tp, p3, wr
    try:
        yield
    finally:
        R.test_projection, R.project_3d, R._wrap = o_tp, o_p3, o_wr


def _decision_margin(ols):
    """ols = [(ol, invalid)] in call order: the first test_projection, then (neg, pos) per loop iteration.  Replays hill_climb's
    yaw branch on the oracle's values and returns the smallest |difference| any of its comparisons rested on."""
    if not ols or ols[0][1]:
        return math.inf
    best, m = ols[0][0], math.inf
    for i in range(1, len(ols) - 1, 2):
        (neg, inv_neg), (pos, inv_pos) = ols[i], ols[i + 1]
        d_pos, d_neg = pos - best, neg - best
        m = min(m, abs(d_pos), abs(d_neg))
        if d_pos > 0:
            m = min(m, abs(pos - neg))
        if d_pos <= 0 and d_neg <= 0:
            continue
        if d_pos > 0 and pos > neg and not inv_pos:
            best = pos
        elif d_neg > 0 and not inv_neg:
            best = neg
    return m


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> Expected(want [3, K, 16] float64 in the layout of m3d_refine_3d's output (zeros for rows that are dropped),
    kept [3, K] bool, n_invalid, margin (smallest decision margin), min_rz (smallest |rz| of any projected corner))."""
    c, inp = BY_NAME[name], inputs(name)
    rows, kept = prepared_rows(inp), kept_mask(inp)
    want = np.zeros((B, c.K, 16))
    n_invalid, margin, min_rz = 0, math.inf, math.inf
    for b in range(B):
        for k in np.nonzero(kept[b])[0]:
            n_invalid += bool(initial_invalid(rows[b, k], inp.p2[b], inp.p2_inv[b]))
            rec = {"ol": [], "rz": math.inf, "wrap": math.inf}
            with _recording(rec):
                v = oracle_row(rows[b, k], inp.p2[b], inp.p2_inv[b], c.hill_climbing, c.step_r_init, c.r_lim)
            margin = min(margin, _decision_margin(rec["ol"]), rec["wrap"])
            min_rz = min(min_rz, rec["rz"])
            want[b, k, 0], want[b, k, 1], want[b, k, 2:15] = 1.0, float(inp.dets[b, k, 5]), v
    want.setflags(write=False)
    return Expected(want, kept, n_invalid, margin, min_rz)


def compare(got, exp, what):
    """got [3, K, 16] against Expected: columns 0, 1, 15 exactly, 2..14 within TOL, dropped rows sixteen exact zeros.
    -> the measured maximum error."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == exp.want.shape, what
    assert np.array_equal(got[:, :, 0] != 0, exp.kept), (what, "valid flags")
    assert np.array_equal(got[:, :, [0, 1, 15]], exp.want[:, :, [0, 1, 15]]), (what, "valid / class / pad columns")
    assert not got[~exp.kept].any() and not np.signbit(got[~exp.kept]).any(), (what, "a dropped row is not sixteen zeros")
    assert np.isfinite(got[exp.kept]).all(), what
    err = np.abs(got[:, :, 2:15] - exp.want[:, :, 2:15])
    bad = np.argwhere(err >= TOL)
    assert bad.size == 0, (what, bad[:5].tolist(), float(err.max()))
    return float(err.max()) if err.size else 0.0
