"""m3d_refine_3d_host -- the host twin of the refinement kernel: the same row function in a plain loop -- against oracle/refine.py
on the seeded cases of tests/refine_cases.py (no GPU).  The twin is what lets the row arithmetic, the per-image p2 / scale / clip
indexing and the bounded angle wrap be checked on any machine; tests/test_gpu_refine.py runs the same cases through the kernel.

Measured on the CPU (x86-64): maximum |twin - oracle| over all cases 8.9e-16 (columns 2..14, tolerance 1e-9); smallest oracle
decision margin 6.4e-5 (case k65_scale_clip), smallest |rz| 5.3e-4 (case k40) -- both must exceed 1e-7."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from m3dssd_amd import _hip
from oracle import refine as R

import refine_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def run_host(name, dets=None):
    """The case through m3d_refine_3d_host into a sentinel-filled buffer -> [3, K, 16] float64."""
    c, inp = RC.BY_NAME[name], RC.inputs(name)
    dets = np.ascontiguousarray(inp.dets if dets is None else dets, dtype=np.float32)
    keep = [dets, np.ascontiguousarray(inp.counts), np.ascontiguousarray(inp.p2), np.ascontiguousarray(inp.p2_inv),
            None if inp.scale is None else np.ascontiguousarray(inp.scale),
            None if inp.clip_wh is None else np.ascontiguousarray(inp.clip_wh)]
    out = np.full((RC.B, c.K, 16), RC.SENTINEL, dtype=np.float64)
    _hip.check(_hip.lib().m3d_refine_3d_host(_p(keep[0]), _p(keep[1]), RC.B, c.K, _p(keep[2]), _p(keep[3]), _p(keep[4]), _p(keep[5]),
                                             RC.SCORE_THRESH, 1 if c.hill_climbing else 0, float(c.step_r_init), float(c.r_lim),
                                             _p(out)))
    return out


@pytest.mark.parametrize("name", RC.NAMES)
def test_cases_are_what_they_claim(name):
    """The generator's promises, from the inputs and the oracle alone: the counts, the planted scores, rows whose initial
    projection is invalid, and oracle decision margins / corner depths well clear of the value tolerance."""
    c, inp, exp = RC.BY_NAME[name], RC.inputs(name), RC.expected(name)
    assert sorted(inp.counts.tolist()) == sorted([0, c.K, c.K // 2 - 3 if c.K > 2 else 1])
    assert len({m.tobytes() for m in inp.p2}) == RC.B
    print("%s: kept %d of %d rows, invalid initial projection %d, min decision margin %.3e, min |rz| %.3e"
          % (name, int(exp.kept.sum()), RC.B * c.K, exp.n_invalid, exp.margin, exp.min_rz))
    assert exp.n_invalid >= (RC.MIN_INVALID if c.K >= 40 else 1)
    assert exp.kept.sum() - exp.n_invalid >= (RC.MIN_INVALID if c.K >= 40 else 1)
    assert exp.margin > RC.MARGIN_MIN and exp.min_rz > RC.MARGIN_MIN
    if c.K >= 40:
        s = inp.dets[:, :, 4]
        inside = np.arange(c.K)[None] < inp.counts[:, None]
        for v, keep in ((np.float32(0.75), True), (np.nextafter(np.float32(0.75), np.float32(0)), False)):
            hit = inside & (s == v)
            assert hit.any() and (exp.kept[hit] == keep).all()
        assert (inside & np.isnan(s)).any() and not exp.kept[np.isnan(s)].any()
        rows = RC.prepared_rows(inp)[exp.kept]
        assert (rows[:, 8] < 0).any() and rows[:, 8].max() > 30 and 0 < np.abs(rows[:, 8]).min() < 1.3
        assert np.abs(rows[:, 12]).max() > 30 and np.abs(rows[:, 12]).max() <= 100
        orig = RC.prepared_rows(inp._replace(clip_wh=None))[exp.kept]                  # original image scale, before the clip
        assert (orig[:, 0] < 0).any() and (orig[:, 2] > 1242).any() and (orig[:, 1] < 0).any()     # partly outside the image
    if c.clip:
        rows = RC.prepared_rows(inp)
        full = int(np.argmax(inp.counts))
        assert (rows[full][exp.kept[full]][:, 2] == rows[full][exp.kept[full]][:, 0]).any()          # clipped to zero width
        assert (rows[full][exp.kept[full]][:, 2] == 599).any() and (rows[full][exp.kept[full]][:, 3] == 199).any()
        other = [b for b in range(RC.B) if 0 < inp.counts[b] < c.K][0]
        unclipped = RC.prepared_rows(inp._replace(clip_wh=None))
        assert inp.clip_wh[other, 0] <= 0 and np.array_equal(rows[other, :, [0, 2]], unclipped[other, :, [0, 2]], equal_nan=True)
        assert not np.array_equal(rows[other, :, [1, 3]], unclipped[other, :, [1, 3]], equal_nan=True)   # ... but y is


@pytest.mark.parametrize("name", RC.NAMES)
def test_host_twin_matches_oracle(name):
    exp = RC.expected(name)
    out = run_host(name)
    err = RC.compare(out, exp, name)
    print("%s: max |twin - oracle| = %.3e" % (name, err))
    assert np.array_equal(run_host(name).view(np.uint64), out.view(np.uint64))      # two calls: bit-identical


def test_kitti_text_of_a_batch_matches_oracle():
    """host.refine.kitti_text on the twin's rows == oracle.refine.kitti_text of the same (scaled and clipped) rows, all three
    class labels present."""
    from m3dssd_amd.host import refine as HR
    name = "k65_scale_clip"
    inp, exp = RC.inputs(name), RC.expected(name)
    out, rows = run_host(name), RC.prepared_rows(inp)
    seen = set()
    for b in range(RC.B):
        n = int(inp.counts[b])
        with np.errstate(invalid="ignore"):
            want = R.kitti_text(rows[b, :n], inp.p2[b], RC.LBLS, nms_topn_post=n)
        assert HR.kitti_text(out[b], RC.LBLS) == want, b
        seen |= {ln.split(" ")[0] for ln in want.splitlines()}
        assert len(want.splitlines()) == int(exp.kept[b].sum())
    assert seen == set(RC.LBLS)


def test_bad_arguments_are_refused():
    L = _hip.lib()
    z = np.zeros(16)
    assert L.m3d_refine_3d_host(None, _p(z), 1, 1, _p(z), _p(z), None, None, 0.75, 1, 0.9, 0.01, _p(z)) == -1
    assert L.m3d_refine_3d_host(_p(z), _p(z), 1, 1, _p(z), _p(z), None, None, 0.75, 1, -0.1, 0.01, _p(z)) == -1


_NONFINITE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import refine_cases as RC
import test_refine_host as T
name = "k40"
inp, exp = RC.inputs(name), RC.expected(name)
b = int(np.argmax(inp.counts))
ks = [int(k) for k in np.nonzero(exp.kept[b])[0] if exp.want[b, k, 12] > 4.0][:3]      # three kept rows that do climb
dets = np.array(inp.dets)
dets[b, ks[0], 12] = np.inf
dets[b, ks[1], 12] = 1e30
dets[b, ks[2], 6:8] = np.nan
np.savez(sys.argv[2], clean=T.run_host(name), dirty=T.run_host(name, dets), b=b, ks=np.array(ks))
"""


def test_non_finite_rows_terminate_and_leave_their_neighbours_alone(tmp_path):
    """alpha = inf, alpha = 1e30 and NaN centre coordinates in rows that pass the score test: the reference's angle wrap would spin
    for ever on the first two (and so did the kernel's); the call must return, flag the rows valid, and leave every other row of
    the batch with the bits it has without them.  In a child process, so that a regression fails here instead of hanging the run.
    (These rows are not fed to oracle.refine: its _wrap is the reference's and does not terminate on them.)"""
    out = str(tmp_path / "nonfinite.npz")
    res = subprocess.run([sys.executable, "-c", _NONFINITE_CHILD, ROOT, out], timeout=30, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    z = np.load(out)
    clean, dirty, b, ks = z["clean"], z["dirty"], int(z["b"]), z["ks"].tolist()
    assert len(ks) == 3
    for k in ks:
        assert clean[b, k, 0] == 1.0 and dirty[b, k, 0] == 1.0 and dirty[b, k, 15] == 0.0
    assert np.isnan(dirty[b, ks[0], 2]) and np.isnan(dirty[b, ks[0], 13])            # inf -> NaN, not a hang
    assert np.isfinite(dirty[b, ks[1], 2:15]).all() and abs(dirty[b, ks[1], 13]) <= np.pi and abs(dirty[b, ks[1], 2]) <= np.pi
    assert np.isnan(dirty[b, ks[2], 10:13]).all()
    rest = np.ones(clean.shape[:2], dtype=bool)
    rest[b, ks] = False
    assert np.array_equal(clean[rest].view(np.uint64), dirty[rest].view(np.uint64))
    assert not (clean == RC.SENTINEL).any() and not (dirty == RC.SENTINEL).any()
