"""The refinement kernel (m3d_refine_3d_ex through host.refine.refine_detections / refine_rows / RefineMeta) on the seeded cases of
tests/refine_cases.py: against oracle/refine.py at 1e-9 (columns 2..14; valid flag, class and pad column exactly), against the
host twin m3d_refine_3d_host at the same tolerance with identical valid flags, run-to-run bit identity, and a sentinel-filled
output buffer so that an unwritten row shows.  B = 3 with a different p2 / scale / clip per image, K in {1, 40, 64, 65, 130}.

Every kept row fed to the device holds finite values only: that the angle wrap terminates on inf / NaN / 1e30 is established on the
host (tests/test_refine_host.py, same row function) and by reading csrc/refine.hip, never by a GPU run.

Measured on the MI355X: max |kernel - oracle| = max |kernel - host twin| = 7.1e-15 (case k65_step0; <= 1.8e-15 elsewhere)."""
import numpy as np
import pytest
import torch

from gpu_common import _dev, _log, _stream
from m3dssd_amd import _hip
from m3dssd_amd.host import refine as HR

import refine_cases as RC
from test_refine_host import run_host

pytestmark = pytest.mark.gpu


def _kept_rows_are_finite(name):
    inp, exp = RC.inputs(name), RC.expected(name)
    assert np.isfinite(inp.dets[exp.kept]).all(), name
    assert np.isfinite(inp.p2).all() and np.isfinite(inp.p2_inv).all()


def _through_refine_detections(name):
    c, inp = RC.BY_NAME[name], RC.inputs(name)
    dev = _dev()
    return HR.refine_detections(torch.from_numpy(np.array(inp.dets)).to(dev), torch.from_numpy(np.array(inp.counts)).to(dev),
                                np.array(inp.p2), score_thresh=RC.SCORE_THRESH, hill_climbing=c.hill_climbing,
                                step_r_init=c.step_r_init, r_lim=c.r_lim, scale=None if inp.scale is None else np.array(inp.scale),
                                clip_wh=None if inp.clip_wh is None else np.array(inp.clip_wh)).cpu().numpy()


@pytest.mark.parametrize("name", RC.NAMES)
def test_kernel_matches_oracle_and_host_twin(name):
    _kept_rows_are_finite(name)
    exp = RC.expected(name)
    got = _through_refine_detections(name)
    err = RC.compare(got, exp, name + " vs oracle")
    twin = run_host(name)
    assert np.array_equal(got[:, :, 0], twin[:, :, 0])                       # identical valid flags
    assert np.array_equal(got[:, :, [1, 15]], twin[:, :, [1, 15]])
    err_twin = float(np.abs(got[:, :, 2:15] - twin[:, :, 2:15]).max())
    _log("refine_kernel", {"case": name, "rows": int(got.shape[0] * got.shape[1]), "kept": int(exp.kept.sum()),
                           "invalid_initial": exp.n_invalid, "max_err_vs_oracle": err, "max_err_vs_host_twin": err_twin,
                           "oracle_margin": exp.margin, "oracle_min_rz": exp.min_rz})
    print("%s: max |kernel - oracle| = %.3e, max |kernel - host twin| = %.3e" % (name, err, err_twin))
    assert err_twin < RC.TOL
    again = _through_refine_detections(name)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))        # two launches: bit-identical


@pytest.mark.parametrize("name", RC.NAMES)
def test_refine_meta_upload_and_refine_rows(name):
    """The path of the captured-graph detector: RefineMeta.upload (p2, its inverse, scale, clip per image) + refine_rows."""
    _kept_rows_are_finite(name)
    c, inp, exp = RC.BY_NAME[name], RC.inputs(name), RC.expected(name)
    dev = _dev()
    meta = HR.RefineMeta(RC.B, dev)
    meta.upload({"p2": np.array(inp.p2), "scale": None if inp.scale is None else np.array(inp.scale),
                 "clip_wh": None if inp.clip_wh is None else np.array(inp.clip_wh)})
    got = HR.refine_rows(torch.from_numpy(np.array(inp.dets)).to(dev), torch.from_numpy(np.array(inp.counts)).to(dev), meta.p2,
                         meta.p2_inv, meta.scale, meta.clip, RC.SCORE_THRESH, c.hill_climbing, c.step_r_init, c.r_lim).cpu().numpy()
    RC.compare(got, exp, name + " via RefineMeta")
    if inp.scale is not None and inp.clip_wh is not None:                    # the buffers hold exactly what was uploaded
        assert np.array_equal(meta.p2.cpu().numpy().reshape(RC.B, 4, 4), inp.p2)
        assert np.array_equal(meta.p2_inv.cpu().numpy().reshape(RC.B, 4, 4), inp.p2_inv)
        assert np.array_equal(meta.scale.cpu().numpy(), inp.scale) and np.array_equal(meta.clip.cpu().numpy(), inp.clip_wh)
        assert np.array_equal(got.view(np.uint64), _through_refine_detections(name).view(np.uint64))


@pytest.mark.parametrize("name", ["k1", "k65_scale_clip", "k130"])
def test_every_row_is_written(name):
    """m3d_refine_3d_ex straight into a buffer that holds a sentinel: rows past the count, below the threshold and with a NaN
    score come back as sixteen exact zeros, nothing keeps the sentinel."""
    _kept_rows_are_finite(name)
    c, inp, exp = RC.BY_NAME[name], RC.inputs(name), RC.expected(name)
    dev = _dev()
    t = [torch.from_numpy(np.array(a)).to(dev) for a in (inp.dets, inp.counts, inp.p2, inp.p2_inv)]
    sc = None if inp.scale is None else torch.from_numpy(np.array(inp.scale)).to(dev)
    cl = None if inp.clip_wh is None else torch.from_numpy(np.array(inp.clip_wh)).to(dev)
    out = torch.full((RC.B, c.K, 16), RC.SENTINEL, device=dev, dtype=torch.float64)
    _hip.check(_hip.lib().m3d_refine_3d_ex(t[0].data_ptr(), t[1].data_ptr(), RC.B, c.K, t[2].data_ptr(), t[3].data_ptr(),
                                           None if sc is None else sc.data_ptr(), None if cl is None else cl.data_ptr(),
                                           RC.SCORE_THRESH, 1 if c.hill_climbing else 0, float(c.step_r_init), float(c.r_lim),
                                           out.data_ptr(), _stream()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not (got == RC.SENTINEL).any()
    RC.compare(got, exp, name + " into a sentinel buffer")
