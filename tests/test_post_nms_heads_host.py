"""Host-only checks of the heads that run behind the NMS: the numpy restatement of ``m3d_post_rows`` on hand-made cases, the three
entry points declared as additive and bound with the header's argument counts, their refusals (which return before anything is
launched), and the rule by which a plan declines the split tail, on plans made by hand (no GPU here)."""
import ctypes
import re
import types

import numpy as np
import torch

import post_nms_ref as R
from m3dssd_amd import _hip
from m3dssd_amd.engine import Engine, _Plan

NEW = {"m3d_topk_decode_planar_2d": 17, "m3d_post_rows": 10, "m3d_fill_post_3d": 15}


# ------------------------------------------------------------------------------------ the restatement
def test_post_rows_ref_by_hand():
    HW = 10
    rows_out = np.array([[37, 7, 12, 25, 3], [4, 14, 24, 34, 9]])          # pixels 7 7 2 5 3 | 4 4 4 4 9
    keep = np.array([[1, 0, 3, 99, 99], [0, 1, 2, 3, 4]])
    num = np.array([3, 5])
    assert R.post_rows_ref(rows_out, keep, num, 40, HW).tolist() == [5, 7, 14, 19]
    assert R.post_rows_ref(rows_out, keep, num, 2, HW).tolist() == [7, 14]       # rows 7 and 37 of image 0: one pixel
    assert R.post_rows_ref(rows_out, keep, num, 1, HW).tolist() == [7, 14]
    assert R.post_rows_ref(rows_out, keep, np.array([0, 0]), 40, HW).size == 0
    assert R.post_rows_ref(rows_out, keep, np.array([0, 5]), 4, HW).tolist() == [14]


def test_post_rows_case_holds_what_its_tests_need():
    HW = 128
    rows_out, keep, num = R.post_rows_case()
    assert num.tolist() == [7, 0, 60]
    p0 = rows_out[0, keep[0, :7]] % HW
    assert p0[0] == p0[1] and rows_out[0, keep[0, 0]] != rows_out[0, keep[0, 1]]      # one pixel, two anchors
    assert (np.diff(p0[:4]) < 0).any()                                                  # not ascending
    assert (keep[0, 7:] >= rows_out.shape[1]).all() and (keep[1] >= rows_out.shape[1]).all()
    for post in (1, 5, 40):
        want = R.post_rows_ref(rows_out, keep, num, post, HW)
        assert (np.diff(want) > 0).all()
        assert not ((want >= HW) & (want < 2 * HW)).any()                               # image 1 lists nothing
        if post > 1:                                                                    # (one row per image cannot repeat a pixel)
            assert want.size < min(7, post) + min(60, post)                             # a pixel was held twice


# ------------------------------------------------------------------------------------ C ABI
def test_entry_points_are_declared_additive_and_bound():
    hdr = open(_hip.HEADER).read()
    history = hdr[hdr.index("added under 5"):hdr.index("#define M3D_ABI_VERSION")]
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = _hip.lib()
    assert L.m3d_abi_version() == 5
    for name, nargs in NEW.items():
        assert re.search(r"\b%s\b" % name, history), name
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, body)
        assert m, "%s is not declared in include/m3dssd_hip.h" % name
        assert len(m.group(1).split(",")) == nargs == len(_hip.SIGNATURES[name][1]), name
        assert hasattr(L, name)
    # additive: the existing decode keeps its signature
    assert _hip.SIGNATURES["m3d_topk_decode_planar_2d"] == _hip.SIGNATURES["m3d_topk_decode_planar"]


def test_refusals_return_before_any_launch():
    L = _hip.lib()
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    E_ARG = _hip.CONSTANTS["M3D_E_ARG"]
    # m3d_post_rows: rows_out, keep, num_keep, B, n, post, HW, rows, n_rows, stream
    assert L.m3d_post_rows(None, p, p, 2, 100, 40, 640, p, p, None) == E_ARG and b"post_rows" in L.m3d_last_error()
    assert L.m3d_post_rows(p, p, p, 2, 100, 40, 640, None, p, None) == E_ARG
    assert L.m3d_post_rows(p, p, p, 2, 100, 40, 640, p, None, None) == E_ARG
    assert L.m3d_post_rows(p, p, p, 2, 100, 0, 640, p, p, None) == E_ARG
    assert L.m3d_post_rows(p, p, p, 103, 100, 40, 640, p, p, None) == E_ARG and b"4096" in L.m3d_last_error()   # 4120 entries
    # m3d_topk_decode_planar_2d needs rows_out
    nb = L.m3d_topk_decode_workspace_bytes(2, 4 * 128)
    assert L.m3d_topk_decode_planar_2d(p, p, p, p, p, p, p, None, p, None, p, nb, 2, 4, 128, 100, None) == E_ARG
    assert b"rows_out" in L.m3d_last_error()
    assert L.m3d_topk_decode_planar_2d(p, p, p, p, p, p, p, None, p, p, p, nb - 1, 2, 4, 128, 100, None) == _hip.CONSTANTS["M3D_E_WORKSPACE"]
    # m3d_fill_post_3d: box, rois, anchors, means, stds, rows_out, keep, counts, B, A, HW, n, post, block, stream
    assert L.m3d_fill_post_3d(p, p, p, p, p, p, p, None, 2, 4, 128, 100, 40, p, None) == E_ARG and b"fill_post_3d" in L.m3d_last_error()
    assert L.m3d_fill_post_3d(p, p, p, p, p, p, p, p, 2, 4, 128, 100, 40, None, None) == E_ARG
    assert L.m3d_fill_post_3d(p, p, p, p, p, p, p, p, 2, 4, 128, 0, 40, p, None) == E_ARG


# ------------------------------------------------------------------------------------ the decline rule
def _plan(writers, post_declined=None, deferred=True):
    """A hand-made plan of six ops, `planar_first_op` = 2, anchor_select = op 2, bundle_outputs = op 5.  Ops 3 and 4 have deferred
    forms that read maps a and b; writers = {map name: index of the op that writes it} (a name left out: never recorded)."""
    plan = _Plan()
    maps = {"a": torch.zeros(4), "b": torch.zeros(4)}
    for i in range(6):
        plan.ops.append(("op%d" % i, "kind", 0.0, lambda st: None, None))
        for name, w in writers.items():
            if w == i:
                plan.wrote(maps[name])
        if deferred and i == 3:
            plan.deferred_form((lambda r: "pre3", "early", 1.0, None), (lambda r: "post3", "late", 2.0, None), [maps["a"]])
        if deferred and i == 4:
            plan.deferred_form(None, (lambda r: "post4", None, None, None), [maps["a"], maps["b"]])
    plan.named["planar_first_op"] = 2
    plan.tail = [("need_rows", "select", 0.0, "need", None), ("op3", "kind", 0.0, "tail3", None), ("op4", "kind", 0.0, "tail4", None)]
    plan.tail_start = 3
    plan.post3d_declined = post_declined
    return plan


def _post3d(plan, B=2, post=40):
    eng = types.SimpleNamespace(conf=types.SimpleNamespace(nms_topN_post=post), device=torch.device("cpu"),
                                POST_ROWS_MAX=Engine.POST_ROWS_MAX)
    stage = types.SimpleNamespace(B=B, HW=16)
    Engine._rpn_post3d(eng, plan, stage, plan.tail_start)
    return stage


def test_split_tail_is_built_from_the_registered_forms():
    plan = _plan({"a": 2, "b": 4})
    stage = _post3d(plan)
    assert [op[:4] for op in plan.tail_pre] == [("need_rows", "select", 0.0, "need"), ("early", "kind", 1.0, "pre3")]
    assert [op[:4] for op in plan.post3d] == [("late", "kind", 2.0, "post3"), ("op4", "kind", 0.0, "post4")]
    assert sorted(w for _, w in plan.post3d_reads) == [2, 4]
    assert plan.post_rows is stage.post_rows and "post_rows" not in plan.named and stage.post_rows.numel() == 2 * 16
    assert plan.tail[1][3] == "tail3"                                               # the one-part tail is left as it was


def test_split_tail_declines():
    cases = {"a map is written in front of planar_first_op": _plan({"a": 1, "b": 4}),
             "a map's writer was never recorded": _plan({"a": 2}),
             "a builder ruled it out": _plan({"a": 2, "b": 4}, post_declined="the attention is not the one-launch route"),
             "nothing registered": _plan({"a": 2, "b": 4}, deferred=False)}
    for why, plan in cases.items():
        _post3d(plan)
        assert plan.tail_pre is None and plan.post3d is None and plan.post3d_reads == [], why
    big = _plan({"a": 2, "b": 4})
    _post3d(big, B=103, post=40)                                                   # 4120 entries: past the sort of m3d_post_rows
    assert big.post3d is None
    ok = _plan({"a": 2, "b": 4})
    _post3d(ok, B=64, post=40)
    assert ok.post3d is not None
