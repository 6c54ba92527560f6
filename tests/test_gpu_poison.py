"""GPU tests (-m gpu): no result depends on device memory that nobody wrote.

Every scratch buffer, staging tensor and padded activation of the package comes from torch.empty, and many are wider than what
the kernels write into them.  A fresh process mostly gets zero pages from the allocator, so a kernel that reads such padding (a
16-byte vector, a GEMM over the padded extent against zero weights: 0 * NaN = NaN) passes every other test and fails in a
long-lived process that reuses freed blocks.  Here each path is built from scratch three times under tests/poison.py -- every
torch.empty tensor on the device pre-filled with 0x00 bytes, with NaN (integers: words of 1) and with 3.39e38 (integers: words of
2) -- and run on the same seeded inputs.  The three runs must agree under torch.equal: the arithmetic is the same, so anything
else is a dependence on memory nobody wrote.  Every test asserts that the helper did fill tensors of the module under test.

The second half owns the buffers: the scratch arguments of the C ABI pre-filled the same way, and NaN in the channels / rows /
columns the descriptors declare as padding."""
import ctypes
import functools
import gc
import os

import numpy as np
import pytest
import torch

from gpu_common import GOLDEN, _dev, _stream
from m3dssd_amd import _hip, synth
from poison import FILLS, poisoned_allocations

pytestmark = pytest.mark.gpu

CROP, B2 = (128, 320), 2
FULL = (384, 1280)


# ------------------------------------------------------------------------------------ helpers
def _thrice(run, *modules):
    """run() once per fill, each time from scratch; returns {fill: result}.  `modules`: path suffixes of the files whose
    allocations the case is about -- the helper must have filled at least one tensor from each of them."""
    out = {}
    for fill in FILLS:
        gc.collect()
        with poisoned_allocations(fill) as st:
            out[fill] = run()
            torch.cuda.synchronize()
        assert st.tensors > 0 and st.bytes > 0, "the helper filled nothing under %r" % fill
        for m in modules:
            assert st.from_file(m) > 0, "no allocation of %s was filled (%s)" % (m, sorted(st.by_file))
    return out


def _equal(a, b):
    """torch.equal, or the same bytes (a NaN the API itself specifies, e.g. an absent statistic, equals itself here)."""
    if torch.equal(a, b):
        return True
    return a.shape == b.shape and a.dtype == b.dtype and \
        torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _assert_same(res, what=""):
    """res = {fill: {name: tensor}}: every tensor of the nan and huge runs torch.equal to the zero run's."""
    ref = res["zero"]
    for fill in ("nan", "huge"):
        got = res[fill]
        assert sorted(got) == sorted(ref), (what, fill)
        bad = [k for k in ref if not _equal(ref[k], got[k])]
        assert not bad, "%s: under %r these differ from the zero-filled run: %s" % (what, fill, bad[:12])


def _rows_below_counts(dets, counts):
    """Detections as a comparable dict: the counts and, per image, the rows below its count.  Rows at or above a count are
    unspecified by the detection API (they happen to be zero in the gather block): they are not compared."""
    out = {"counts": counts.clone()}
    for b, k in enumerate(counts.tolist()):
        out["rows%d" % b] = dets[b, :k].clone()
    return out


@functools.lru_cache(maxsize=None)
def _sd(config, back_bone):
    flags = synth.config_flags(config)
    return synth.synth_state_dict(0, back_bone=back_bone, **flags)


def _build(config, crop, B, dtype="f32", back_bone="dla34"):
    """A new network (new engine, new packed weights, new plan buffers), the way tests/test_gpu_configs.py and
    tests/test_gpu_dla102.py build theirs."""
    from model.M3d_inference_align import build
    flags = synth.config_flags(config)
    conf = synth.synth_conf(crop, 0, batch_size=B, device="cuda:0", back_bone=back_bone, **flags)
    net = build(conf, "test")
    net.load_state_dict(_sd(config, back_bone), strict=True)
    net.set_compute_dtype(dtype)
    return net.to(_dev()), conf


def _valid(v):
    """The region of a plan buffer its writer owns: [..., :c] of an NHWC view with pixel stride cs (the padding bytes between c
    and cs legitimately differ between fills), the whole of a plain tensor."""
    if torch.is_tensor(v):
        return v.clone()
    if hasattr(v, "cs") and torch.is_tensor(getattr(v, "t", None)):
        off = (v.ptr - v.t.data_ptr()) // v.t.element_size()
        return v.t.view(v.n, v.h, v.w, v.cs)[..., off:off + v.c].clone()
    return None


def _engine_run(make, B, crop, named=True):
    """x1, x2, x1 through net(x) (fresh outputs), then detect_batch(x1) (the plan-owned outputs + the detection stage) -> every
    returned tensor, the detections, every named plan buffer's valid region, and the plan's op kinds."""
    from lib.rpn_util import detect_batch
    dev = _dev()
    x1, x2 = synth.synth_frames(B, crop, 1234).to(dev), synth.synth_frames(B, crop, 4321).to(dev)
    net, conf = make()
    with torch.no_grad():
        a = [t.clone() for t in net(x1)]
        b = [t.clone() for t in net(x2)]
        c = [t.clone() for t in net(x1)]
    # scratch a kernel leaves dirty for the next step would show here, inside one build
    for i, (u, v) in enumerate(zip(a, c)):
        assert torch.equal(u, v), "output %d of x1 differs after a forward of x2" % i
    assert not torch.equal(a[3], b[3])
    res = {"x1.%d" % i: t for i, t in enumerate(a)}
    res.update({"x2.%d" % i: t for i, t in enumerate(b)})
    dets, counts = detect_batch(net, x1, conf)
    assert int(counts.sum()) > 0
    res.update({"det." + k: v for k, v in _rows_below_counts(dets, counts).items()})
    plan = net.engine().plan_for(B, *crop)
    if named:
        for k, v in plan.named.items():
            t = _valid(v)
            if t is not None:
                res["named." + k] = t
    torch.cuda.synchronize()
    return res, [op[1] for op in plan.ops], [op[0] for op in plan.ops]


def _engine_case(make, B, crop, module, named=True):
    runs = _thrice(lambda: _engine_run(make, B, crop, named), module)
    _assert_same({f: r[0] for f, r in runs.items()}, module)
    assert runs["zero"][1] == runs["nan"][1] == runs["huge"][1]
    if named:
        assert sum(k.startswith("named.") for k in runs["zero"][0]) >= 10
    return runs["zero"][1], runs["zero"][2]


ENGINE_FILE = {"f32": "m3dssd_amd/engine.py", "bf16": "m3dssd_amd/engine_bf16.py"}


# ------------------------------------------------------------------------------------ engines
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("config", ["anab_fullalign", "base", "anab"])
def test_dla34_engine_outputs_and_plan_buffers(config, dtype):
    """DLA-34, the default (fullalign), base and ANAB-only configurations, fp32 and bf16, crop 128x320, B = 2."""
    kinds, names = _engine_case(lambda: _build(config, CROP, B2, dtype), B2, CROP, ENGINE_FILE[dtype])
    with_anab = config != "base"
    assert any(k.startswith("anab") or k.startswith("bf16_anab") for k in kinds) == with_anab
    assert (("align" in kinds) == (config == "anab_fullalign")) and names[-1] == "bundle_outputs"
    if dtype == "bf16":
        fam = {k.split("<")[0] for k in kinds}
        assert {"bf16_frontend2", "bf16_head2", "bf16_tree_entry", "bf16_halo"} <= fam, kinds
        assert "bf16_dcn_patch" in fam or "bf16_conv<128,deform>" in kinds or "bf16_conv<64,deform>" in kinds, kinds
    else:
        assert any(k.startswith("head_mlp") for k in kinds) and any(k.startswith("igemm") or k.startswith("conv_wave") for k in kinds)


@pytest.mark.parametrize("config", ["anab_fullalign", "base"])
def test_dla102_engine_outputs_and_plan_buffers(config):
    """DLA-102 as tests/test_gpu_dla102.py builds it (fp32: the bf16 engine has no DLA-102 walk)."""
    kinds, names = _engine_case(lambda: _build(config, CROP, B2, "f32", "dla102"), B2, CROP, ENGINE_FILE["f32"])
    assert sum(n.endswith(".conv3") for n in names) >= 20, "not the DLA-102 tree of Bottlenecks (DLA-34 has no conv3)"
    assert any(k.startswith("anab") for k in kinds) == (config != "base")
    assert any(k.startswith("head_mlp<3") for k in kinds)


def _full_f32(route, monkeypatch):
    import m3dssd_amd.engine as E
    if route == "no_wino44":
        monkeypatch.setattr(E, "USE_WINO44", False)
    elif route == "no_wgsplit":
        monkeypatch.setattr(E, "USE_CONV_WAVE_WGSPLIT", False)
    elif route == "no_offmask_wave":
        monkeypatch.setattr(E, "USE_OFFMASK_WAVE", False)
    else:
        assert route == "default"


@pytest.mark.parametrize("route", ["default", "no_wino44", "no_wgsplit", "no_offmask_wave"])
def test_fp32_benchmarked_plan_and_its_switched_routes(route, monkeypatch):
    """The fp32 plan bench.py measures (B = 8, 1280x384: kernel choice depends on shape) and the routes the suite switches on it:
    M3D_WINO44=0 (F(2x2) wave kernel and its split-K workspace), M3D_CONV_WAVE_WGSPLIT=0 (the wave conv's global split-K workspace +
    reduce launch), M3D_OFFMASK_WAVE=0 (the offset / mask convs back on the split-K igemm) -- by their module flags."""
    _full_f32(route, monkeypatch)
    kinds, names = _engine_case(lambda: _build("anab_fullalign", FULL, 8, "f32"), 8, FULL, ENGINE_FILE["f32"], named=False)
    wave = [k for k in kinds if k.startswith("conv_wave")]
    om_wg = [n for n, k in zip(names, kinds) if "wgsplit" in k and n.endswith(".offset_mask")]
    if route == "no_wino44":
        assert any(k.startswith("wino_wave") for k in kinds) and not any(k.startswith("wino44<") for k in kinds), kinds
    else:
        assert any(k.startswith("wino44<") and "splitk" in k for k in kinds), kinds       # the F(4x4) split-K workspace
    if route == "no_wgsplit":
        assert not any("wgsplit" in k for k in kinds) and any("splitk" in k for k in wave), wave
    elif route == "no_offmask_wave":
        assert not om_wg and any("wgsplit" in k for k in wave), wave
    else:
        assert len(om_wg) == 4 and not any("splitk" in k for k in wave), wave
    assert any(k.startswith("igemm") and "splitk" in k for k in kinds), kinds                # the igemm split-K workspace


def test_bf16_benchmarked_plan():
    """The bf16 plan bench.py measures: B = 64, 1280x384 (the kernel families of the bf16 soak test)."""
    kinds, _ = _engine_case(lambda: _build("anab_fullalign", FULL, 64, "bf16"), 64, FULL, ENGINE_FILE["bf16"], named=False)
    fam = {k.split("<")[0] for k in kinds}
    assert {"bf16_halo", "bf16_conv", "bf16_head2", "bf16_frontend2", "bf16_anab", "bf16_dcn_patch"} <= fam, fam


# (fused ANAB, bf16 K|V, fused heads, fused front end, round-5 heads, fused tree entry): the A/B forms of
# tests/test_gpu_bf16.py::test_bf16_engine_alternative_paths_agree (its first row, the default, is covered above)
BF16_ALTS = [(False, True, True, True, True, True), (True, False, True, True, True, True), (False, False, True, True, True, True),
             (True, True, False, True, True, True), (True, True, True, False, True, True), (True, True, True, True, False, True),
             (True, True, True, True, True, False)]


# a 16x48 feature map: the pooling windows nest there, so the K|V form (KV_BF16) is a choice; at 16x40 both take the item list
CROP_NESTED = (128, 384)
BF16_ALT_CASES = [(CROP, a) for a in BF16_ALTS] + [(CROP_NESTED, (True,) * 6)] + [(CROP_NESTED, a) for a in BF16_ALTS[:3]]


@pytest.mark.parametrize("crop,alt", BF16_ALT_CASES, ids=lambda v: "x".join(str(int(e)) for e in v))
def test_bf16_engine_alternative_paths(crop, alt, monkeypatch):
    from m3dssd_amd import engine_bf16
    fused, kv16, heads, front, heads2, entry = alt
    for name, v in zip(("FUSED_ANAB", "KV_BF16", "FUSED_HEADS", "FUSED_FRONT", "HEADS2", "TREE_ENTRY"), alt):
        monkeypatch.setattr(engine_bf16, name, v)
    kinds, names = _engine_case(lambda: _build("anab_fullalign", crop, B2, "bf16"), B2, crop, ENGINE_FILE["bf16"])
    kinds = set(kinds)
    nested = crop == CROP_NESTED
    kv16 = kv16 and nested
    assert ("anab.pool_nested" in names) == nested and ("anab.pool_partial" in names) == (not nested)
    assert ("bf16_anab" in kinds) == fused and ("softmax_bf16" in kinds) == (not fused)
    assert ("bf16_head2" in kinds) == (heads and heads2) and ("bf16_head_mlp" in kinds) == (heads and not heads2)
    assert ("bf16_frontend2" in kinds) == front and ("stem_bf16" in kinds) == (not front)
    assert ("bf16_tree_entry" in kinds) == entry
    assert ("bf16_qkvs" in kinds) == (kv16 and heads2)
    assert ("anab.kvs" in names) == (not kv16) and ("convert" in kinds) == (not kv16)


# ------------------------------------------------------------------------------------ detection and serving
def _p2():
    return np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884],
                     [0.0, 0.0, 0.0, 1.0]])


def _meta(i):
    p2 = _p2()
    return {"p2": np.stack([p2, p2 * np.array([[1.0 + 0.01 * i], [1.0], [1.0], [1.0]])]),
            "scale": np.array([1.0, 0.9 - 0.1 * i], np.float32), "clip_wh": np.array([[0, 0], [300, 100 + i]], np.float32)}


def _refined(rows, counts):
    """Refined rows [B, K, 16] below the counts (the rest is unspecified for a caller that has only the counts)."""
    return {"refined%d" % b: rows[b, :k].clone() for b, k in enumerate(counts.tolist())}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_detect_batch_with_and_without_scale(dtype):
    from m3dssd_amd.host.detect import detect_batch

    def run():
        net, conf = _build("anab_fullalign", CROP, B2, dtype)
        res = {}
        for i in range(2):
            x = synth.synth_frames(B2, CROP, 40 + i).to(_dev())
            d, c = detect_batch(net, x, conf)
            res.update({"plain%d.%s" % (i, k): v for k, v in _rows_below_counts(d, c).items()})
            d, c = detect_batch(net, x, conf, scale=np.array([1.0, 0.8], np.float32))
            res.update({"scaled%d.%s" % (i, k): v for k, v in _rows_below_counts(d, c).items()})
        assert int(res["plain0.counts"].sum()) > 0 and not torch.equal(res["plain0.rows1"], res["scaled0.rows1"])
        return res
    _assert_same(_thrice(run, "m3dssd_amd/host/detect.py", ENGINE_FILE[dtype]), "detect_batch")


@pytest.mark.parametrize("mode", ["plain", "refine", "uint8"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_frame_detector(dtype, mode):
    """FrameDetector warms up outside capture: the buffers its graph owns are allocated (and poisoned) there; what is allocated
    while capturing is left as it is (counted by the helper, not filled)."""
    from m3dssd_amd.pipeline import FrameDetector
    fh, fw = 120, 310

    def run():
        net, conf = _build("anab_fullalign", CROP, B2, dtype)
        det = FrameDetector(net, conf, CROP[0], CROP[1], batch=B2, refine=(mode == "refine"),
                            u8_frame=(fh, fw) if mode == "uint8" else None)
        res = {}
        rng = np.random.RandomState(3)
        for i in range(3):
            if mode == "uint8":
                x = torch.from_numpy(rng.randint(0, 256, size=(B2, fh, fw, 3)).astype(np.uint8)).to(_dev())
            else:
                x = synth.synth_frames(B2, CROP, 20 + i).to(_dev())
            r = det.detect(x, meta=_meta(i)) if mode == "refine" else det.detect(x)
            res.update({"f%d.%s" % (i, k): v for k, v in _rows_below_counts(r[0], r[1]).items()})
            if mode == "refine":
                res.update({"f%d.%s" % (i, k): v for k, v in _refined(r[2], r[1]).items()})
                assert float(r[2][:, :, 0].sum()) > 0
        assert int(res["f0.counts"].sum()) > 0 and not torch.equal(res["f0.rows0"], res["f1.rows0"])
        return res
    _assert_same(_thrice(run, "m3dssd_amd/host/detect.py", ENGINE_FILE[dtype]), "FrameDetector")


@pytest.mark.parametrize("planar", [True, False])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_pipelined_detector_step_pair(dtype, planar):
    from m3dssd_amd.pipeline import PipelinedDetector

    def run():
        net, conf = _build("anab_fullalign", CROP, B2, dtype)
        pipe = PipelinedDetector(net, conf, B2, CROP[0], CROP[1], planar=planar)
        xs = [synth.synth_frames(B2, CROP, 40 + i).to(_dev()) for i in range(2)]
        assert pipe.step(xs[0]) is None
        res = {"k0." + k: v for k, v in _rows_below_counts(*pipe.step(xs[1])).items()}
        res.update({"k1." + k: v for k, v in _rows_below_counts(*pipe.flush()).items()})
        assert int(res["k0.counts"].sum()) > 0 and not torch.equal(res["k0.rows0"], res["k1.rows0"])
        return res
    _assert_same(_thrice(run, "m3dssd_amd/host/detect.py", ENGINE_FILE[dtype]), "PipelinedDetector")


def test_nms_sorted():
    from m3dssd_amd.host import ops
    g = torch.Generator().manual_seed(5)
    B, n = 3, 777                                              # no multiple of 64: a ragged last mask word
    cx, cy = torch.rand(B, n, generator=g) * 400, torch.rand(B, n, generator=g) * 200
    w, h = torch.rand(B, n, generator=g) * 80 + 5, torch.rand(B, n, generator=g) * 60 + 5
    boxes = torch.stack([cx, cy, cx + w, cy + h, torch.rand(B, n, generator=g).sort(descending=True).values], 2).to(_dev())

    def run():
        res = {}
        for name, bx in (("batched", boxes), ("single", boxes[1, :130])):
            keep, num = ops.nms_sorted(bx, 0.4)
            res[name + ".num"] = num.clone()
            for b, k in enumerate(num.tolist()):                # keep[b, num[b]:] is unspecified
                res["%s.keep%d" % (name, b)] = keep[b, :k].clone()
        assert 0 < int(res["batched.num"].min()) and int(res["batched.num"].max()) < n
        return res
    _assert_same(_thrice(run, "m3dssd_amd/host/ops.py"), "nms_sorted")


def test_refine_detections():
    from m3dssd_amd.host import refine as HR
    g = np.load(os.path.join(GOLDEN, "refine.npz"))
    rows = g["rows"]
    dets = np.zeros((2, 40, 14), dtype=np.float32)
    dets[0] = rows[:40]
    dets[1, :8] = rows[40:]
    dets[1, 8:] = 123.0
    d = torch.from_numpy(dets).to(_dev())
    counts = torch.tensor([40, 8], dtype=torch.int32, device=_dev())

    def run():
        res = {"all": HR.refine_detections(d, counts, g["p2"]).clone(),      # rows past the counts are documented as zeros
               "no_hill": HR.refine_detections(d, counts, g["p2"], hill_climbing=False).clone(),
               "scaled": HR.refine_detections(d, counts, g["p2"], scale=[1.0, 0.9], clip_wh=[[0, 0], [300, 100]]).clone()}
        assert float(res["all"][:, :, 0].sum()) > 0 and not res["all"][1, 8:].any()
        return res
    _assert_same(_thrice(run, "m3dssd_amd/host/refine.py"), "refine_detections")


def test_preprocess():
    from m3dssd_amd.host.preprocess import preprocess
    g = np.load(os.path.join(GOLDEN, "preprocess.npz"))
    rng = np.random.RandomState(3)
    frames = torch.from_numpy(rng.randint(0, 256, size=(3, 50, 70, 3)).astype(np.uint8)).to(_dev())   # padded to 64x96

    def run():
        out = preprocess(frames, (64, 96), g["mean"], g["stds"]).clone()
        assert out.shape == (3, 3, 64, 96) and torch.isfinite(out).all()
        return {"out": out}
    _assert_same(_thrice(run, "m3dssd_amd/host/preprocess.py"), "preprocess")


def test_rotate_iou_eval():
    from m3dssd_amd.eval.eval import rotate_iou_eval
    rng = np.random.RandomState(11)

    def boxes(n):
        return np.concatenate([rng.rand(n, 2) * 20, rng.rand(n, 2) * 4 + 1, rng.rand(n, 1) * 6 - 3], 1).astype(np.float32)
    a, q = boxes(67), boxes(45)                                # neither a multiple of the 64-box tile

    def run():
        res = {"iou%d" % c: torch.from_numpy(rotate_iou_eval(a, q, criterion=c)) for c in (-1, 0, 1)}
        assert float(res["iou-1"].max()) > 0
        return res
    _assert_same(_thrice(run, "m3dssd_amd/eval/eval.py"), "rotate_iou_eval")


# ------------------------------------------------------------------------------------ training ops
def _dcn_inputs(dg):
    """The smallest parity case of tests/test_gpu_dcn_backward.py (3x3, stride 1, pad 1, Ho * Wo = 99) with dg deformable groups:
    (input, offset, mask, weight, bias, grad_output) on the device + the host case for the float64 reference."""
    import dcn_grad_ref as R
    ts, go, args = R.make_case(2, 8, 6, 9, 11, 3, 1, 1, 1, dg, 0.5, 10)
    return [t.to(_dev()).contiguous() for t in ts + (go,)], (ts, go, args)


@pytest.mark.parametrize("dg", [1, 2])
def test_dcn_v2_forward_and_backward(dg):
    """Forward and four of the five gradients: the same bits under every fill.  grad_input is accumulated with float atomics (the
    header: "may differ in its last bits between runs"), so bit equality is not its contract: each fill's grad_input is held to
    the float64 reference of tests/dcn_grad_ref.py within the bound of tests/test_gpu_dcn_backward.py, 2e-4 (1 + |ref|) -- a
    NaN or 3.39e38 that leaked in would miss it by orders of magnitude."""
    import dcn_grad_ref as R
    from m3dssd_amd.host import ops
    from test_gpu_dcn_backward import BOUND
    (inp, off, mask, wgt, bias, gout), (ts, go, args) = _dcn_inputs(dg)
    ref_gin = R.ref_grads(ts, go, args)[1][0]

    def run():
        res = {"out": ops.dcn_v2_forward(inp, off, mask, wgt, bias, 1, 1, 1, dg).clone()}
        for name, t in zip(("g_input", "g_offset", "g_mask", "g_weight", "g_bias"),
                           ops.dcn_v2_backward(inp, off, mask, wgt, gout, 1, 1, 1, dg)):
            res[name] = t.clone()
        part = ops.dcn_v2_backward(inp, off, mask, wgt, gout, 1, 1, 1, dg, needs=(False, True, False, True, False))
        assert part[0] is None and part[2] is None and part[4] is None
        res["g_offset_alone"], res["g_weight_alone"] = part[1].clone(), part[3].clone()
        assert all(torch.isfinite(t).all() for t in res.values()) and float(res["g_offset"].abs().max()) > 0
        return res
    runs = _thrice(run, "m3dssd_amd/host/ops.py")
    for fill, res in runs.items():
        g = res.pop("g_input").cpu().double()
        err = float(((g - ref_gin).abs() / (1.0 + ref_gin.abs())).max())
        print("dcn_v2 dg=%d fill=%s: grad_input vs float64 reference %.3e (bound %.1e)" % (dg, fill, err, BOUND))
        assert err <= BOUND, (fill, err)
    _assert_same(runs, "dcn_v2 dg=%d" % dg)


def test_rpn_targets_and_loss():
    """The smallest case of tests/test_gpu_rpn_loss.py (the shipped 128x320 golden batch): targets, then loss, stats, the sampled
    mask and all three gradients.  The workspace holds float partials in a byte buffer (the helper gives it small words only):
    test_cabi_scratch_contents_do_not_matter fills it with NaN as well."""
    from m3dssd_amd.host import loss as hl
    from m3dssd_amd.host import ops
    from test_gpu_rpn_loss import _case
    conf, case = _case("shipped")
    dev = _dev()
    cls, prob, b2, b3, imobjs, fs = case
    vec = hl.pack_conf(conf.bbox_means, conf.bbox_stds, conf.fg_thresh, conf.ign_thresh, conf.bg_thresh_lo, conf.bg_thresh_hi,
                       conf.best_thresh, conf.box_samples, conf.fg_fraction, conf.focal_loss, conf.cls_2d_lambda, conf.iou_2d_lambda,
                       conf.bbox_2d_lambda, conf.bbox_3d_lambda, conf.feat_stride)
    table = hl.pack_gts(imobjs, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h)
    anchors = torch.from_numpy(np.asarray(conf.anchors, dtype=np.float64)).to(dev)

    def run():
        res = dict(zip(("t.labels", "t.gt_index", "t.targets", "t.scores"),
                       (t.clone() for t in ops.rpn_targets(cls.to(dev), prob.to(dev), anchors, vec, table, fs))))
        ins = [t.to(dev).requires_grad_(True) for t in (cls, b2, b3)]
        loss, stats, det = ops.rpn_loss(ins[0], prob.to(dev), ins[1], ins[2], anchors, vec, table, fs, return_details=True)
        loss.backward()
        res.update(loss=loss.detach().clone(), stats=stats.clone(), sampled=det["sampled"].clone(), labels=det["labels"].clone(),
                   targets=det["targets"].clone())
        for k, t in zip(("g_cls", "g_bbox_2d", "g_bbox_3d"), ins):
            res[k] = t.grad.clone()
        assert torch.isfinite(res["loss"]) and int((res["sampled"] == 1).sum()) > 0 and float(res["g_bbox_3d"].abs().max()) > 0
        return res
    _assert_same(_thrice(run, "m3dssd_amd/host/loss.py"), "rpn_loss")


# ------------------------------------------------------------------------------------ C ABI: the test owns the scratch
# What the scratch of an entry holds on entry must not matter.  "float": the header documents fp32 / fp64 partials -> bytes
# 0x00, 0xFF (NaN) and 0x7F (3.39e38); "words": it documents counters, flags or bit masks -> 32-bit words 0, 1, 2 (small on
# purpose: a word read before it is written stays inside every buffer).  Workspaces that hold both get both.
def _scratch(nbytes, fill, kind):
    """A device buffer of at least nbytes (+ 256 spare), 256-byte aligned, pre-filled; returns (tensor, pointer)."""
    from poison import poison_
    t = torch.zeros((int(nbytes) + 3) // 4 + 128, dtype=torch.int32, device=_dev())
    poison_(t.view(torch.float32) if kind == "float" else t, fill)
    return t, (t.data_ptr() + 255) // 256 * 256


def _conv_nhwc_case(x, wt, bias, act, res, **kw):
    """host.standalone.conv_nhwc with the split-K workspace it allocates (fp32, torch.empty) under each fill."""
    from m3dssd_amd.host import standalone as S
    dev = _dev()
    v, _ = S._to_nhwc(x.to(dev))
    rv = S._to_nhwc(res.to(dev))[0] if res is not None else None
    wd, bd = wt.to(dev), None if bias is None else bias.to(dev)
    outs = {}
    for fill in FILLS:
        with poisoned_allocations(fill) as st, torch.no_grad():
            out, keep = S.conv_nhwc(v, wd, bd, None, 1, 1, act=act, res=rv, **kw)
            outs[fill] = {"out": S._to_nchw(out, wt.shape[0]).clone()}
            torch.cuda.synchronize()
        assert keep[3] is not None, "the layer did not take its split-K form"
        assert st.from_file("m3dssd_amd/host/standalone.py") > 0 and st.by_dtype[torch.float32] > 0
    return outs


def _case_conv2d_splitk():
    n, ci, h, w, co = 3, 512, 4, 10, 512                              # level5-like, small M (gpu_common.CONV_CASES): split by default
    g = torch.Generator().manual_seed(1)
    x, wt = torch.randn(n, ci, h, w, generator=g), torch.randn(co, ci, 3, 3, generator=g) / (ci * 9) ** 0.5
    return _conv_nhwc_case(x, wt, torch.randn(co, generator=g), 1, torch.randn(n, co, h, w, generator=g))


def _case_wino_splitk(case):
    n, ci, h, w, co, sg = case
    g = torch.Generator().manual_seed(2)
    x, wt = torch.randn(n, ci, h, w, generator=g), torch.randn(co, ci, 3, 3, generator=g) / (ci * 9) ** 0.5
    return _conv_nhwc_case(x, wt, torch.randn(co, generator=g), 0 if sg >= 0 else 1, None, sigmoid_from=sg, wino=True,
                           wino_variant=1, wino_splitk=True)


def _case_wino44_splitk():
    n, ci, h, w, co = 4, 128, 24, 80, 500                             # Cout 500 (pad 512): the smallest split case of test_gpu_conv.py
    g = torch.Generator().manual_seed(3)
    x, wt = torch.randn(n, ci, h, w, generator=g), torch.randn(co, ci, 3, 3, generator=g) / (ci * 9) ** 0.5
    return _conv_nhwc_case(x, wt, torch.randn(co, generator=g), 0, None, wino44=True, wino44_nb=2, wino_splitk=True)


def _case_conv_wave_splitk(name):
    import test_gpu_conv_wgsplit as T
    L = _hip.lib()
    d, out, want, co, out_cs, keep = T._case(name)
    unsplit = T._run(L.m3d_conv_wave_forward, d, out)
    outs = {}
    for fill in FILLS:
        ws, ptr = _scratch(8 * T.H * T.W * d.Cout_pad * 4, fill, "float")
        d.splitk_ws, d.splitk_ws_bytes = ptr, 8 * T.H * T.W * d.Cout_pad * 4
        outs[fill] = {"out": T._run(L.m3d_conv_wave_forward, d, out)}
        d.splitk_ws, d.splitk_ws_bytes = None, 0
    assert not torch.equal(outs["zero"]["out"], unsplit), "the workspace split did not run"
    return outs


def _case_anab_pool(form):
    """partial + finish, nested and nested_bf16_ex on the 32x48 map of test_anab_nested_pooling_matches_generic_pooling."""
    from m3dssd_amd.engine import Engine
    L, dev = _hip.lib(), _dev()
    B, H, W, ck, cv = 2, 32, 48, 40, 24
    C = ck + cv
    g = torch.Generator().manual_seed(11)
    kv = torch.randn(B, H, W, C, generator=g).to(dev)
    kv16 = kv.to(torch.bfloat16).contiguous()
    gate = torch.rand(B, H, W, 4, generator=g).to(dev)
    items, bin_scale, bin_slots, bin_inv = Engine._anab_items(H, W)
    n_bins, max_slots, keys_pad, ck_pad = len(bin_scale), int(bin_slots.max()), 352, 64
    d_items, d_bs = torch.from_numpy(items).to(dev), torch.from_numpy(bin_scale).to(dev)
    d_sl, d_inv = torch.from_numpy(bin_slots).to(dev), torch.from_numpy(bin_inv).to(dev)
    outs = {}
    for fill in FILLS:
        khat, vhatT = torch.zeros(B, keys_pad, ck_pad, device=dev), torch.zeros(B, cv, keys_pad, device=dev)
        res = {"khat": khat, "vhatT": vhatT}
        if form == "partial_finish":
            ws, p = _scratch(B * n_bins * max_slots * C * 4, fill, "float")
            _hip.check(L.m3d_anab_pool_partial(kv.data_ptr(), C, gate.data_ptr(), 4, d_items.data_ptr(), items.shape[0],
                                               d_bs.data_ptr(), n_bins, p, max_slots, B, H, W, C, _stream()))
            _hip.check(L.m3d_anab_pool_finish(p, d_sl.data_ptr(), d_inv.data_ptr(), n_bins, max_slots, ck, cv, khat.data_ptr(),
                                              keys_pad, ck_pad, vhatT.data_ptr(), B, 0, _stream()))
        else:
            ws, p = _scratch(L.m3d_anab_pool_nested_scratch_bytes(B, C), fill, "float")
            if form == "nested":
                _hip.check(L.m3d_anab_pool_nested(kv.data_ptr(), C, gate.data_ptr(), 4, B, H, W, ck, cv, p, khat.data_ptr(), keys_pad,
                                                  ck_pad, vhatT.data_ptr(), 0, _stream()))
            else:
                k16 = torch.zeros(B, keys_pad, ck_pad, device=dev, dtype=torch.bfloat16)
                v16 = torch.zeros(B, cv, keys_pad, device=dev, dtype=torch.bfloat16)
                _hip.check(L.m3d_anab_pool_nested_bf16_ex(kv16.data_ptr(), C, gate.data_ptr(), 4, B, H, W, ck, cv, p, khat.data_ptr(),
                                                          keys_pad, ck_pad, vhatT.data_ptr(), 0, k16.data_ptr(), v16.data_ptr(), _stream()))
                res.update(khat16=k16, vhat16=v16)
        torch.cuda.synchronize()
        assert float(khat.abs().max()) > 0 and torch.isfinite(khat).all() and torch.isfinite(vhatT).all()
        outs[fill] = res
    return outs


def _case_topk(entry, kind):
    """m3d_topk_decode on the bundled tensors (B = 3, R = 5000, k = 700), the planar forms on R = 10007, k = 3000 (not a multiple
    of 4), the multi-workgroup one with 7 workgroups per image (empty last slices)."""
    from gpu_common import _sortable_bits, _topk_inputs
    L, dev = _hip.lib(), _dev()
    g = torch.Generator().manual_seed(5)
    B = 3
    R, k = (5000, 700) if entry == "bundled" else (10007, 3000)
    scores = torch.rand(B, R, generator=g) ** 6
    scores[:, ::9] = 0.5                                              # ties across the cut
    bits = torch.from_numpy(_sortable_bits(scores).numpy().astype(np.uint32).view(np.int32)).to(dev)
    if entry == "bundled":
        prob = torch.zeros(B, R, 4)
        prob[:, :, 1] = scores
        b2, b3 = torch.randn(B, R, 4, generator=g), torch.randn(B, R, 7, generator=g)
        _, _, _, rois, anchors, means, stds = _topk_inputs(R, 36, 1, scores[0])
        d = [t.to(dev).contiguous() for t in (prob, b2, b3, rois, anchors, means, stds)]
        nb = L.m3d_topk_decode_workspace_bytes(B, R)
    else:
        from test_gpu_frame_detector import _planar_inputs
        d = _planar_inputs(B, R, g)
        nb = L.m3d_topk_decode_mw_workspace_bytes(B, R, k) if entry == "planar_mw" else L.m3d_topk_decode_workspace_bytes(B, R)
    outs = {}
    for fill in FILLS:
        ws, p = _scratch(nb, fill, kind)
        ab = torch.zeros(B, k, 14, device=dev)
        rows = torch.zeros(B, k, device=dev, dtype=torch.int32)
        ptrs = [bits.data_ptr(), *[t.data_ptr() for t in d]]
        if entry == "bundled":
            _hip.check(L.m3d_topk_decode(*ptrs, ab.data_ptr(), rows.data_ptr(), p, nb, B, R, k, _stream()))
        elif entry == "planar":
            _hip.check(L.m3d_topk_decode_planar(*ptrs, None, ab.data_ptr(), rows.data_ptr(), p, nb, B, 1, R, k, _stream()))
        else:
            _hip.check(L.m3d_topk_decode_planar_mw(*ptrs, None, ab.data_ptr(), rows.data_ptr(), p, nb, B, 1, R, k, 7, _stream()))
        torch.cuda.synchronize()
        outs[fill] = {"aboxes": ab, "rows": rows}
    key = _sortable_bits(scores).numpy().astype(np.int64)
    for b in range(B):
        assert np.array_equal(outs["zero"]["rows"][b].cpu().numpy(), np.lexsort((np.arange(R), -key[b]))[:k])
    return outs


def _case_nms():
    L, dev = _hip.lib(), _dev()
    B, n = 2, 3000                                                    # synth boxes as in test_nms_batched_device_api_and_properties
    from oracle import nms as onms
    dets = np.stack([synth.synth_boxes(n, seed=100 + i) for i in range(B)])
    srt = torch.from_numpy(np.stack([d[onms.order_desc_stable(d[:, 4])] for d in dets])).to(dev).contiguous()
    outs = {}
    for fill in FILLS:
        ws, p = _scratch(L.m3d_nms_workspace_bytes(B, n), fill, "words")      # bit masks
        keep, _ = _scratch(B * n * 4, fill, "words")
        num, _ = _scratch(B * 4, fill, "words")
        _hip.check(L.m3d_nms_sorted_dev(srt.data_ptr(), B, n, 5, 0.4, p, keep.data_ptr(), num.data_ptr(), _stream()))
        torch.cuda.synchronize()
        nk = num[:B].tolist()
        assert all(0 < v < n for v in nk)
        outs[fill] = {"num": num[:B].clone(), **{"keep%d" % b: keep[b * n:b * n + v].clone() for b, v in enumerate(nk)}}
    return outs


def _case_dcn_v2_forward(dg):
    L = _hip.lib()
    (inp, off, mask, wgt, bias, _), _ = _dcn_inputs(dg)
    n, c, h, w = inp.shape
    co, k = wgt.shape[0], wgt.shape[2]
    nb = L.m3d_dcn_v2_workspace_bytes_grouped(n, c, h, w, co, k, k, 1, 1, 1, dg)
    outs = {}
    for fill in FILLS:
        ws, p = _scratch(nb, fill, "float")                           # the reference's `ones` / `columns` tensors
        out, _ = _scratch(n * co * h * w * 4, fill, "float")
        _hip.check(L.m3d_dcn_v2_forward(inp.data_ptr(), wgt.data_ptr(), bias.data_ptr(), off.data_ptr(), mask.data_ptr(),
                                        out.data_ptr(), n, c, h, w, co, k, k, 1, 1, 1, 1, 1, 1, dg, p, nb, _stream()))
        torch.cuda.synchronize()
        outs[fill] = {"out": out.view(torch.float32)[:n * co * h * w].clone()}
        assert torch.isfinite(outs[fill]["out"]).all()
    return outs


def _case_rpn_loss(kind):
    """m3d_rpn_targets + m3d_rpn_loss on one workspace (the loss must get the targets' workspace untouched): gt maxima, best rows,
    counters, the selection block and the float64 partial sums of the loss launch all live in it."""
    from m3dssd_amd.host import loss as hl
    from test_gpu_rpn_loss import _case
    conf, case = _case("shipped")
    dev = _dev()
    cls, prob, b2, b3, imobjs, fs = (t.to(dev) if torch.is_tensor(t) else t for t in case)
    vec = hl.pack_conf(conf.bbox_means, conf.bbox_stds, conf.fg_thresh, conf.ign_thresh, conf.bg_thresh_lo, conf.bg_thresh_hi,
                       conf.best_thresh, conf.box_samples, conf.fg_fraction, conf.focal_loss, conf.cls_2d_lambda, conf.iou_2d_lambda,
                       conf.bbox_2d_lambda, conf.bbox_3d_lambda, conf.feat_stride)
    table = hl.pack_gts(imobjs, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h)
    anchors = torch.from_numpy(np.asarray(conf.anchors, dtype=np.float64)).to(dev)
    outs = {}
    for fill in FILLS:
        ctx = hl._Ctx(anchors, vec, table, fs, cls.shape[0], cls.shape[1], dev)
        ctx.ws, ctx.ws_base = _scratch(ctx.ws_bytes, fill, kind)
        labels, gidx, targets, scores = hl._targets(ctx, cls, prob)
        loss, stats, sampled, grads = hl._loss(ctx, cls, b2, b3, labels, targets, scores)
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and int((sampled == 1).sum()) > 0
        outs[fill] = dict(labels=labels, gt_index=gidx, targets=targets, scores=scores, loss=loss, stats=stats, sampled=sampled,
                          g_cls=grads[0], g_bbox_2d=grads[1], g_bbox_3d=grads[2])
    return outs


def _case_dcn_ws_flags(hand_over):
    """The per-tile flag words of the bf16 LDS-patch DCNv2 kernel: every word 0, 1 or 2 on entry.  hand_over: one offset beyond
    the window radius, so that a tile raises its flag and the implicit-GEMM kernel behind recomputes what touches it."""
    from gpu_common import _run_conv
    from test_gpu_bf16 import _dcn_case
    x, wt, b, off, m, om = _dcn_case((2, 64, 16, 32, 128), 1.0, 2, 4.0)
    if hand_over:
        om = om.clone()
        om[1, 7, 9, 5] = 10.25
    base = _run_conv(x, wt, b, None, 1, 1, 0, None, 0, -1, 0, om, variant=0)
    outs = {f: {"out": _run_conv(x, wt, b, None, 1, 1, 0, None, 0, -1, 0, om, variant=4, patch=True, ws_word=i)}
            for i, f in enumerate(FILLS)}
    got = outs["zero"]["out"]
    assert not torch.equal(got[0], base[0]), "the patch kernel did not run"
    assert torch.equal(got[1], base[1]) == hand_over, "image 1: the implicit-GEMM kernel's bits exactly when a tile handed over"
    return outs


def _case_refine():
    """m3d_refine_3d_ex has no scratch; it owns every element of its output block (rows past a count are documented as zeros)."""
    L, dev = _hip.lib(), _dev()
    g = np.load(os.path.join(GOLDEN, "refine.npz"))
    rows, p2 = g["rows"], np.asarray(g["p2"], dtype=np.float64)
    dets = np.zeros((2, 40, 14), dtype=np.float32)
    dets[0] = rows[:40]
    dets[1, :8] = rows[40:]
    dets[1, 8:] = 123.0
    d, counts = torch.from_numpy(dets).to(dev), torch.tensor([40, 8], dtype=torch.int32, device=dev)
    P = torch.from_numpy(np.stack([p2, p2]).reshape(2, 16)).to(dev)
    Pi = torch.from_numpy(np.stack([np.linalg.inv(p2)] * 2).reshape(2, 16)).to(dev)
    outs = {}
    for fill in FILLS:
        out, _ = _scratch(2 * 40 * 16 * 8, fill, "float")
        _hip.check(L.m3d_refine_3d_ex(d.data_ptr(), counts.data_ptr(), 2, 40, P.data_ptr(), Pi.data_ptr(), None, None, 0.75, 1,
                                      0.3 * np.pi, 0.01, out.data_ptr(), _stream()))
        torch.cuda.synchronize()
        o = out.view(torch.float64)[:2 * 40 * 16].view(2, 40, 16).clone()
        assert float(o[:, :, 0].sum()) > 0 and not o[1, 8:].any()
        outs[fill] = {"out": o}
    return outs


SCRATCH_CASES = {
    "m3d_conv2d_forward.splitk": _case_conv2d_splitk,
    "m3d_conv_wave_forward.splitk.deform": lambda: _case_conv_wave_splitk("deform_c64_co128_s4_resmode1"),
    "m3d_conv_wave_forward.splitk.plain": lambda: _case_conv_wave_splitk("plain_3x3_stride2_c64_co128_s4"),
    "m3d_wino_conv3x3_forward_ex.splitk": lambda: _case_wino_splitk((2, 256, 8, 20, 256, -1)),
    "m3d_wino_conv3x3_forward_ex.splitk.sigmoid": lambda: _case_wino_splitk((1, 128, 10, 12, 27, 18)),
    "m3d_wino44_conv3x3_forward_ex.splitk": _case_wino44_splitk,
    "m3d_anab_pool_partial+finish": lambda: _case_anab_pool("partial_finish"),
    "m3d_anab_pool_nested": lambda: _case_anab_pool("nested"),
    "m3d_anab_pool_nested_bf16_ex": lambda: _case_anab_pool("nested_bf16_ex"),
    "m3d_topk_decode.words": lambda: _case_topk("bundled", "words"),
    "m3d_topk_decode.bytes": lambda: _case_topk("bundled", "float"),
    "m3d_topk_decode_planar.words": lambda: _case_topk("planar", "words"),
    "m3d_topk_decode_planar.bytes": lambda: _case_topk("planar", "float"),
    "m3d_topk_decode_planar_mw.words": lambda: _case_topk("planar_mw", "words"),
    "m3d_topk_decode_planar_mw.bytes": lambda: _case_topk("planar_mw", "float"),
    "m3d_nms_sorted_dev": _case_nms,
    "m3d_dcn_v2_forward.dg1": lambda: _case_dcn_v2_forward(1),
    "m3d_dcn_v2_forward.dg2": lambda: _case_dcn_v2_forward(2),
    "m3d_rpn_loss.words": lambda: _case_rpn_loss("words"),
    "m3d_rpn_loss.bytes": lambda: _case_rpn_loss("float"),
    "bf16_dcn_patch.dcn_ws": lambda: _case_dcn_ws_flags(False),
    "bf16_dcn_patch.dcn_ws.hand_over": lambda: _case_dcn_ws_flags(True),
    "m3d_refine_3d_ex": _case_refine,
}


@pytest.mark.parametrize("entry", sorted(SCRATCH_CASES))
def test_cabi_scratch_contents_do_not_matter(entry):
    _assert_same(SCRATCH_CASES[entry](), entry)


# ------------------------------------------------------------------------------------ C ABI: NaN in declared padding
# n, c, h, w, co of the case of each variant (tests/test_bf16_conv_route_host.py asks the library about them without a GPU)
BF16_CONV_SHAPES = {0: (2, 64, 12, 20, 64), 1: (2, 64, 15, 31, 64), 2: (128, 64, 24, 96, 64), 5: (1, 64, 8, 16, 128),
                    8: (8, 64, 128, 256, 64), 6: (1, 128, 9, 13, 128), 3: (3, 64, 8, 16, 128), 4: (1, 32, 16, 16, 100)}


def _bf16_conv_args(variant):
    """One case per bf16 convolution variant (m3d_conv_bf16_variant), the smallest of its test in tests/test_gpu_bf16.py, with
    in_cs = Cin + 8: the eight channels between Cin and in_cs belong to nobody."""
    from test_gpu_bf16 import _dcn_case, _r
    g = torch.Generator().manual_seed(40 + variant)

    def plain(n, c, h, w, co):
        return (_r(torch.randn(n, c, h, w, generator=g)), _r(torch.randn(co, c, 3, 3, generator=g) / (c * 9) ** 0.5),
                torch.randn(co, generator=g) * 0.1)
    if variant in (0, 1, 2, 5, 8):
        n, c, h, w, co = BF16_CONV_SHAPES[variant]
        x, wt, b = plain(n, c, h, w, co)
        return (x, wt, b, None, 1, 1, 1), dict(out_mode=1 if variant == 2 else 0, in_cs=c + 8, variant=variant, wide=variant == 5)
    if variant == 6:                                                  # 1x1 DCNv2 128 -> 128 on a ragged single tile
        n, c, h, w, _ = BF16_CONV_SHAPES[variant]
        x = _r(torch.randn(n, c, h, w, generator=g) + 0.5)
        wt, b = _r(torch.randn(c, c, 1, 1, generator=g) / c ** 0.5), torch.randn(c, generator=g) * 0.1
        om = torch.cat([torch.randn(n, 2, h, w, generator=g) * 2.5, torch.rand(n, 1, h, w, generator=g), torch.zeros(n, 1, h, w)],
                       1).permute(0, 2, 3, 1).contiguous()
        return (x, wt, b, None, 1, 0, 0), dict(om=om, in_cs=c + 8, variant=6)
    shape, std = BF16_CONV_SHAPES[variant], {3: 0.3, 4: 1.0}[variant]
    x, wt, b, off, m, om = _dcn_case(shape, std, 1, None)
    return (x, wt, b, None, 1, 1, 0), dict(om=om, in_cs=shape[1] + 8, variant=variant, patch=True)


@pytest.mark.parametrize("variant", [0, 1, 2, 5, 8, 3, 4, 6])
def test_bf16_conv_ignores_nan_between_cin_and_in_cs(variant):
    """The descriptor gives Cin and the pixel stride in_cs: the channels in between are not the kernel's.  With NaN there the
    output must be finite and the bits of the run whose padding holds the finite sentinel (768.0)."""
    from gpu_common import _run_conv
    args, kw = _bf16_conv_args(variant)
    want = _run_conv(*args, **kw)
    got = _run_conv(*args, pad_value=float("nan"), **kw)
    assert torch.isfinite(got).all(), "NaN from the channels between Cin and in_cs reached the output"
    assert torch.equal(got, want)
    assert float(want.abs().max()) > 0


@pytest.mark.parametrize("entry", ["f32", "bf16"])
def test_anab_attend_ignores_nan_in_the_padding_of_khat_and_vhat(entry):
    """Both attention entries: the rows of khat and the columns of vhatT past `keys`, and -- in the fp32 entry, which takes Ck and the
    row stride k_cs -- the columns of khat past Ck (tests/test_gpu_conv.py and tests/test_gpu_bf16.py fill them with 7.0) hold NaN
    here; the output must be finite and equal to the run with 7.0.  The bf16 entry has no Ck argument: it multiplies all Ck_pad
    columns, those of q being zero by its contract, so the columns [Ck, Ck_pad) of the VALID khat rows are operand, not padding,
    and stay zero."""
    L, dev = _hip.lib(), _dev()
    g = torch.Generator().manual_seed(7)
    B, h, w, keys, cv = 2, 8, 16, 337, 128
    HW = h * w
    BF16 = torch.bfloat16
    res = torch.randn(B * HW, cv, generator=g)
    scale, shift = (torch.rand(cv, generator=g) + 0.5).to(dev), (torch.randn(cv, generator=g) * 0.1).to(dev)
    outs = {}
    if entry == "f32":
        ck = 168
        kcs, kp, qcs = ck + 24, (keys + 31) // 32 * 32, ck + 8
        q, khat = torch.randn(B * HW, ck, generator=g) * 0.5, torch.randn(B, keys, ck, generator=g) * 0.3
        vhat = torch.randn(B, cv, keys, generator=g)
        for pad in (7.0, float("nan")):
            dq = torch.full((B * HW, qcs), 3.0)
            dq[:, :ck] = q
            dk = torch.full((B, kp, kcs), pad)
            dk[:, :keys, :ck] = khat
            dv = torch.full((B, cv, kp), pad)
            dv[:, :, :keys] = vhat
            dq, dk, dv, dr = (t.contiguous().to(dev) for t in (dq, dk, dv, res))
            out = torch.full((B * HW, cv + 4), 512.0, device=dev)
            _hip.check(L.m3d_anab_attend_f32(dq.data_ptr(), qcs, dk.data_ptr(), kcs, dv.data_ptr(), B, HW, ck, keys, kp, cv, dr.data_ptr(),
                                             cv, 1, scale.data_ptr(), shift.data_ptr(), 1, out.data_ptr(), cv + 4, _stream()))
            torch.cuda.synchronize()
            assert (out[:, cv:] == 512.0).all()
            outs[pad == 7.0] = out[:, :cv].clone()
    else:
        ck, ckp = 168, 192
        kp = (keys + 63) // 64 * 64
        q = torch.zeros(B * HW, ckp)                                  # (the header wants q's channels [Ck, Ck_pad) zero: they are the caller's)
        q[:, :ck] = torch.randn(B * HW, ck, generator=g) * 0.5
        kh, vh = torch.randn(B, keys, ck, generator=g) * 0.3, torch.randn(B, cv, keys, generator=g)
        for pad in (7.0, float("nan")):
            dk = torch.full((B, kp, ckp), pad)
            dk[:, :keys] = 0.0
            dk[:, :keys, :ck] = kh
            dv = torch.full((B, cv, kp), pad)
            dv[:, :, :keys] = vh
            dq, dk, dv, dr = (t.to(BF16).contiguous().to(dev) for t in (q, dk, dv, res))
            out = torch.full((B * HW, cv + 8), 512.0, device=dev, dtype=BF16)
            _hip.check(L.m3d_anab_attend_bf16(dq.data_ptr(), ckp, dk.data_ptr(), dv.data_ptr(), B, HW, ckp, keys, kp, cv, dr.data_ptr(), cv,
                                              scale.data_ptr(), shift.data_ptr(), 1, out.data_ptr(), cv + 8, _stream()))
            torch.cuda.synchronize()
            assert (out[:, cv:].float() == 512.0).all()
            outs[pad == 7.0] = out[:, :cv].float().clone()
    assert torch.isfinite(outs[True]).all()
    assert torch.isfinite(outs[False]).all(), "NaN from the padding of khat / vhatT reached the output"
    assert torch.equal(outs[False], outs[True])
