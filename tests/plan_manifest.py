"""The plan manifest: what a launch plan and the packed parameters of an engine look like from outside, as plain JSON data.

``dump_case`` is shared by tools/gen_golden_plan_manifest.py (which records tests/golden/plan_manifest.json.gz) and
tests/test_gpu_plan_manifest.py (which compares a freshly built plan with the record, with no tolerance).  It reads only the
surface that bench.py, pipeline.py, host/detect.py and the tests read: the 5-slot ops, ``plan.branches`` / ``tail`` /
``tail_start`` / ``named`` and ``eng.P``, and of a descriptor in slot 4 every field (``_desc``).  Building a plan launches nothing but
the parameter packing."""
import ctypes
import importlib

import torch

from m3dssd_amd import synth

# id -> (dtype, configuration, back_bone, B, crop)
CASES = {}
for _dt in ("f32", "bf16"):
    for _cfg in ("base", "anab", "anab_fullalign"):
        CASES["%s-%s-b2-128x320" % (_dt, _cfg)] = (_dt, _cfg, "dla34", 2, (128, 320))
# a 12x28 feature map: no multiple of 128 pixels, so the unfused attention and a tail with no row-list attention
CASES["f32-anab_fullalign-b2-96x224"] = ("f32", "anab_fullalign", "dla34", 2, (96, 224))
CASES["f32-dla102-anab_fullalign-b1-128x320"] = ("f32", "anab_fullalign", "dla102", 1, (128, 320))
# The fp32 conv planner chooses a kernel family by workgroup counts against the chip (WINO44_MIN_WGS_NB1, WINO_MIN_BLOCKS, the
# library's wave thresholds), which the B = 2 maps above never reach: there every conv is an igemm.  The benchmark's shape reaches
# F(4x4) (plain, split-K, K-pair, own and folded touch), F(2x2), the wave kernel (plain, workgroup-split, deformable) and the igemm;
# tests/size_cases.py's batch of 20 sends the unfused ANAB GEMMs to the wave kernel with fragment-ordered per-image weights.
BENCH = ("f32", "anab_fullalign", "dla34", 8, (384, 1280))
CASES["f32-anab_fullalign-b8-384x1280"] = BENCH
CASES["f32-anab_fullalign-b20-160x192"] = ("f32", "anab_fullalign", "dla34", 20, (160, 192))
# id -> {"module.ATTRIBUTE" of m3dssd_amd: value} set while the case's engine and plan are built.  engine_bf16: the bf16 backbone paths
# that the defaults do not reach (the un-fused tree entries; stem, level0 and level1 as three launches).  engine: the routes of the
# fp32 conv planner that the defaults do not reach at the benchmark's shape -- F(2x2) where F(4x4) would run, no Winograd at all, no
# wave kernel (igemm with the deformable gather and split-K), the wave kernel's split-K through a workspace, the offset / mask convs
# on the split-K igemm, F(4x4) with no split-K, with 128-channel workgroups, with no touch and with a touch launch per layer, and
# the unfused ANAB chain.
KNOBS = {}
for _knob in ("TREE_ENTRY", "FUSED_FRONT"):
    _id = "bf16-anab_fullalign-b2-128x320-%s=False" % _knob
    CASES[_id] = CASES["bf16-anab_fullalign-b2-128x320"]
    KNOBS[_id] = {"engine_bf16." + _knob: False}
for _knobs in ({"USE_WINO44": False}, {"USE_WINO": False}, {"USE_CONV_WAVE": False, "USE_DCN_WAVE": False},
               {"USE_CONV_WAVE_WGSPLIT": False}, {"USE_OFFMASK_WAVE": False}, {"USE_WINO44_SPLITK": False}, {"WINO44_MIN_WGS": 200},
               {"WINO44_TOUCH": False}, {"WINO44_TOUCH_SPAN": 0}, {"FUSED_ANAB": False}):
    _id = "f32-anab_fullalign-b8-384x1280-" + ",".join("%s=%s" % kv for kv in _knobs.items())
    CASES[_id] = BENCH
    KNOBS[_id] = {"engine." + k: v for k, v in _knobs.items()}


def build_engine(dtype, config, back_bone, B, crop):
    from model.M3d_inference_align import build
    flags = synth.config_flags(config)
    conf = synth.synth_conf(crop, 0, batch_size=B, device="cuda:0", back_bone=back_bone, **flags)
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0, back_bone=back_bone, **flags), strict=True)
    net.set_compute_dtype(dtype)
    return net.to(torch.device("cuda:0")).engine()


def _tensor(t):
    """dtype and shape as one short string, e.g. "float32[64,3,3]"."""
    return "%s[%s]" % (str(t.dtype).replace("torch.", ""), ",".join(str(d) for d in t.shape))


def _param(v):
    if v is None:
        return None
    if torch.is_tensor(v):
        return _tensor(v)
    if isinstance(v, (list, tuple)):
        return [_param(e) for e in v]
    return {"class": type(v).__name__, "dims": [v.cout, v.cin, v.kh, v.kw, v.cout_pad],
            "tensors": {k: _tensor(t) for k, t in sorted(vars(v).items()) if torch.is_tensor(t)}}


def _cost(c):
    if c is None:
        return None
    if hasattr(c, "hbm_bytes"):
        return {"hbm_bytes": c.hbm_bytes}
    return [type(c).__name__, len(c) if hasattr(c, "__len__") else 1]


def _desc(d):
    """Every field of a ctypes descriptor: integers and floats by value, pointers as "null" / "ptr"; None for any other slot."""
    if not isinstance(d, ctypes.Structure):
        return None
    out = {}
    for name, ctype in d._fields_:
        v = getattr(d, name)
        pointer = issubclass(ctype, (ctypes.c_void_p, ctypes.c_char_p, ctypes._Pointer))
        out[name] = ("ptr" if v else "null") if pointer else v
    return out


def dump_case(case_id):
    dtype, config, back_bone, B, crop = CASES[case_id]
    knobs = [(importlib.import_module("m3dssd_amd." + k.split(".")[0]), k.split(".")[1], v) for k, v in KNOBS.get(case_id, {}).items()]
    saved = [(mod, attr, getattr(mod, attr)) for mod, attr, _ in knobs]
    try:
        for mod, attr, v in knobs:
            setattr(mod, attr, v)
        eng = build_engine(dtype, config, back_bone, B, crop)
        plan = eng.plan_for(B, *crop)
    finally:
        for mod, attr, v in saved:
            setattr(mod, attr, v)
    tail = plan.tail
    dense = plan.ops[plan.tail_start:-1] if tail is not None else []
    return {
        "ops": [[op[0], op[1], op[2], _cost(op[4]), _desc(op[4])] for op in plan.ops],
        "branches": [list(br) for br in plan.branches],
        "tail_start": plan.tail_start,
        "tail": None if tail is None else [op[0] for op in tail],
        # per tail entry behind need_rows: is it the dense op itself (the same object)?
        "tail_is_dense": None if tail is None else [t is d for t, d in zip(tail[1:], dense)],
        "named": sorted(plan.named),
        "P": {k: _param(eng.P[k]) for k in sorted(eng.P)},
    }
