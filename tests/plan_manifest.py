"""The plan manifest: what a launch plan and the packed parameters of an engine look like from outside, as plain JSON data.

``dump_case`` is shared by tools/gen_golden_plan_manifest.py (which records tests/golden/plan_manifest.json.gz) and
tests/test_gpu_plan_manifest.py (which compares a freshly built plan with the record, with no tolerance).  It reads only the
surface that bench.py, pipeline.py, host/detect.py and the tests read: the 5-slot ops, ``plan.branches`` / ``tail`` /
``tail_start`` / ``named`` and ``eng.P``.  Building a plan launches nothing but the parameter packing."""
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
# id -> m3dssd_amd.engine_bf16 module attributes set while the case's engine and plan are built: the bf16 backbone paths that the
# defaults do not reach (the un-fused tree entries; stem, level0 and level1 as three launches)
KNOBS = {}
for _knob in ("TREE_ENTRY", "FUSED_FRONT"):
    _id = "bf16-anab_fullalign-b2-128x320-%s=False" % _knob
    CASES[_id] = CASES["bf16-anab_fullalign-b2-128x320"]
    KNOBS[_id] = {_knob: False}


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


def dump_case(case_id):
    from m3dssd_amd import engine_bf16
    dtype, config, back_bone, B, crop = CASES[case_id]
    knobs = KNOBS.get(case_id, {})
    saved = {k: getattr(engine_bf16, k) for k in knobs}
    try:
        for k, v in knobs.items():
            setattr(engine_bf16, k, v)
        eng = build_engine(dtype, config, back_bone, B, crop)
        plan = eng.plan_for(B, *crop)
    finally:
        for k, v in saved.items():
            setattr(engine_bf16, k, v)
    tail = plan.tail
    dense = plan.ops[plan.tail_start:-1] if tail is not None else []
    return {
        "ops": [[op[0], op[1], op[2], _cost(op[4])] for op in plan.ops],
        "branches": [list(br) for br in plan.branches],
        "tail_start": plan.tail_start,
        "tail": None if tail is None else [op[0] for op in tail],
        # per tail entry behind need_rows: is it the dense op itself (the same object)?
        "tail_is_dense": None if tail is None else [t is d for t, d in zip(tail[1:], dense)],
        "named": sorted(plan.named),
        "P": {k: _param(eng.P[k]) for k in sorted(eng.P)},
    }
