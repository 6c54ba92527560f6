"""CPU checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/m3dssd_hip.h declares (no compute calls -- there is no GPU here), the ctypes signature table
covers exactly the header, and the import-path shims expose the reference's names."""
import ctypes
import os
import re

import pytest
import torch

from m3dssd_amd import _hip


def _declared():
    hdr = open(_hip.HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(m3d_[a-z0-9_]+|_nms)\s*\(", hdr))


def test_library_exports_every_declared_symbol():
    assert os.path.exists(_hip.SO_PATH), "run __graft_entry__.build() first"
    L = _hip.lib()
    names = _declared()
    assert len(names) >= 25
    for n in names:
        assert hasattr(L, n), n
    assert names == set(_hip.SIGNATURES), (names ^ set(_hip.SIGNATURES))
    assert L.m3d_abi_version() == 5


def test_lib_types_every_declared_symbol():
    """lib() has set restype / argtypes, from the table, on every function the header declares."""
    L = _hip.lib()
    names = _declared()
    assert len(names) == len(_hip.SIGNATURES) >= 126
    for n in names:
        fn, (res, args) = getattr(L, n), _hip.SIGNATURES[n]
        assert fn.argtypes is not None and list(fn.argtypes) == args, n
        assert fn.restype is res, n
        assert res in (None, ctypes.c_int, ctypes.c_longlong, ctypes.c_char_p), (n, res)
    assert L._nms.restype is None and L.m3d_last_error.restype is ctypes.c_char_p and L.m3d_last_error.argtypes == []


def test_abi_version_mismatch_is_refused(monkeypatch):
    """A library built from a header of another M3D_ABI_VERSION is refused at load, with both numbers and the build command."""
    monkeypatch.setattr(_hip, "_lib", None)
    monkeypatch.setitem(_hip.CONSTANTS, "M3D_ABI_VERSION", 6)
    with pytest.raises(RuntimeError, match=r"(?s)version 5\b.*declares 6\b.*build\(\)"):
        _hip.lib()
    assert _hip._lib is None


def _header_structs():
    """{struct: [(field, "ptr" or its scalar type words)]} read off the header text, independently of the binding's reader."""
    hdr = re.sub(r"/\*.*?\*/", "", open(_hip.HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"typedef struct (\w+) \{(.*?)\} \1;", hdr, flags=re.S):
        fields = out[m.group(1)] = []
        for decl in m.group(2).split(";")[:-1]:
            first, *more = decl.split(",")
            words = first.replace("*", " * ").split()
            base = " ".join(w for w in words[:-1] if w not in ("const", "*"))
            fields.append((words[-1], "ptr" if "*" in words else base))
            fields += [(d.strip().lstrip("* "), "ptr" if d.strip().startswith("*") else base) for d in more]
    return out


def test_conv_desc_layout_matches_header():
    """Field order/count of the ctypes structures follows the C structs (names differ only for `in`), and every field has the
    class of its declaration: a pointer, or the scalar of that width."""
    scalar = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float}
    structs = _header_structs()
    assert sorted(structs) == sorted(_hip.STRUCTS) and len(structs) == 8
    for name, fields in structs.items():
        cls = _hip.STRUCTS[name]
        assert cls is getattr(_hip, "".join(w.capitalize() for w in name.split("_")[1:]))
        assert [("in" if n == "inp" else n) for n, _ in cls._fields_] == [n for n, _ in fields], name
        for (n, kind), (_, ctype) in zip(fields, cls._fields_):
            assert ctype is (ctypes.c_void_p if kind == "ptr" else scalar[kind]), (name, n, kind, ctype)
    assert _hip.STRUCTS["m3d_conv_desc"] is _hip.ConvDesc and _hip.STRUCTS["m3d_head2_bf16_desc"] is _hip.Head2Bf16Desc
    hdr = open(_hip.HEADER).read()
    body = hdr[hdr.index("typedef struct m3d_conv_desc {"):hdr.index("} m3d_conv_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";")[:-1]:
        decl = decl.split("{")[-1].strip()
        if not decl:
            continue
        names = decl.replace("*", " ").split()
        first = len([t for t in names if t in ("const", "float", "int", "long")])
        fields += [n.strip(",") for n in names[first:]]
    mine = [("in" if n == "inp" else n) for n, _ in _hip.ConvDesc._fields_]
    assert fields == mine


def test_shims_expose_reference_names():
    import lib.nms.gpu_nms as g
    import lib.rpn_util as r
    import model.DCNv2.dcn_v2 as d
    import model.M3d_inference_align as m
    import model.module.attention as a
    import model.module.feturealign_mgpu as f
    import model.pose_dla_dcn as p
    for mod, names in ((m, ["build", "RPN"]), (p, ["DLASeg", "DeformConv", "DLA", "dla34", "IDAUp", "DLAUp"]),
                       (d, ["DCNv2", "DCN"]), (a, ["ANAB", "PAPAModule"]), (f, ["center_align", "shape_align"]),
                       (g, ["gpu_nms"]), (r, ["locate_anchors", "calc_output_size", "flatten_tensor", "im_detect_3d"])):
        for n in names:
            assert hasattr(mod, n), (mod.__name__, n)


def test_product_path_fails_loudly_without_a_gpu():
    """No CPU fallback anywhere on the product path."""
    from m3dssd_amd import synth
    from model.M3d_inference_align import build
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    conf = synth.synth_conf((128, 320), 0, device="cpu")
    net = build(conf, "test")
    with pytest.raises(NotImplementedError):
        net(torch.zeros(1, 3, 128, 320))
    import model.DCNv2.dcn_v2 as d
    with pytest.raises(NotImplementedError):
        d.DCNv2(4, 4, 3, 1, 1)(torch.zeros(1, 4, 4, 4), torch.zeros(1, 18, 4, 4), torch.zeros(1, 9, 4, 4))


def test_product_does_not_import_the_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bad = []
    for base in ("m3dssd_amd", "model", "lib"):
        for dp, _, files in os.walk(os.path.join(root, base)):
            for f in files:
                if f.endswith((".py", ".hip", ".h", ".cpp")):
                    txt = open(os.path.join(dp, f)).read()
                    if re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M) or "liboracle" in txt:
                        bad.append(os.path.join(dp, f))
    assert not bad, bad
