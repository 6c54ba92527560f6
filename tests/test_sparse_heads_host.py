"""Host-only checks of the needed-pixel entry points: declared as additive, bound with the header's argument counts, and every
refusal returns before anything is launched (no GPU here)."""
import ctypes
import re

from m3dssd_amd import _hip

NEW = {"m3d_need_rows_workspace_bytes": 2, "m3d_need_rows": 12, "m3d_head_mlp_forward_rows": 6, "m3d_align_offsets_gated": 18}


def test_entry_points_are_declared_additive_and_bound():
    hdr = open(_hip.HEADER).read()
    history = hdr.split("#define M3D_ABI_VERSION")[0]
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = _hip.lib()
    assert L.m3d_abi_version() == 5
    for name, nargs in NEW.items():
        assert name in history, name                                   # listed under "added under 5"
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, body)
        assert m, "%s is not declared in include/m3dssd_hip.h" % name
        assert len(m.group(1).split(",")) == nargs == len(_hip.SIGNATURES[name][1]), name
        assert hasattr(L, name)


def test_need_rows_workspace_rule_and_refusals():
    L = _hip.lib()
    f = L.m3d_need_rows_workspace_bytes
    assert f(0, 640) == -1 and f(2, 0) == -1
    assert f(2, 640) == 2 * 3 * 2048 * 4 + 2 * 3 * 4                   # three histograms + one count per 256-pixel slice
    assert f(8, 7680) == 8 * 3 * 2048 * 4 + 8 * 30 * 4
    buf = (ctypes.c_char * 64)()                                       # 16-byte aligned stand-in for every pointer: nothing is launched
    p = (ctypes.addressof(buf) + 15) & ~15
    nb = f(2, 640)
    args = lambda **kw: [kw.get("bits", p), 2, 36, 640, kw.get("k", 3000), p, p, kw.get("rows", p), p, p, kw.get("nb", nb), None]
    assert L.m3d_need_rows(*args(k=0)) == -1 and b"need_rows" in L.m3d_last_error()
    assert L.m3d_need_rows(*args(bits=None)) == -1
    assert L.m3d_need_rows(*args(rows=None)) == -1
    assert L.m3d_need_rows(*args(bits=p + 4)) == -1                    # misaligned keys
    assert L.m3d_need_rows(*args(nb=nb - 1)) == -3 and b"workspace" in L.m3d_last_error()


def test_head_rows_and_gated_offsets_refusals():
    L = _hip.lib()
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    d = _hip.MlpDesc()
    d.inp, d.in_cs, d.M, d.Cin, d.HW = p, 128, 1280, 128, 640
    for slot in "123":
        for k in "wst":
            setattr(d, k + slot, p)
    d.Cout, d.Cout_pad, d.out, d.out_img_stride = 36, 64, p, 36 * 640
    arr = (_hip.MlpDesc * 1)(d)
    assert L.m3d_head_mlp_forward_rows(arr, 1, None, p, 1, None) == -1 and b"row list" in L.m3d_last_error()
    assert L.m3d_head_mlp_forward_rows(arr, 1, p, None, 1, None) == -1
    assert L.m3d_head_mlp_forward_rows(arr, 1, p, p, 0b10, None) == -1 and b"sparse_head_mask" in L.m3d_last_error()
    d.Cout_pad = 256
    assert L.m3d_head_mlp_forward_rows((_hip.MlpDesc * 1)(d), 1, p, p, 1, None) == -1 and b"Cout_pad" in L.m3d_last_error()
    d.Cout_pad, d.w1 = 64, None
    d.Cin = 256
    assert L.m3d_head_mlp_forward_rows((_hip.MlpDesc * 1)(d), 1, p, p, 1, None) == -1   # two-layer form
    assert L.m3d_align_offsets_gated(p, p, 0.5, p, p, p, 0.0, 1.0, 0.0, 1.0, None, p, 4, 2, 36, 640, 11 * 36 * 640, None) == -1
    assert b"need map" in L.m3d_last_error()
