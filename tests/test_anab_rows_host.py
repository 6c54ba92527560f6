"""Host-only checks of the row-list attention entry point: declared as additive, bound with the header's argument count, the dense
entry's arguments first, and every refusal returns before anything is launched (no GPU here)."""
import ctypes
import re

from m3dssd_amd import _hip

NAME, DENSE = "m3d_anab_attend_f32_rows", "m3d_anab_attend_f32"


def _params(body, name):
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, body)
    assert m, "%s is not declared in include/m3dssd_hip.h" % name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_entry_point_is_declared_additive_and_bound():
    hdr = open(_hip.HEADER).read()
    history = hdr.split("#define M3D_ABI_VERSION")[0]
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = _hip.lib()
    assert L.m3d_abi_version() == 5
    assert NAME in history                                             # listed under "added under 5"
    rows, dense = _params(body, NAME), _params(body, DENSE)
    assert len(rows) == 22 == len(_hip.SIGNATURES[NAME][1])
    # the dense entry's arguments, then the device list and its length in front of the stream
    assert rows == dense[:-1] + ["const int *rows", "const int *n_rows", dense[-1]]
    assert _hip.SIGNATURES[NAME][1][:19] == _hip.SIGNATURES[DENSE][1][:19]
    assert hasattr(L, NAME)


def test_refusals_launch_nothing():
    L = _hip.lib()
    buf = (ctypes.c_char * 64)()                                       # 16-byte aligned stand-in for every pointer
    p = (ctypes.addressof(buf) + 15) & ~15

    def call(**kw):
        a = dict(q=p, khat=p, vhatT=p, HW=256, Ck=168, keys=337, keys_pad=352, Cv=128, out=p, rows=p, n_rows=p)
        a.update(kw)
        return L.m3d_anab_attend_f32_rows(a["q"], 192, a["khat"], 192, a["vhatT"], 3, a["HW"], a["Ck"], a["keys"], a["keys_pad"], a["Cv"],
                                          None, 0, 0, None, None, 0, a["out"], 128, a["rows"], a["n_rows"], None)

    assert call(rows=None) == -1 and b"row list" in L.m3d_last_error()
    assert call(n_rows=None) == -1 and b"row list" in L.m3d_last_error()
    assert call(q=None) == -1
    assert call(HW=200) == -1 and b"multiple of 128" in L.m3d_last_error()
    assert call(Ck=96) == -1
    assert call(Ck=64, Cv=256) == -1 and b"Ck = 168" in L.m3d_last_error()
    assert call(keys=353) == -1
    assert call(out=p + 4) == -1 and b"aligned" in L.m3d_last_error()
