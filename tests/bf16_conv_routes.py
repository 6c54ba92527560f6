"""Descriptors for m3d_conv_bf16_variant on the host (tests/test_bf16_conv_route_host.py, tools/gen_golden_bf16_conv_routes.py).

The query reads no memory behind a descriptor's pointers, only whether they are null: every pointer here is a made-up non-null
address and nothing is allocated.  The library is opened with ctypes alone (no torch, no device), so that

    python tests/bf16_conv_routes.py

can be started as a fresh process per knob setting: it prints the codes of PROBES, separated by blanks.
"""
import ctypes
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from m3dssd_amd import _hip  # noqa: E402

RECORD = os.path.join(ROOT, "tests", "golden", "bf16_conv_routes.json.gz")
ADDR = 0x10000                # a made-up, 16-byte aligned, non-null address

# the descriptor grid, itertools.product in this order
GRID = (
    ("k", (1, 3)),
    ("stride", (1, 2)),
    ("cin", (16, 64, 128)),
    ("cout_pad", (32, 64, 128)),                                       # = Cout
    ("hw", ((8, 16), (16, 32), (12, 40), (24, 80), (15, 31), (7, 16))),
    ("n", (1, 2, 1024)),
    ("deform", (0, 1)),
    ("wgt_wave", (0, 1)),
    ("patch", (0, 1)),                                                  # wgt_f16 + dcn_ws
    ("out_mode", (0, 1, 2)),
    ("sigmoid_from", (-1, 18)),
    ("groups", (1, 2)),
    ("per_image", (0, 1)),
)

# one descriptor per route and per way to fall off one (3x3 / stride 1 / pad 1 but the 1x1 DCNv2): n, cin, h, w, cout_pad, options
PROBES = (
    ("c64", (2, 64, 16, 32, 64), {}),
    ("halo16", (2, 128, 16, 32, 128), {}),
    ("halo32", (1024, 128, 8, 32, 64), {}),
    ("wide", (2, 64, 8, 16, 128), dict(wgt_wave=1)),
    ("dcn1x1", (2, 128, 8, 16, 128), dict(k=1, deform=1)),
    ("patch8", (2, 64, 8, 16, 128), dict(deform=1, patch=1)),
    ("patch16", (2, 64, 16, 32, 128), dict(deform=1, patch=1)),
    ("deform without wgt_f16", (2, 64, 8, 16, 128), dict(deform=1)),
    ("deform with wgt_f16 and wgt_wave", (2, 64, 16, 32, 128), dict(deform=1, patch=1, wgt_wave=1)),
)

_lib = None


def lib():
    """The library through ctypes alone, with the two entry points the descriptors need."""
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(_hip.SO_PATH)
        for name in ("m3d_conv_bf16_variant", "m3d_conv_bf16_dcn_ws_bytes"):
            getattr(_lib, name).restype, getattr(_lib, name).argtypes = _hip.SIGNATURES[name]
    return _lib


def desc(n, cin, h, w, cout_pad, k=3, stride=1, cout=None, d=None, **options):
    """The descriptor of one case: pad = k // 2, Kpad = k * k * Cin rounded up to 64, in_cs = Cin, out_cs = Cout_pad, and the
    `options` of set_options.  d: a descriptor to fill again instead of a new one."""
    d = _hip.ConvBf16Desc() if d is None else d
    pad = k // 2
    d.inp, d.in_cs, d.N, d.H, d.W, d.Cin = ADDR, cin, n, h, w, cin
    d.wgt, d.Cout, d.Cout_pad, d.Kpad = ADDR, cout_pad if cout is None else cout, cout_pad, (k * k * cin + 63) // 64 * 64
    d.kh, d.kw, d.stride, d.pad = k, k, stride, pad
    d.Ho, d.Wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    d.out, d.out_cs = ADDR, cout_pad
    d.dcn_om_cs = 28 if k == 3 else 4              # the rows of the offset / mask map, where the case has one
    d.dcn_ws_bytes = max(1024, lib().m3d_conv_bf16_dcn_ws_bytes(n, d.Ho, d.Wo))        # of the patch workspace, likewise
    return set_options(d, **options)


def set_options(d, deform=0, wgt_wave=0, patch=0, out_mode=0, sigmoid_from=-1, groups=1, per_image=0):
    """What a case has beyond its geometry: an offset / mask map, fragment-ordered weights, the fp16 weights and the workspace of the
    LDS-patch kernel, the output mode, a sigmoid, groups, per-image weight sets of Cout_pad * Kpad elements."""
    d.dcn_offmask = ADDR if deform else None
    d.wgt_wave = ADDR if wgt_wave else None
    d.wgt_f16 = d.dcn_ws = ADDR if patch else None
    d.out_mode, d.sigmoid_from, d.groups = out_mode, sigmoid_from, groups
    d.wgt_img_stride = d.Cout_pad * d.Kpad if per_image else 0
    return d


def code(*shape, **options):
    """What m3d_conv_bf16_variant answers for desc(*shape, **options)."""
    return lib().m3d_conv_bf16_variant(ctypes.byref(desc(*shape, **options)))


def grid_codes():
    """The codes of the whole grid, in its order, one digit each."""
    query, d = lib().m3d_conv_bf16_variant, _hip.ConvBf16Desc()
    ref = ctypes.byref(d)
    values = [v for _, v in GRID]
    assert [name for name, _ in GRID[:6]] == ["k", "stride", "cin", "cout_pad", "hw", "n"]
    out = []
    for k, stride, cin, cout_pad, (h, w), n in itertools.product(*values[:6]):
        desc(n, cin, h, w, cout_pad, k, stride, d=d)
        for options in itertools.product(*values[6:]):       # deform, wgt_wave, patch, out_mode, sigmoid_from, groups, per_image
            set_options(d, *options)
            out.append(query(ref))
    assert all(0 <= v <= 9 for v in out)
    return "".join(map(str, out))


def probe_codes():
    return [code(*shape, **options) for _, shape, options in PROBES]


if __name__ == "__main__":
    print(" ".join(map(str, probe_codes())))
