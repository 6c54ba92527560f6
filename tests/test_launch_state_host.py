"""Source scan of the launcher state of csrc/ (CPU): the runtime queries that belong to the helpers of common.h / api.hip occur
nowhere else, and every M3D_* tuning knob is read through m3d_env_int with a literal name, once, with the default below."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "m3dssd_amd", "csrc")

# (name, default) of every knob, copied by hand from the sources BEFORE the reads moved onto m3d_env_int: a default that changes
# by accident fails here.  M3D_BF16_HALO_WK was `(e && atoi(e) == 64) ? 0 : 1`: only "is it 64" matters, 32 stands for "unset".
KNOBS = {
    "M3D_ABLATE": 0, "M3D_ABLATE_MLP": 0, "M3D_ANAB_ONLINE": 1, "M3D_BF16_C64": 1, "M3D_BF16_DCN1X1": 1, "M3D_BF16_DCN_PATCH": 1,
    "M3D_BF16_HALO": 1, "M3D_BF16_HALO_WK": 32, "M3D_BF16_WIDE": 1, "M3D_BM_THRESHOLD": 400, "M3D_CONV_WAVE_MIN": 900,
    "M3D_CONV_WAVE_SPLITK": 1, "M3D_DCN_WAVE_MIN": 1500, "M3D_FORCE_BN": 0, "M3D_L0_VALU": 0, "M3D_NMS_DIV": 0, "M3D_SPLITK": 1,
    "M3D_TE_CB64": 0, "M3D_UPLOAD_WGS": 8, "M3D_UPSAMPLE_ROWS": 1, "M3D_W44_KPAIR_MAX": 300, "M3D_W44_OCC2": 1,
    "M3D_W44_SPLIT_FILL": 0, "M3D_W44_SPLIT_NB": 1, "M3D_WAVE_VEC_EPILOGUE": 1, "M3D_WINO_SPLITK": 0, "M3D_WINO_VARIANT": 1,
    "M3D_WINO_WAVE_MIN": 800,
}


def _sources(pattern):
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, pattern)))}


def test_runtime_queries_live_only_in_the_helpers():
    hips = _sources("*.hip")
    assert len(hips) >= 26 and "api.hip" in hips
    for name, txt in hips.items():
        if name == "api.hip":
            continue
        for spelling in ("hipFuncSetAttribute(", "hipDeviceAttributeMultiprocessorCount", "hipFuncGetAttributes(", "getenv("):
            assert spelling not in txt, (name, spelling)
        assert not re.search(r"static\s+bool\s+attr", txt), name
        assert not re.search(r"static\s+int\s+[^;()]*=\s*-1\s*[;,]", txt), name          # the `static int v = -1` once-flag
    for spelling in ("hipFuncSetAttribute(", "hipDeviceAttributeMultiprocessorCount", "hipFuncGetAttributes(", "getenv("):
        assert spelling in hips["api.hip"], spelling


def test_every_knob_is_a_literal_read_once_with_its_default():
    calls = []
    for name, txt in {**_sources("*.hip"), **_sources("*.h")}.items():
        for m in re.finditer(r"\bm3d_env_int\s*\(([^()]*)\)", txt):
            arg = m.group(1).strip()
            if arg == "const char *name, int dflt":                                          # the declaration / the definition
                continue
            lit = re.fullmatch(r'"(M3D_[A-Z0-9_]+)"\s*,\s*(-?\d+)', arg)
            assert lit, (name, arg)                                                          # a string literal and a number
            calls.append((lit.group(1), int(lit.group(2))))
    assert sorted(calls) == sorted(KNOBS.items())                                            # each knob once, nothing else
