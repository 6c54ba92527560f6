"""ctypes binding of libm3dssd_hip.so, derived at import from include/m3dssd_hip.h.

The library is built in-tree (m3dssd_amd/csrc/build/) by ``build()`` -- plain hipcc for gfx950,
no torch headers.  There is NO fallback: if the shared object is missing or a symbol is absent the
import fails loudly, and every entry point that returns a non-zero status raises RuntimeError with
the library's message (the reference surfaced THError/THArgCheck the same way).

Nothing of the header is repeated here.  ``_cdecl.parse`` reads it (the dialect it accepts -- and refuses anything beyond -- is
written down in _cdecl.py) and this module turns what it returns into ctypes:

    struct      one ``ctypes.Structure`` per ``typedef struct m3d_x_y_desc``, bound as module attribute ``XYDesc`` (``m3d_`` dropped,
                every word capitalised: m3d_conv_bf16_desc -> ConvBf16Desc); fields in C order under their C names, except ``in`` ->
                ``inp`` (a Python keyword)
    scalars     int -> c_int, unsigned int -> c_uint, long long -> c_longlong, float -> c_float, double -> c_double (char, unsigned
                char and short, which the header only has behind pointers today, -> c_byte, c_ubyte, c_short)
    pointers    ``const m3d_x_desc *`` -> POINTER(XDesc), so that a wrong descriptor raises in Python; every other pointer, at any
                depth, and m3d_stream_t -> c_void_p, which takes an address, None, byref(), a ctypes array or a ctypes pointer
    returns     ``const char *`` -> c_char_p, void -> None
    constants   ``#define NAME <integer>`` and the enumerators -> CONSTANTS[NAME]

A new entry point is therefore the header and the .hip file; ``lib()`` resolves every declared name when it opens the library and
refuses one whose m3d_abi_version() is not the header's M3D_ABI_VERSION -- a stale build is the one way left to call with another
layout than the library's.
"""
import ctypes
import os
import subprocess

from . import _cdecl

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO_PATH = os.environ.get("M3D_HIP_LIB") or os.path.join(CSRC, "build", "libm3dssd_hip.so")   # (override: diagnostic builds only)
HEADER = os.path.join(os.path.dirname(_HERE), "include", "m3dssd_hip.h")

c_int, c_float, c_ll, c_void_p = ctypes.c_int, ctypes.c_float, ctypes.c_longlong, ctypes.c_void_p
P = c_void_p

with open(HEADER) as _f:
    DECLS = _cdecl.parse(_f.read())
CONSTANTS = DECLS.constants          # {"M3D_ABI_VERSION": 5, "M3D_RPN_MAX_GT": 128, ...}: the #defines and enumerators

_BY_VALUE = {"char": ctypes.c_byte, "unsigned char": ctypes.c_ubyte, "short": ctypes.c_short, "int": c_int,
             "unsigned int": ctypes.c_uint, "long long": c_ll, "float": c_float, "double": ctypes.c_double}
STRUCTS = {}                         # C name -> its ctypes.Structure, also bound below as ConvDesc, MlpDesc, ...


def _ctype(kind, returned=False):
    kind = DECLS.typedefs.get(kind, kind)
    if kind.endswith("*"):
        if kind[:-1] in STRUCTS:
            return ctypes.POINTER(STRUCTS[kind[:-1]])
        return ctypes.c_char_p if returned and kind == "char*" else c_void_p
    return None if kind == "void" else _BY_VALUE[kind]


for _name, _fields in DECLS.structs.items():
    if not _name.startswith("m3d_"):
        raise ValueError("struct `%s` of include/m3dssd_hip.h: the Python name is made from what follows `m3d_`" % _name)
    STRUCTS[_name] = type("".join(w.capitalize() for w in _name[len("m3d_"):].split("_")), (ctypes.Structure,), {
        "__doc__": "``%s`` of include/m3dssd_hip.h." % _name,
        "_fields_": [("inp" if f == "in" else f, _ctype(k)) for k, f in _fields]})
    globals()[STRUCTS[_name].__name__] = STRUCTS[_name]

# name -> (restype, argtypes), for every function the header declares
SIGNATURES = {name: (_ctype(ret, returned=True), [_ctype(k) for k, _ in params]) for name, (ret, params) in DECLS.functions.items()}

_lib = None


def build(force=False, verbose=False):
    """Compile every HIP source for gfx950 into csrc/build/libm3dssd_hip.so (make, hipcc)."""
    # (os.cpu_count() is the whole host's count, not what this process may use: at most 16 jobs, MAX_JOBS lowers it)
    jobs = min(16, int(os.environ.get("MAX_JOBS") or 0) or os.cpu_count() or 4)
    cmd = ["make", "-C", CSRC, "-j", str(jobs)] + (["-B"] if force else [])
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise RuntimeError("building libm3dssd_hip.so failed")
    return SO_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                "libm3dssd_hip.so is missing (%s): run `python -c 'import __graft_entry__ as g; g.build()'`; "
                "there is no non-HIP fallback for the M3DSSD hot path" % SO_PATH)
        # torch first: PyTorch-ROCm ships its own libamdhip64; a library dlopen()ed BEFORE torch binds the system's /opt/rocm copy and
        # the process ends up with two HIP runtimes -- kernels registered in one, the device initialised in the other ("no
        # ROCm-capable device is detected" at the first launch; seen with `python __graft_entry__.py smoke` = build() then smoke()
        # in one process, round 6).  With torch loaded the library's libamdhip64 dependency resolves to the copy torch already mapped.
        import torch  # noqa: F401
        L = ctypes.CDLL(SO_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)            # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        if L.m3d_abi_version() != CONSTANTS["M3D_ABI_VERSION"]:
            raise RuntimeError(
                "libm3dssd_hip.so (%s) has ABI version %d, include/m3dssd_hip.h declares %d: the library was built from another "
                "header, rebuild it with `python -c 'import __graft_entry__ as g; g.build()'`"
                % (SO_PATH, L.m3d_abi_version(), CONSTANTS["M3D_ABI_VERSION"]))
        _lib = L
    return _lib


def lib_source_hashes():
    """{file name: sha256[:16]} of the sources the LOADED library was built from (m3d_source_hashes)."""
    txt = lib().m3d_source_hashes().decode()
    return dict(item.split(":", 1) for item in txt.split(";") if item)


def tree_source_hashes():
    """The same record computed from the sources in the tree (what the library would carry if it were rebuilt now)."""
    import hashlib
    files = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith(".hip") or f.endswith(".h")] + [HEADER]
    return {os.path.basename(f): hashlib.sha256(open(f, "rb").read()).hexdigest()[:16] for f in files}


def check(status):
    if status != 0:
        raise RuntimeError("m3dssd_hip error %d: %s" % (status, lib().m3d_last_error().decode()))
