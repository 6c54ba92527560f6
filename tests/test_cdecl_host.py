"""CPU checks of the declaration reader (m3dssd_amd/_cdecl.py) that the ctypes binding is derived with: the exact result on a
synthetic header that uses every accepted form, a ValueError for every refused one, and the layout of the derived structures
against what a C compiler makes of the real header."""
import ctypes
import os
import shutil
import subprocess

import pytest

from m3dssd_amd import _cdecl, _hip

SYNTHETIC = """
/* a block comment with code in it: int foo(int x); typedef struct bad { int a[3]; } bad;
 * #define NOT_A_CONSTANT 7 */
#ifndef SYNTH_H
#define SYNTH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void *handle_t;   // a line comment: int bar(float);
#define ROWS 12
  #  define MASK 0x10
enum {
    E_OK = 0,
    E_BAD = -3,     /* explicit, negative */
    E_NEXT,         /* implicit: -2 */
    E_AFTER,
    E_TEN = 10,
    E_ELEVEN,
};
enum { LONE };
typedef struct desc_a {
    const float *in;          /* [n] */
    int N, H, W;
    const float *scale, *shift;
    long long stride;
    void *out; int out_cs;
    const void *const *slots;
    float *const tail;
    unsigned int mask; unsigned flags;
    unsigned char tag; short s; char c; double d;
} desc_a;
typedef struct desc_b { void **pp, *p; float f; } desc_b;
const char *last_error(void);
void reset( void );
int run(const desc_a *d, desc_b *e, handle_t stream);
long long bytes(int n, long long m, unsigned int flags, float f, double d);
int mixed(const void *const *src, void **dst, const unsigned char *u8, short *s16, const double *x /* [n] */,
          const char *name, unsigned k);
#ifdef __cplusplus
}
#endif
#endif /* SYNTH_H */
"""


def test_reader_parses_every_accepted_form_exactly():
    d = _cdecl.parse(SYNTHETIC)
    assert d.constants == {"ROWS": 12, "MASK": 16, "E_OK": 0, "E_BAD": -3, "E_NEXT": -2, "E_AFTER": -1, "E_TEN": 10, "E_ELEVEN": 11,
                           "LONE": 0}
    assert d.typedefs == {"handle_t": "void*"}
    assert list(d.structs) == ["desc_a", "desc_b"]
    assert d.structs["desc_a"] == [
        ("float*", "in"), ("int", "N"), ("int", "H"), ("int", "W"), ("float*", "scale"), ("float*", "shift"),
        ("long long", "stride"), ("void*", "out"), ("int", "out_cs"), ("void**", "slots"), ("float*", "tail"),
        ("unsigned int", "mask"), ("unsigned int", "flags"), ("unsigned char", "tag"), ("short", "s"), ("char", "c"), ("double", "d")]
    assert d.structs["desc_b"] == [("void**", "pp"), ("void*", "p"), ("float", "f")]
    assert list(d.functions) == ["last_error", "reset", "run", "bytes", "mixed"]
    assert d.functions["last_error"] == ("char*", [])
    assert d.functions["reset"] == ("void", [])
    assert d.functions["run"] == ("int", [("desc_a*", "d"), ("desc_b*", "e"), ("handle_t", "stream")])
    assert d.functions["bytes"] == ("long long", [("int", "n"), ("long long", "m"), ("unsigned int", "flags"), ("float", "f"),
                                                  ("double", "d")])
    assert d.functions["mixed"] == ("int", [("void**", "src"), ("void**", "dst"), ("unsigned char*", "u8"), ("short*", "s16"),
                                            ("double*", "x"), ("char*", "name"), ("unsigned int", "k")])


REFUSED = {
    "unknown type word": "int f(size_t n);",
    "unknown type word in a struct": "typedef struct s { uint32_t a; } s;",
    "unknown return type": "long f(int n);",
    "array field": "typedef struct s { float m[4]; } s;",
    "array parameter": "int f(float m[4]);",
    "function-pointer parameter": "int f(void (*cb)(int x), int n);",
    "unnamed parameter": "int f(int, float *p);",
    "unnamed pointer parameter": "int f(int n, const float *);",
    "unnamed typedef parameter": "typedef void *h_t; int f(int n, h_t);",
    "nested struct": "typedef struct s { int a; struct { int b; } inner; } s;",
    "bit-field": "typedef struct s { int a : 3; } s;",
    "struct by value": "typedef struct s { int a; } s; int f(s d);",
    "void parameter by value": "int f(void v);",
    "named enum": "enum colour { RED };",
    "enumerator that is an expression": "enum { A = 1 << 2 };",
    "macro with a value that is no integer": "#define SCALE 1.5f",
    "macro with parameters": "#define SQ(x) ((x) * (x))",
    "global variable with an initialiser": "int counter = 0;",
    "plain struct definition": "struct s { int a; };",
    "struct whose names differ": "typedef struct s { int a; } t;",
    "name declared twice": "int f(int a); int f(int a);",
    "missing semicolon": "int f(int a)",
    "function definition": "int f(int a) { return a; }",
}


@pytest.mark.parametrize("form", sorted(REFUSED))
def test_reader_refuses(form):
    with pytest.raises(ValueError) as e:
        _cdecl.parse(REFUSED[form])
    assert "`" in str(e.value)          # the message quotes the declaration


def _compiler():
    for cc in (os.environ.get("CC"), "cc", "/opt/rocm/lib/llvm/bin/clang", "/opt/rocm/llvm/bin/clang"):
        if cc and shutil.which(cc.split()[0]):
            return cc.split()
    return None


def test_structure_layout_matches_the_c_compiler(tmp_path):
    """sizeof, offsetof and the size of every field of every struct, as a C99 compiler lays out the header, against the derived
    ctypes classes: the one check that does not go through the reader's idea of C."""
    cc = _compiler()
    if cc is None:
        pytest.skip("no C compiler ($CC, cc, ROCm's clang)")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "m3dssd_hip.h"', "int main(void) {"]
    for name, fields in _hip.DECLS.structs.items():
        lines.append('    printf("%s sizeof %%zu\\n", sizeof(%s));' % (name, name))
        for _, f in fields:
            lines.append('    printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (name, f, name, f, name, f))
    (tmp_path / "layout.c").write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.run(cc + ["-std=c99", "-I", os.path.dirname(_hip.HEADER), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")],
                   check=True)
    got = subprocess.run([str(tmp_path / "layout")], check=True, stdout=subprocess.PIPE, text=True).stdout.split("\n")[:-1]
    want = []
    for name, fields in _hip.DECLS.structs.items():
        cls = _hip.STRUCTS[name]
        want.append("%s sizeof %d" % (name, ctypes.sizeof(cls)))
        for _, f in fields:
            member = getattr(cls, "inp" if f == "in" else f)
            want.append("%s %s %d %d" % (name, f, member.offset, member.size))
    assert len(_hip.DECLS.structs) == 8 and len(want) == 8 + sum(len(f) for f in _hip.DECLS.structs.values())
    assert got == want
    assert "m3d_conv_desc sizeof 184" in got and "m3d_conv_desc wgt_img_stride 40 8" in got
    assert "m3d_conv_bf16_desc wgt_wave 224 8" in got
