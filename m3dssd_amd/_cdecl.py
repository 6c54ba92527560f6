"""Declaration reader for the dialect of C that include/m3dssd_hip.h is written in (plain Python, no C front end).

``parse(text)`` returns a ``Decls`` of four dicts in declaration order (the #defines stand before the enumerators):

    constants  {NAME: int}                      ``#define NAME <integer>`` and the enumerators of anonymous enums
    typedefs   {NAME: type}                     ``typedef void *m3d_stream_t;``
    structs    {NAME: [(type, field), ...]}     ``typedef struct NAME { ... } NAME;`` with flat fields
    functions  {NAME: (type, [(type, parameter), ...])}

A type is its canonical spelling without ``const``: a base type (BASE_TYPES; a bare ``unsigned`` reads as ``unsigned int``), a
struct name or a typedef name, then one ``*`` per pointer level -- ``"int"``, ``"long long"``, ``"float*"``, ``"void**"``,
``"m3d_conv_desc*"``, ``"m3d_stream_t"``.  ``void`` without a pointer is a return type only; a struct is only ever pointed to.

Accepted: ``/* */`` and ``//`` comments (removed first: they hold code-like text); preprocessor lines (dropped, except that
``#define NAME <integer>`` is a constant; a ``#define`` with any other value is refused); one ``extern "C" { }`` wrapper; the
typedef, enum (explicit values, or the previous one + 1), struct (several declarators per declaration) and prototype (every
parameter named, or ``(void)``) forms above.  Everything else -- an unknown type word, an array declarator, a function pointer, a
bit-field, a nested struct, an unnamed parameter, a name declared twice, any other statement -- raises ValueError naming the
declaration.  Nothing is skipped: a declaration the binding does not know about is a wrong call waiting to happen.
"""
import collections
import re

BASE_TYPES = ("void", "char", "unsigned char", "short", "int", "unsigned int", "long long", "float", "double")

Decls = collections.namedtuple("Decls", "constants typedefs structs functions")

_NAME = r"[A-Za-z_]\w*"


def _refuse(what, decl):
    raise ValueError("%s in `%s`" % (what, " ".join(decl.split())))


def _integer(text, decl):
    if not re.fullmatch(r"[-+]?(0[xX][0-9a-fA-F]+|\d+)", text):
        _refuse("`%s` is not an integer constant" % text, decl)
    return int(text, 0)


def _declarators(text, known, decl, void_ok=False):
    """``const float *scale, *shift`` -> [("float*", "scale"), ("float*", "shift")]; `known`: the type names so far."""
    out, base = [], None
    for part in text.split(","):
        odd = re.search(r"[^\w\s*]|\b\d", part)
        if odd:
            _refuse("`%s` is not part of a plain declarator (no arrays, function pointers, bit-fields, initialisers or nested "
                    "structs)" % odd.group(), decl)
        tokens = [t for t in re.findall(r"\w+|\*", part) if t != "const"]
        first = tokens.index("*") if "*" in tokens else max(len(tokens) - 1, 0)       # where the declarator starts
        words, rest = " ".join(tokens[:first]), tokens[first:]
        if base is None:
            base = "unsigned int" if words == "unsigned" else words
            if base not in known:
                _refuse("unknown type `%s`, or a declarator without a name," % base, decl)
        elif words:
            _refuse("`%s` in front of a later declarator" % words, decl)
        if not rest or rest.count("*") != len(rest) - 1 or rest[-1] == "*" or rest[-1] in known or rest[-1] in ("unsigned", "long"):
            _refuse("a declarator without a name", decl)
        depth = len(rest) - 1
        if depth == 0 and (isinstance(known[base], list) or base == "void" and not void_ok):
            _refuse("`%s` by value" % base, decl)
        out.append((base + "*" * depth, rest[-1]))
    return out


def _declarator(text, known, decl, void_ok=False):
    found = _declarators(text, known, decl, void_ok)
    if len(found) != 1:
        _refuse("more than one declarator", decl)
    return found[0]


def _statements(text):
    """The pieces between the semicolons that stand outside braces."""
    depth, start = 0, 0
    for m in re.finditer(r"[{};]", text):
        depth += (m.group() == "{") - (m.group() == "}")
        if depth < 0:
            _refuse("`}` without its `{`", text[start:m.end()])
        if m.group() == ";" and depth == 0:
            yield text[start:m.start()].strip()
            start = m.end()
    if text[start:].strip():
        _refuse("no `;` at the end", text[start:])


def parse(text):
    out = Decls({}, {}, {}, {})
    known = dict.fromkeys(BASE_TYPES)         # type name -> None (base type), its type (typedef) or its field list (struct)

    def add(table, name, value, decl):
        if any(name in t for t in out) or name in known:
            _refuse("`%s` is declared twice" % name, decl)
        table[name] = value
        if table is out.typedefs or table is out.structs:
            known[name] = value

    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    lines = text.split("\n")
    for i, line in enumerate(lines):
        if line.lstrip().startswith("#"):
            m = re.fullmatch(r"\s*#\s*define\s+(%s)(\s.*)?" % _NAME, line)
            if line.rstrip().endswith("\\") or re.match(r"\s*#\s*define\b", line) and not m:
                _refuse("a macro with parameters or a continued line", line)
            if m and (m.group(2) or "").strip():
                add(out.constants, m.group(1), _integer(m.group(2).strip(), line), line)
            lines[i] = ""
    text, wrappers = re.subn(r'extern\s+"C"\s*\{', " ", "\n".join(lines))
    if wrappers:
        if wrappers > 1 or not text.rstrip().endswith("}"):
            _refuse("more than one wrapper, or one that does not close at the end,", 'extern "C" {')
        text = text.rstrip()[:-1]

    for decl in _statements(text):
        struct = re.fullmatch(r"typedef\s+struct\s+(%s)\s*\{(.*)\}\s*(%s)" % (_NAME, _NAME), decl, flags=re.S)
        enum = re.fullmatch(r"enum\s*\{(.*)\}", decl, flags=re.S)
        proto = re.fullmatch(r"([^()]*)\((.*)\)", decl, flags=re.S)
        if struct:
            tag, body, name = struct.groups()
            if tag != name or not body.rstrip().endswith(";"):
                _refuse("tag and typedef name differ, or the last field has no `;`,", decl)
            fields = []
            add(out.structs, name, fields, decl)
            for field in body.split(";")[:-1]:
                fields += _declarators(field, known, decl)
            if len(set(n for _, n in fields)) != len(fields):
                _refuse("a field name is used twice", decl)
        elif enum:
            value, items = -1, enum.group(1).split(",")
            for item in items[:-1] if not items[-1].strip() else items:       # (C99 allows one trailing comma)
                name, eq, number = (s.strip() for s in item.partition("="))
                if not re.fullmatch(_NAME, name):
                    _refuse("`%s` is not an enumerator" % name, decl)
                value = _integer(number, decl) if eq else value + 1
                add(out.constants, name, value, decl)
        elif "{" in decl or "}" in decl:
            _refuse("braces other than `typedef struct X { ... } X;` and an anonymous `enum { ... };`", decl)
        elif re.match(r"typedef\b", decl):
            kind, name = _declarator(decl[len("typedef"):], known, decl)
            add(out.typedefs, name, kind, decl)
        elif proto:
            ret, name = _declarator(proto.group(1), known, decl, void_ok=True)
            params = [] if proto.group(2).strip() == "void" else [p for text in proto.group(2).split(",")
                                                                  for p in _declarators(text, known, decl)]
            if len(set(n for _, n in params)) != len(params):
                _refuse("a parameter name is used twice", decl)
            add(out.functions, name, (ret, params), decl)
        else:
            _refuse("neither a typedef, an enum, a struct nor a function prototype", decl)
    return out
