"""The two checks of the ctypes mirror that need no library: every prototype of include/pagan_dp.h and include/pagan_host.h
against the tables the library is declared from (abi.PROTOTYPES, host.PROTOTYPES), and every struct mirror against what a
C compiler makes of the headers.  Both return a list of problems, each starting with the name it is about; [] means agreement.
tests/test_abi_cpu.py runs them, on the tree and on planted faults."""
import ctypes as C
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADERS = ("pagan_dp.h", "pagan_host.h")

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "uint8_t": C.c_uint8, "float": C.c_float, "double": C.c_double, "long long": C.c_longlong}


def header_text(name):
    with open(os.path.join(INCLUDE, name)) as f:
        return f.read()


class Header:
    """What a header declares: structs {name: [(C type, field), ...]}, the opaque handle types, the function-pointer
    typedefs and prototypes {name: (C return type, [C parameter type, ...])}; a C type is (base, pointer depth)."""

    def __init__(self, text):
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
        text = re.sub(r'extern\s+"C"\s*\{', "", text)
        text = re.sub(r"\benum\s*\w*\s*\{[^}]*\}\s*;", "", text)
        self.structs = {}
        for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{([^}]*)\}\s*(\w+)\s*;", text):
            assert m.group(1) == m.group(3), m.group(0)
            self.structs[m.group(1)] = [f for decl in m.group(2).split(";") if decl.strip() for f in self._fields(decl)]
        text = re.sub(r"typedef\s+struct\s+\w+\s*\{[^}]*\}\s*\w+\s*;", "", text)
        self.opaque = set(re.findall(r"typedef\s+struct\s+(\w+)\s+\1\s*;", text))
        text = re.sub(r"typedef\s+struct\s+\w+\s+\w+\s*;", "", text)
        self.callbacks = set(re.findall(r"typedef\s+\w+\s*\(\s*\*\s*(\w+)\s*\)\s*\([^)]*\)\s*;", text))
        text = re.sub(r"typedef\s+\w+\s*\(\s*\*\s*\w+\s*\)\s*\([^)]*\)\s*;", "", text)
        self.prototypes = {}
        for decl in text.split(";"):
            decl = decl.replace("}", " ").strip()
            if not decl:
                continue
            m = re.fullmatch(r"(.*?)\b(pagan_\w+)\s*\((.*)\)", decl, flags=re.S)
            assert m, "not a prototype: %r" % decl
            params = m.group(3).strip()
            self.prototypes[m.group(2)] = (self._ctype(m.group(1), named=False),
                                           [] if params in ("", "void") else [self._ctype(p, named=True) for p in params.split(",")])

    @staticmethod
    def _ctype(decl, named):
        """'const int32_t *hits' -> ('int32_t', 1); an array parameter decays to a pointer."""
        depth = decl.count("*") + len(re.findall(r"\[[^\]]*\]", decl))
        words = re.sub(r"\[[^\]]*\]|\*|\bconst\b", " ", decl).split()
        base = " ".join(words[:2]) if words[:2] == ["long", "long"] else words[0]
        rest = words[len(base.split()):]
        assert len(rest) <= (1 if named else 0), "cannot read %r" % decl
        return base, depth

    @classmethod
    def _fields(cls, decl):
        """'int32_t end_x, end_y' -> [(('int32_t', 0), 'end_x'), (('int32_t', 0), 'end_y')]"""
        first, *more = decl.split(",")
        base, depth = cls._ctype(first, named=True)
        out = [((base, depth), re.findall(r"\w+", first)[-1])]
        for d in more:
            out.append(((base, d.count("*")), re.findall(r"\w+", d)[-1]))
        return out


def headers(texts=None):
    """One Header over both files (texts: {file name: text} to read instead of the tree's)."""
    texts = texts or {}
    return Header("\n".join(texts.get(h) or header_text(h) for h in HEADERS))


def to_ctypes(ctype, hdr, structs, callback):
    """The ctypes type of a C type: structs {C name: mirror class}, callback the type of a function-pointer typedef."""
    base, depth = ctype
    if base == "void":
        t = None if depth == 0 else C.c_void_p
        depth = max(depth - 1, 0)
    elif base == "char" and depth:
        t, depth = C.c_char_p, depth - 1
    elif base in hdr.opaque:
        assert depth, "an opaque %s by value" % base
        t, depth = C.c_void_p, depth - 1
    elif base in hdr.callbacks:
        t = callback
    elif base in SCALARS:
        t = SCALARS[base]
    else:
        t = structs[base]
    for _ in range(depth):
        t = C.POINTER(t)
    return t


def kind(t):
    """What makes two ctypes types the same to a call: c_int is c_int32 here, c_longlong is c_int64."""
    if t is None:
        return "void"
    code = getattr(t, "_type_", None)
    if isinstance(code, str):
        if code in "zZP?":
            return code
        return ("float" if code in "fdg" else "signed" if code.islower() else "unsigned", C.sizeof(t))
    if code is not None and issubclass(t, C._Pointer):
        return ("pointer", kind(code))
    return t            # a Structure or a CFUNCTYPE: the class itself


def compare_prototypes(hdr, table, structs, callback):
    """hdr's prototypes against table {name: (restype, (argtypes...))}."""
    problems = []
    for name in sorted(set(hdr.prototypes) - set(table)):
        problems.append("%s: declared in the headers, missing from the tables" % name)
    for name in sorted(set(table) - set(hdr.prototypes)):
        problems.append("%s: in the tables, not declared in the headers" % name)
    for name in sorted(set(table) & set(hdr.prototypes)):
        ret, params = hdr.prototypes[name]
        restype, argtypes = table[name]
        try:
            want = [to_ctypes(ret, hdr, structs, callback)] + [to_ctypes(p, hdr, structs, callback) for p in params]
        except KeyError as e:
            problems.append("%s: type %s has no mirror" % (name, e))
            continue
        if len(params) != len(argtypes):
            problems.append("%s: %d arguments in the header, %d in the table" % (name, len(params), len(argtypes)))
            continue
        for k, (w, g) in enumerate(zip(want, [restype] + list(argtypes))):
            if kind(w) != kind(g):
                problems.append("%s: %s is %s in the header, %s in the table" %
                                (name, "return value" if k == 0 else "argument %d" % k, getattr(w, "__name__", w), getattr(g, "__name__", g)))
    return problems


def compiler():
    for cand in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang"):
        path = shutil.which(cand)
        if path:
            return path
    return None


C_NAMES = {("signed", 4): "int32_t", ("unsigned", 4): "uint32_t", ("signed", 8): "int64_t", ("unsigned", 8): "uint64_t",
           ("unsigned", 1): "uint8_t", ("float", 4): "float", ("float", 8): "double"}


def layout_source(structs):
    """A C11 translation unit that compiles if and only if every mirror of structs {C name: mirror class} has the size, the
    field offsets and the field types of the struct the headers declare.  Every assertion's message starts with `LAYOUT name`."""
    lines = ["#include <stddef.h>", '#include "pagan_host.h"']
    for cname, cls in structs.items():
        lines.append('_Static_assert(sizeof(%s) == %d, "LAYOUT %s: sizeof");' % (cname, C.sizeof(cls), cname))
        for field, t in cls._fields_:
            what = "%s.%s" % (cname, field)
            lines.append('_Static_assert(offsetof(%s, %s) == %d, "LAYOUT %s: offsetof");' % (cname, field, getattr(cls, field).offset, what))
            k = kind(t)
            if k in C_NAMES:
                lines.append('_Static_assert(_Generic(((%s *)0)->%s, %s: 1, default: 0), "LAYOUT %s: not %s");' %
                             (cname, field, C_NAMES[k], what, C_NAMES[k]))
            else:
                lines.append('_Static_assert(sizeof(((%s *)0)->%s) == %d, "LAYOUT %s: sizeof");' % (cname, field, C.sizeof(t), what))
    return "\n".join(lines) + "\n"


def compare_structs(hdr, structs, cc, workdir):
    """Every struct with a body in hdr against structs {C name: mirror class}: a mirror for each, the same field names in
    the same order, and -- by the compiler cc over layout_source -- the same sizes, offsets and types."""
    problems = ["%s: a struct of the headers without a mirror" % s for s in sorted(set(hdr.structs) - set(structs))]
    problems += ["%s: a mirror of no struct in the headers" % s for s in sorted(set(structs) - set(hdr.structs))]
    known = {s: cls for s, cls in structs.items() if s in hdr.structs}
    for cname, cls in known.items():
        want, got = [f for _, f in hdr.structs[cname]], [f for f, _ in cls._fields_]
        if want != got:
            odd = sorted(set(want) ^ set(got)) or [w for w, g in zip(want, got) if w != g]
            problems.append("%s: fields %s differ from the header's (%s)" % (cname, ", ".join(odd), ", ".join(want)))
    src = os.path.join(str(workdir), "layout.c")
    with open(src, "w") as f:
        f.write(layout_source(known))
    run = subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", INCLUDE, src], capture_output=True, text=True)
    failed = sorted(set(re.findall(r"LAYOUT ([\w.]+: [\w ]+)", run.stderr)))
    problems += failed
    if run.returncode != 0 and not failed:
        problems.append("layout.c: the compiler failed: %s" % run.stderr.strip()[-400:])
    return problems
