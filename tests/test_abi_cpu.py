"""CPU, no library: the ctypes mirror against the headers.  Every prototype of include/pagan_dp.h and include/pagan_host.h
against the tables the library is declared from, every struct mirror against what a C compiler makes of the headers, the same
two comparisons on planted faults (a check that cannot fail proves nothing), and that loading the library declares both tables."""
import ctypes as C
import re

import pytest

import abi_check
import pagan2_msa_amd as pg
from pagan2_msa_amd import abi, host


def tables():
    return dict(abi.PROTOTYPES, **host.PROTOTYPES)


def prototype_problems(texts=None):
    return abi_check.compare_prototypes(abi_check.headers(texts), tables(), host.STRUCTS, host.BATCH_FN)


def struct_problems(tmp_path, structs=None):
    cc = abi_check.compiler()
    if cc is None:
        pytest.skip("no C compiler (cc, gcc, clang, ROCm's clang)")
    return abi_check.compare_structs(abi_check.headers(), structs or host.STRUCTS, cc, tmp_path)


# ---- the tree as it stands ----------------------------------------------------------------------------------------------------

def test_the_parser_reads_what_the_headers_hold():
    hdr = abi_check.headers()
    assert {"pagan_batch", "pagan_fb", "pagan_msa", "pagan_hgraph"} <= hdr.opaque and not hdr.opaque & set(hdr.structs)
    assert hdr.callbacks == {"pagan_batch_fn"}
    assert hdr.prototypes["pagan_dp_version"] == (("char", 1), [])
    assert hdr.prototypes["pagan_batch_last_ms"] == (("int", 0), [("pagan_batch", 1), ("double", 1)])          # double ms[2] decays
    assert hdr.prototypes["pagan_msa_create"][1][1] == ("char", 2) and hdr.prototypes["pagan_parents_device_calls"][0] == ("long long", 0)
    assert [f for _, f in hdr.structs["pagan_result"]][3:5] == ["end_x", "end_y"]                              # int32_t end_x, end_y;
    # every prototype of either file is found by the plain reading test_library_exports_every_declared_symbol makes as well
    text = "".join(re.sub(r"/\*.*?\*/", "", abi_check.header_text(h), flags=re.S) for h in abi_check.HEADERS)
    assert set(hdr.prototypes) == set(re.findall(r"\b(pagan_[a-z0-9_]+)\s*\(", text))


def test_every_prototype_agrees_with_its_table_entry():
    assert not set(abi.PROTOTYPES) & set(host.PROTOTYPES)
    hdr = abi_check.headers()
    assert set(hdr.prototypes) == set(tables()) and len(tables()) == len(abi.PROTOTYPES) + len(host.PROTOTYPES)
    for name, (ret, params) in hdr.prototypes.items():
        assert len(params) == len(tables()[name][1]), name
    assert prototype_problems() == []
    # a table belongs to its header
    for name, table in zip(abi_check.HEADERS, (abi.PROTOTYPES, host.PROTOTYPES)):
        assert list(abi_check.Header(abi_check.header_text(name)).prototypes) == list(table), name


def test_the_name_lists_are_the_tables():
    assert abi.EXPORTED == list(abi.PROTOTYPES) and host.HOST_EXPORTED == list(host.PROTOTYPES)


def test_every_struct_mirror_has_the_compilers_layout(tmp_path):
    hdr = abi_check.headers()
    assert set(hdr.structs) == set(host.STRUCTS)              # a new struct cannot be forgotten
    assert set(abi.STRUCTS) == set(abi_check.Header(abi_check.header_text("pagan_dp.h")).structs)
    assert struct_problems(tmp_path) == []
    src = abi_check.layout_source(host.STRUCTS)
    assert src.count("sizeof(pagan_") == len(host.STRUCTS) and src.count("offsetof(") == sum(len(c._fields_) for c in host.STRUCTS.values())
    assert "_Generic(((pagan_result *)0)->score, double: 1, default: 0)" in src and "sizeof(((pagan_result *)0)->cols) == %d" % C.sizeof(C.c_void_p) in src


# ---- the checks can fail ------------------------------------------------------------------------------------------------------

def planted(name, old, new):
    text = abi_check.header_text(name)
    assert text.count(old) == 1, old
    return {name: text.replace(old, new)}


@pytest.mark.parametrize("texts, name, what", [
    (planted("pagan_dp.h", "int pagan_dp_select_device(int32_t device);", "int pagan_dp_select_device(void);"),
     "pagan_dp_select_device", "0 arguments in the header, 1 in the table"),
    (planted("pagan_dp.h", "int32_t k, void *dst, int64_t bytes);", "int32_t k, void *dst, int32_t bytes);"),
     "pagan_batch_debug_trace", "argument 4"),
    (planted("pagan_dp.h", "int64_t pagan_batch_cells(", "int32_t pagan_batch_cells("), "pagan_batch_cells", "return value"),
    (planted("pagan_host.h", "void pagan_msa_destroy(pagan_msa *m);", "void pagan_msa_destroy(pagan_msa *m);\nint pagan_msa_new(pagan_msa *m);"),
     "pagan_msa_new", "missing from the tables"),
], ids=["argument removed", "int64 to int32", "return type", "function added"])
def test_a_fault_in_a_header_is_reported_by_name(texts, name, what):
    problems = prototype_problems(texts)
    assert len(problems) == 1 and problems[0].startswith(name + ": ") and what in problems[0], problems


def faulty(cname, change):
    fields = list(host.STRUCTS[cname]._fields_)
    change(fields)
    return dict(host.STRUCTS, **{cname: type("Faulty", (C.Structure,), {"_fields_": fields})})


def swap_end_x_end_y(fields):
    fields[3], fields[4] = fields[4], fields[3]
    assert [f for f, _ in fields[3:5]] == ["end_y", "end_x"]


def level_as_float(fields):
    assert fields[3] == ("level", C.c_int32)
    fields[3] = ("level", C.c_float)


def drop_last(fields):
    assert fields.pop()[0] == "n_forced_gaps"           # (the struct's size stays: the tail padding takes the four bytes)


@pytest.mark.parametrize("cname, change, want", [
    ("pagan_result", swap_end_x_end_y, ["pagan_result.end_x: offsetof", "pagan_result.end_y: offsetof", "pagan_result: fields end_x, end_y differ"]),
    ("pagan_node_info", level_as_float, ["pagan_node_info.level: not float"]),
    ("pagan_node_info", drop_last, ["pagan_node_info: fields n_forced_gaps differ"]),
], ids=["two fields swapped", "int32 to float", "trailing field dropped"])
def test_a_fault_in_a_mirror_is_reported_by_name(tmp_path, cname, change, want):
    problems = struct_problems(tmp_path, faulty(cname, change))
    assert len(problems) == len(want), problems
    for w in want:
        assert any(p.startswith(w) for p in problems), (w, problems)


def test_a_struct_without_a_mirror_is_reported(tmp_path):
    structs = dict(host.STRUCTS)
    del structs["pagan_anc_info"]
    assert struct_problems(tmp_path, structs) == ["pagan_anc_info: a struct of the headers without a mirror"]
    # ... and with it the prototypes that take one
    hdr = abi_check.headers()
    problems = abi_check.compare_prototypes(hdr, tables(), structs, host.BATCH_FN)
    assert sorted(p.split(":")[0] for p in problems) == ["pagan_anc_reconstruct", "pagan_msa_ancestral"]


# ---- declared at load ---------------------------------------------------------------------------------------------------------

class StandIn:
    """Attribute access creates a blank function object, as a CDLL does."""

    def __getattr__(self, name):
        fn = type("Fn", (), {})()
        setattr(self, name, fn)
        return fn


def test_loading_the_library_declares_both_tables(tmp_path, monkeypatch):
    standin = StandIn()
    path = tmp_path / "libpagan_dp.so"
    path.write_bytes(b"")
    monkeypatch.setattr(pg, "_lib", None)
    monkeypatch.setattr(pg, "LIB_PATH", str(path))
    monkeypatch.setattr(C, "CDLL", lambda p: standin if p == str(path) else None)
    assert pg.lib() is standin and host._lib() is pg.lib()
    assert set(vars(standin)) == set(tables())
    for name, (restype, argtypes) in tables().items():
        fn = getattr(standin, name)
        assert fn.argtypes == list(argtypes) and fn.restype is restype, name
    assert standin.pagan_msa_node_graph.restype is C.c_void_p and standin.pagan_hgraph_leaf.restype is C.c_void_p
    assert not hasattr(host, "_declared")
