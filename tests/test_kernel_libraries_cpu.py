"""The table of kernel libraries (geometry_rl_amd/hip.py ``LIBRARIES``) without a GPU.  The two satellites -- libgrl_attention.so
(csrc/grl_attention.h: the EMPN key / query attention kernels) and libgrl_transformer.so (csrc/grl_transformer.h: the transformer baseline
actor's kernels) -- parse with the binder of include/grl_hip.h, export exactly what their headers declare, carry the tree's source hash,
and neither their names nor their objects reach libgrl_hip.so, whose export list stays the main header's.  One index sends every entry
point's name to its library; a library is opened by the first call into it, not before."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

from geometry_rl_amd import hip
from test_abi_and_host import ROOT, declared_symbols

RECORDS = {l.name: l for l in hip.LIBRARIES}
NAMES = {"attention": ["grl_attention_blocks", "grl_edge_attend_bwd", "grl_edge_attend_fwd", "grl_edge_logits_bwd", "grl_edge_logits_fwd",
                       "grl_kq_bwd_blocks", "grl_kq_partial_size", "grl_kq_project_bwd", "grl_kq_project_fwd"],
         "transformer": ["grl_postfc_head_blocks", "grl_postfc_head_bwd", "grl_postfc_head_fwd", "grl_postfc_head_partial_size",
                         "grl_transformer_blocks", "grl_transformer_bwd", "grl_transformer_fwd", "grl_transformer_group_rows",
                         "grl_transformer_partial_size", "grl_transformer_ws_row"]}
A_QUERY = {"attention": "grl_kq_partial_size", "transformer": "grl_transformer_ws_row"}


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if l.strip())


def test_the_table_holds_the_three_libraries():
    assert [(l.name, l.file, os.path.relpath(l.paths()[1], ROOT)) for l in hip.LIBRARIES] == [
        ("main", "libgrl_hip.so", "include/grl_hip.h"), ("attention", "libgrl_attention.so", "geometry_rl_amd/csrc/grl_attention.h"),
        ("transformer", "libgrl_transformer.so", "geometry_rl_amd/csrc/grl_transformer.h")]
    assert RECORDS["main"].path == hip.LIB_PATH and RECORDS["main"].sources == hip.SOURCES and RECORDS["main"].variants == hip.VARIANTS
    assert RECORDS["attention"].sources == ["attention_ops.hip"] and RECORDS["transformer"].sources == ["transformer_ops.hip"]
    assert not RECORDS["attention"].variants and not RECORDS["transformer"].variants
    # every source file belongs to exactly one record
    owned = [s for l in hip.LIBRARIES for s in l.sources]
    assert sorted(owned) == sorted(f for f in os.listdir(hip.CSRC) if f.endswith(".hip")) and len(set(owned)) == len(owned)
    assert all(s in l.sources for l in hip.LIBRARIES for s, _, _ in l.variants)
    # another checkout: the same files under its root
    assert RECORDS["attention"].paths("/x") == ("/x/geometry_rl_amd/libgrl_attention.so", "/x/geometry_rl_amd/csrc/grl_attention.h")
    assert RECORDS["main"].paths("/x") == ("/x/geometry_rl_amd/libgrl_hip.so", "/x/include/grl_hip.h")


@pytest.mark.parametrize("name", list(NAMES))
def test_header_parses_and_library_exports_exactly_its_names(name):
    hip.build(verbose=False)
    path, header = RECORDS[name].paths()
    decls = hip.parse_header(open(header).read())
    assert sorted(decls) == NAMES[name]
    for entry, params in decls.items():   # launches end in the stream, the shape / size queries take none
        assert (params[-1:] or [("",)])[-1][0] == ("hipStream_t" if entry.endswith(("_fwd", "_bwd")) else "int" if params else "")
    assert _exported(path) == NAMES[name]
    assert hip.embedded_hash(path) == hip.source_hash() == hip.embedded_hash(hip.LIB_PATH)
    assert not set(NAMES[name]) & set(_exported(hip.LIB_PATH)) and not set(NAMES[name]) & set(declared_symbols())


def test_attention_host_queries():
    hip.build(verbose=False)
    lib = ctypes.CDLL(RECORDS["attention"].path)   # host-only queries are callable without a GPU
    assert lib.grl_kq_partial_size() == 2 * 128 * 64 + 2 * 128
    assert lib.grl_kq_bwd_blocks(0) == 1 and lib.grl_kq_bwd_blocks(65) == 2 and lib.grl_kq_bwd_blocks(10 ** 8) == 512
    assert lib.grl_attention_blocks(0) == 1 and lib.grl_attention_blocks(5) == 2 and lib.grl_attention_blocks(10 ** 8) == 2048


def test_transformer_host_queries_and_the_abi_number():
    """The kernels are a library of their own, libgrl_transformer.so, declared in geometry_rl_amd/csrc/grl_transformer.h (as the EMPN
    attention kernels are): include/grl_hip.h keeps its declarations and libgrl_hip.so its export list, ABI 216 names the addition."""
    hip.build(verbose=False)
    text = open(os.path.join(ROOT, "include", "grl_hip.h")).read()
    assert hip.ABI_VERSION == 216 and int(re.search(r"#define GRL_HIP_VERSION (\d+)", text).group(1)) == 216
    lib = ctypes.CDLL(RECORDS["transformer"].path)   # host-only queries are callable without a GPU
    assert lib.grl_transformer_partial_size(15) == 54656 + 64 * 15 and lib.grl_transformer_partial_size(65) == -2
    assert lib.grl_transformer_ws_row() == 320 and lib.grl_postfc_head_partial_size() == 2080
    # one sample per group until the batch exceeds the 256 workgroups, then as many as keep a group within 256 rows
    assert [lib.grl_transformer_group_rows(B, 33) for B in (1, 256, 257, 4096)] == [33, 33, 66, 231]
    assert [lib.grl_transformer_blocks(B, 33) for B in (1, 256, 257, 4096)] == [1, 256, 129, 256]
    assert lib.grl_transformer_blocks(4, 257) == -2 and lib.grl_postfc_head_blocks(0) == 1 and lib.grl_postfc_head_blocks(10 ** 6) == 256


@pytest.mark.parametrize("name", list(NAMES))
def test_missing_library_is_an_error_at_the_first_call_into_it(name, monkeypatch, tmp_path):
    hip.build(verbose=False)
    monkeypatch.setattr(RECORDS[name], "path", str(tmp_path / "missing.so"))
    monkeypatch.setattr(RECORDS[name], "entries", None)
    assert hip.query("grl_edge_partial_size") == 64 * 14 + 64 + 4096 + 64 + 4096   # the main library does not need it
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        hip.query(A_QUERY[name])


def test_undeclared_name_is_refused():
    hip.build(verbose=False)
    assert "grl_version" not in RECORDS["attention"].load() and "grl_version" in RECORDS["main"].load()
    nowhere = "grl_declared_nowhere"
    with pytest.raises(AttributeError, match="is not declared"):
        hip.query(nowhere)
    with pytest.raises(AttributeError, match="is not declared"):
        hip.call(nowhere, 1, stream=ctypes.c_void_p(0))


def test_every_name_has_exactly_one_library():
    decls = {l.name: hip.parse_header(open(l.paths()[1]).read()) for l in hip.LIBRARIES}
    index = hip.entry_index((l, open(l.paths()[1]).read()) for l in hip.LIBRARIES)
    assert len(index) == sum(len(d) for d in decls.values()) == 138 + 9 + 10
    for l in hip.LIBRARIES:
        assert all(index[entry] is l for entry in decls[l.name])
    one = "typedef void* hipStream_t;\nint grl_a(int n);\nint grl_b(const float* x, hipStream_t stream);\n"
    assert hip.entry_index([("p", one), ("q", "int grl_c(void);\n")]) == {"grl_a": "p", "grl_b": "p", "grl_c": "q"}
    with pytest.raises(ValueError, match="grl_b is declared by two headers"):
        hip.entry_index([("p", one), ("q", "int grl_c(void);\nint grl_b(int n);\n")])


def test_a_library_is_opened_by_the_first_call_into_it():
    """In a fresh process: a query of the main library opens libgrl_hip.so alone, one of the attention library opens that as well, and
    libgrl_transformer.so is still not mapped."""
    hip.build(verbose=False)
    code = ("from geometry_rl_amd import hip\n"
            "mapped = lambda: [l.name for l in hip.LIBRARIES if l.file in open('/proc/self/maps').read()]\n"
            "print(mapped())\n"
            "assert hip.query('grl_edge_partial_size') > 0\n"
            "print(mapped())\n"
            "assert hip.query('grl_kq_partial_size') > 0\n"
            "print(mapped())\n")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout.splitlines() == ["[]", "['main']", "['main', 'attention']"]


def test_build_info_lists_every_library():
    hip.build(verbose=False)
    info = json.load(open(os.path.join(ROOT, "BUILD_INFO.json")))
    assert sorted(info["libraries"]) == ["attention", "main", "transformer"] and info["objects_total"] == 12 + 6 + 1 + 1 + 1
    for name, entry in info["libraries"].items():
        path = os.path.join(ROOT, entry["path"])
        assert path == RECORDS[name].path and entry["bytes"] == os.path.getsize(path)
        assert entry["source_hash"] == hip.source_hash() == hip.embedded_hash(path)
    main = info["libraries"]["main"]
    assert (info["library"], info["library_bytes"], info["library_source_hash"]) == (main["path"], main["bytes"], main["source_hash"])
