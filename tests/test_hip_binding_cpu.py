"""The typed C-ABI boundary (geometry_rl_amd/hip.py): include/grl_hip.h parses completely, and the binder marshals every parameter type of
the header's vocabulary exactly -- checked without a GPU on a small echo library that is built here and bound by the same binder."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from geometry_rl_amd import hip
from test_abi_and_host import ROOT, declared_symbols

HEADER = open(os.path.join(ROOT, "include", "grl_hip.h")).read()


# ---- 1. the header ---------------------------------------------------------------------------------------------------------------------
def test_header_parses_completely():
    decls = hip.parse_header(HEADER)
    assert sorted(decls) == declared_symbols() and len(decls) == 138
    for name, params in decls.items():
        for decl, pname, ctype in params:
            assert pname.isidentifier() and (ctype in hip.SCALARS.values() or issubclass(ctype, hip.Pointer)), (name, decl, pname)
    assert decls["grl_version"] == [] and [p[1] for p in decls["grl_source_hash"]] == ["buf", "cap"]
    # the comment inside a parameter list is not part of it, and every launch ends in the stream
    assert [p[:2] for p in decls["grl_value_loss"][8:]] == [("float*", "mean_out"), ("int", "batch"), ("hipStream_t", "stream")]
    assert sum(p[0] == "double" for params in decls.values() for p in params) == 11   # count1 / count2 of the DeepSets chain, grl_value_loss


@pytest.mark.parametrize("bad, named", [("int grl_odd(short x);", "short x"), ("int grl_odd(const float** x);", "const float** x"),
                                        ("int grl_odd(float* const* const* x);", "x"), ("long grl_odd(int x);", "long grl_odd")])
def test_unknown_declaration_raises_and_is_named(bad, named):
    text = HEADER.replace("int grl_version(void);", "int grl_version(void);\n" + bad)
    with pytest.raises(ValueError, match=re.escape(named)):
        hip.parse_header(text)


def test_dtype_rule_per_pointee():
    """The pointee decides which tensor dtypes a pointer takes: its kind and width.  (The function that applies the table, Pointer.address,
    checks the dtype before the device and words the two refusals differently: the wrong-dtype cases below fail when only it is dropped.)"""
    takes = lambda decl: hip.CTYPES[decl].dtypes
    assert takes("const float*") == {torch.float32} and takes("double*") == {torch.float64} and takes("grl_bf16*") == {torch.bfloat16}
    for decl in ("const int*", "unsigned int*", "int*"):
        assert torch.int32 in takes(decl) and not takes(decl) & {torch.int64, torch.float32, torch.int16, torch.uint8}
    for decl in ("const long long*", "unsigned long long*"):
        assert torch.int64 in takes(decl) and not takes(decl) & {torch.int32, torch.float64, torch.complex64}
    assert {torch.uint8, torch.int8, torch.bool} <= takes("const unsigned char*") and torch.int16 not in takes("const unsigned char*")
    assert takes("const void*") is None and takes("void*") is None   # anything
    assert not takes("const float* const*")   # a HOST array of pointers is never a tensor itself ...
    assert hip.CTYPES["const grl_bf16* const*"].inner.dtypes == {torch.bfloat16}   # ... its elements follow the pointee's rule


# ---- 2. an echo library behind the same binder --------------------------------------------------------------------------------------------
ECHO_H = """typedef void* hipStream_t;
typedef unsigned short grl_bf16;
/* every function writes what it received into a caller-supplied HOST buffer */
int grl_echo_scalars(int i, unsigned u, long long l, float f, double d, double* out /* [5] */);
int grl_echo_arrays(const float* f, const int* i, const long long* l, const double* d, int n, double* out /* [4][n] */);
int grl_echo_pointers(const float* const* a, void* const* b, int n, const void* v, const grl_bf16* h, long long* out /* [2n + 2] */);
int grl_echo_none(void);
int grl_echo_launch(const float* x, int n, float scale, double* out, hipStream_t stream);
"""
ECHO_C = 'extern "C" {\n' + ECHO_H + """
int grl_echo_scalars(int i, unsigned u, long long l, float f, double d, double* out) { out[0] = i; out[1] = u; out[2] = (double)l; out[3] = f; out[4] = d; return 0; }
int grl_echo_arrays(const float* f, const int* i, const long long* l, const double* d, int n, double* out) {
  for (int k = 0; k < n; ++k) { out[k] = f[k]; out[n + k] = i[k]; out[2 * n + k] = (double)l[k]; out[3 * n + k] = d[k]; }
  return 0; }
int grl_echo_pointers(const float* const* a, void* const* b, int n, const void* v, const grl_bf16* h, long long* out) {
  for (int k = 0; k < n; ++k) { out[k] = (long long)a[k]; out[n + k] = (long long)b[k]; }
  out[2 * n] = (long long)v; out[2 * n + 1] = (long long)h; return 0; }
int grl_echo_none(void) { return 7; }
int grl_echo_launch(const float* x, int n, float scale, double* out, hipStream_t stream) {
  if (n < 0) return -2;
  for (int k = 0; k < n; ++k) out[k] = (double)(x[k] * scale);
  out[n] = (double)(long long)stream; return 0; }
}
"""


@pytest.fixture(scope="module")
def echo_entries(tmp_path_factory):
    d = tmp_path_factory.mktemp("echo")
    (d / "echo.h").write_text(ECHO_H)
    (d / "echo.cpp").write_text(ECHO_C)
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-shared", "-fPIC", str(d / "echo.cpp"), "-o", str(d / "libecho.so")], check=True)
    return hip.bind((d / "echo.h").read_text(), ctypes.CDLL(str(d / "libecho.so")))


@pytest.fixture
def echo(echo_entries):
    return lambda name, *args: hip.invoke(echo_entries, name, args)


def test_scalars_arrive_exact(echo):
    out = (ctypes.c_double * 5)()
    assert echo("grl_echo_scalars", -3, 2 ** 32 - 1, 2 ** 40, 0.1, 1 / 3, out) == 0
    assert list(out) == [-3.0, 2.0 ** 32 - 1, 2.0 ** 40, ctypes.c_float(0.1).value, 1 / 3]   # (1/3: all 53 bits; 0.1: rounded once to float)
    echo("grl_echo_scalars", True, 0, -1, 3, 5, out)   # an int for a float or a double parameter converts; a bool is an int
    assert list(out) == [1.0, 0.0, -1.0, 3.0, 5.0]
    echo("grl_echo_scalars", ctypes.c_int(4), ctypes.c_uint(9), ctypes.c_longlong(-2 ** 40), ctypes.c_float(0.5), ctypes.c_double(2 / 3), out)
    assert list(out) == [4.0, 9.0, -2.0 ** 40, 0.5, 2 / 3]   # ctypes instances of the declared type pass through
    assert echo("grl_echo_none") == 7


def test_lists_and_arrays_arrive(echo):
    out = (ctypes.c_double * 12)()
    echo("grl_echo_arrays", [0.5, 1, 2.5], [1, -2, 3], [2 ** 40, 0, -1], (1 / 3, 2, 3), 3, out)
    assert list(out) == [0.5, 1.0, 2.5, 1.0, -2.0, 3.0, 2.0 ** 40, 0.0, -1.0, 1 / 3, 2.0, 3.0]
    echo("grl_echo_arrays", (ctypes.c_float * 3)(1, 2, 3), (ctypes.c_int * 3)(4, 5, 6), (ctypes.c_longlong * 3)(7, 8, 9),
         (ctypes.c_double * 3)(0.1, 0.2, 0.3), 3, out)
    assert list(out) == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 0.1, 0.2, 0.3]
    buf = ctypes.create_string_buffer(16)
    addr = ctypes.addressof(buf)
    ptrs = (ctypes.c_longlong * 8)()
    echo("grl_echo_pointers", [addr, None, addr + 4], [None, addr + 8, 0], 3, buf, None, ptrs)
    assert list(ptrs) == [addr, 0, addr + 4, 0, addr + 8, 0, addr, 0]
    echo("grl_echo_pointers", (ctypes.c_void_p * 1)(addr), (ctypes.c_void_p * 1)(None), 1, ctypes.c_void_p(addr + 2),
         ctypes.byref(ctypes.c_ushort(1)), ptrs)
    assert list(ptrs)[:3] == [addr, 0, addr + 2] and ptrs[3] != 0


def test_refused_arguments_name_entry_point_and_parameter(echo):
    out = (ctypes.c_double * 5)()
    f3, d3 = torch.zeros(3), torch.zeros(3, dtype=torch.float64)
    refused = [
        (TypeError, "'i' (int)", ("grl_echo_scalars", 1.5, 0, 0, 0.0, 0.0, out)),                     # a float for an int parameter
        (TypeError, "'l' (long long)", ("grl_echo_scalars", 1, 0, 2.0, 0.0, 0.0, out)),
        (TypeError, "'f' (float)", ("grl_echo_scalars", 1, 0, 0, "1", 0.0, out)),
        (TypeError, "'d' (double)", ("grl_echo_scalars", 1, 0, 0, 0.0, ctypes.c_float(1.0), out)),    # a ctypes instance of another type
        (TypeError, "'out' (double*)", ("grl_echo_scalars", 1, 0, 0, 0.0, 0.0, [0.0] * 5)),            # a list where the pointee is not const
        (TypeError, "'out' (double*)", ("grl_echo_scalars", 1, 0, 0, 0.0, 0.0, (ctypes.c_float * 5)())),   # element width
        (TypeError, "'out' (double*)", ("grl_echo_scalars", 1, 0, 0, 0.0, 0.0, 0)),                    # an integer is no pointer
        (TypeError, "takes 6 arguments (i, u, l, f, d, out), 5 given", ("grl_echo_scalars", 1, 0, 0, 0.0, 0.0)),
        (TypeError, "takes 6 arguments (i, u, l, f, d, out), 7 given", ("grl_echo_scalars", 1, 0, 0, 0.0, 0.0, out, 0)),
        (TypeError, "takes 0 arguments", ("grl_echo_none", 0)),
        (ValueError, "'f' (const float*)", ("grl_echo_arrays", torch.zeros(3, 2)[:, 0], [1] * 3, [1] * 3, [1.0] * 3, 3, out)),   # non-contiguous
        # the dtype rule, refused as such (not by the device rule, whose words are others: the next test)
        (TypeError, "'f' (const float*), argument 1: TypeError: const float* does not point at torch.float64 elements",
         ("grl_echo_arrays", d3, [1] * 3, [1] * 3, [1.0] * 3, 3, out)),
        (TypeError, "'i' (const int*), argument 2: TypeError: const int* does not point at torch.int64 elements",
         ("grl_echo_arrays", [1.0] * 3, d3.long(), [1] * 3, [1.0] * 3, 3, out)),
        (TypeError, "'l' (const long long*), argument 3: TypeError: const long long* does not point at torch.int32 elements",
         ("grl_echo_arrays", [1.0] * 3, [1] * 3, d3.int(), [1.0] * 3, 3, out)),
        (TypeError, "'d' (const double*), argument 4: TypeError: const double* does not point at torch.float32 elements",
         ("grl_echo_arrays", [1.0] * 3, [1] * 3, [1] * 3, f3, 3, out)),
        (TypeError, "'h' (const grl_bf16*), argument 5: TypeError: const grl_bf16* does not point at torch.float32 elements",
         ("grl_echo_pointers", [], [], 0, None, f3, out)),
        (TypeError, "'a' (const float* const*), argument 1: TypeError: const float* does not point at torch.float64 elements",
         ("grl_echo_pointers", [d3], [None], 1, None, None, out)),                                     # ... also as an element of a list
        (TypeError, "'a' (const float* const*), argument 1: TypeError: const float* const* does not point at torch.float32 elements",
         ("grl_echo_pointers", f3, [None], 1, None, None, out)),                                       # a tensor is no HOST array of pointers
        (TypeError, "'i' (const int*)", ("grl_echo_arrays", [1.0] * 3, [1, 2.5, 3], [1] * 3, [1.0] * 3, 3, out)),   # a float in an int list
    ]
    for kind, words, (name, *args) in refused:
        with pytest.raises(kind, match=re.escape(words)) as e:
            echo(name, *args)
        assert name in str(e.value), (name, str(e.value))
    with pytest.raises(AttributeError, match="grl_echo_missing is not declared"):
        echo("grl_echo_missing", 1)


def test_host_tensors_are_refused_on_every_pointer_parameter(echo):
    """The device rule: a pointer parameter points at device memory, so a CPU tensor of the right dtype is refused wherever it is handed in."""
    out = (ctypes.c_double * 12)()
    f, i, l, d = torch.zeros(3), torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.float64)
    h, b = torch.zeros(3, dtype=torch.bfloat16), torch.zeros(3, dtype=torch.uint8)
    good = [[1.0] * 3, [1] * 3, [1] * 3, [1.0] * 3]
    for k, t in enumerate((f, i, l, d)):
        with pytest.raises(TypeError, match="const .* points at device memory, the tensor is on cpu"):
            echo("grl_echo_arrays", *good[:k], t, *good[k + 1:], 3, out)
    for args in (([f], [None], 1, None, None), ([None], [b], 1, None, None), ([None], [None], 1, b, None), ([None], [None], 1, None, h),
                 ([None], [None], 1, None, None, l)):
        with pytest.raises(TypeError, match="points at device memory, the tensor is on cpu"):
            echo("grl_echo_pointers", *args, *([out] if len(args) == 5 else []))
    with pytest.raises(TypeError, match=re.escape("'out' (double*), argument 6: TypeError: double* points at device memory")):
        echo("grl_echo_scalars", 1, 0, 0, 0.0, 0.0, d)


def test_call_and_query_go_through_the_binder(echo_entries, monkeypatch):
    """hip.call / hip.query on the echo library: the stream is appended last, KERNEL_ROWS / the status error behave as before."""
    library = hip.Library("echo", "libecho.so", "echo.h", [])
    library.entries = echo_entries
    monkeypatch.setattr(hip, "_index", dict.fromkeys(echo_entries, library))
    x, out = (ctypes.c_float * 2)(1.5, -2.0), (ctypes.c_double * 3)()
    assert hip.call("grl_echo_launch", x, 2, 2, out, stream=ctypes.c_void_p(1234)) is None
    assert list(out) == [3.0, -4.0, 1234.0]
    assert hip.query("grl_echo_none") == 7 and hip.query("grl_echo_launch", x, 1, 1.0, out, None) == 0 and out[1] == 0.0
    with pytest.raises(RuntimeError, match="grl_echo_launch failed with status -2"):
        hip.call("grl_echo_launch", x, -1, 1.0, out, stream=ctypes.c_void_p(0))
    with pytest.raises(TypeError, match=re.escape("grl_echo_launch takes 5 arguments (x, n, scale, out, stream), 4 given")):
        hip.call("grl_echo_launch", x, 2, out, stream=ctypes.c_void_p(0))


# ---- 3. every literal entry-point name in the tree is declared --------------------------------------------------------------------------
def test_every_literal_entry_point_name_is_declared():
    decls = {}
    for library in hip.LIBRARIES:   # hip.call / hip.query serve every library: a name may be declared by any of the headers
        decls.update(hip.parse_header(open(library.paths()[1]).read()))
    files =[os.path.join(ROOT, "bench.py")] + [os.path.join(ROOT, d, f) for d in ("geometry_rl_amd", "tests")
                                                 for f in sorted(os.listdir(os.path.join(ROOT, d))) if f.endswith(".py")]
    files.remove(os.path.abspath(__file__))   # (the echo library's names)
    used, missing = 0, []
    for path in files:
        for m in re.finditer(r'\bhip\.(call|query)\(\s*"(grl_[a-z0-9_]+)"(\s*\+\s*[\w.]*prec\b)?', open(path).read()):
            used += 1
            for name in [m.group(2)] + ([m.group(2) + "_bf16"] if m.group(3) else []):
                if name not in decls or (decls[name][-1:] or [("",)])[-1][0] != "hipStream_t" and m.group(1) == "call":
                    missing.append((os.path.relpath(path, ROOT), m.group(1), name))
    assert used > 255 and not missing, missing   # (262 sites, 36 of them the satellites'; launches must also end in the stream that hip.call appends)
