"""libgrl_attention.so, the EMPN key / query attention kernels' own library (geometry_rl_amd/csrc/grl_attention.h), without a GPU: the
header parses with the binder of include/grl_hip.h, the library exports exactly what it declares, carries the tree's source hash, and
neither its names nor its object reach libgrl_hip.so, whose export list stays the main header's."""
import ctypes
import os
import subprocess

import pytest

from geometry_rl_amd import hip
from test_abi_and_host import declared_symbols

NAMES = ["grl_attention_blocks", "grl_edge_attend_bwd", "grl_edge_attend_fwd", "grl_edge_logits_bwd", "grl_edge_logits_fwd",
         "grl_kq_bwd_blocks", "grl_kq_partial_size", "grl_kq_project_bwd", "grl_kq_project_fwd"]


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if l.strip())


def test_header_parses_and_library_exports_exactly_its_names():
    hip.build(verbose=False)
    decls = hip.parse_header(open(os.path.join(hip.CSRC, hip.ATTENTION_HEADER)).read())
    assert sorted(decls) == NAMES
    for name, params in decls.items():   # launches end in the stream, the three shape queries take none
        assert (params[-1:] or [("",)])[-1][0] == ("hipStream_t" if name.endswith(("_fwd", "_bwd")) else "int" if params else "")
    assert _exported(hip.ATTENTION_LIB_PATH) == NAMES
    assert hip.embedded_hash(hip.ATTENTION_LIB_PATH) == hip.source_hash() == hip.embedded_hash(hip.LIB_PATH)
    assert not set(NAMES) & set(_exported(hip.LIB_PATH)) and not set(NAMES) & set(declared_symbols())
    # host-only queries are callable without a GPU
    lib = ctypes.CDLL(hip.ATTENTION_LIB_PATH)
    assert lib.grl_kq_partial_size() == 2 * 128 * 64 + 2 * 128
    assert lib.grl_kq_bwd_blocks(0) == 1 and lib.grl_kq_bwd_blocks(65) == 2 and lib.grl_kq_bwd_blocks(10 ** 8) == 512
    assert lib.grl_attention_blocks(0) == 1 and lib.grl_attention_blocks(5) == 2 and lib.grl_attention_blocks(10 ** 8) == 2048


def test_missing_attention_library_is_an_error(monkeypatch, tmp_path):
    monkeypatch.setattr(hip, "ATTENTION_LIB_PATH", str(tmp_path / "missing.so"))
    monkeypatch.setattr(hip, "_att_bound", None)
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        hip.attention_query("grl_kq_partial_size")


def test_undeclared_name_is_refused():
    with pytest.raises(AttributeError, match="is not declared"):
        hip.attention_query("grl_version")
