"""ctypes binding of the C-ABI kernel library ``libgrl_hip.so`` (declared in include/grl_hip.h).

There is NO fallback: if the shared library is missing or a symbol cannot be resolved the import of this module (and
therefore every op of the package) raises.  Tensors are passed as raw device pointers + the current HIP stream.
"""
import ctypes
import os
import re
import subprocess
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("GRL_LIB", os.path.join(_HERE, "libgrl_hip.so"))  # GRL_LIB: debugging builds only
ABI_VERSION = 216   # include/grl_hip.h GRL_HIP_VERSION
SOURCES = ["edge_conv.hip", "edge_conv16.hip", "node_ops.hip", "node_mlp.hip", "node_mlp16.hip", "head_ops.hip",
           "critic_ops.hip", "train_ops.hip", "weight_images.hip", "calib.hip", "oneshot.hip", "stats_ops.hip"]
# The EMPN key / query attention kernels are a library of their own, libgrl_attention.so, declared in csrc/grl_attention.h: the export
# list of libgrl_hip.so is exactly include/grl_hip.h, which they leave as it is.  Same flags, same binder (attention_call / attention_query).
ATTENTION_SOURCES = ["attention_ops.hip"]
ATTENTION_HEADER = "grl_attention.h"
ATTENTION_LIB_PATH = os.path.join(_HERE, "libgrl_attention.so")
# The transformer baseline actor's kernels (encoder forward / backward, post_fc head) likewise: libgrl_transformer.so, declared in
# csrc/grl_transformer.h, bound by transformer_call / transformer_query (ABI 216 of include/grl_hip.h names the addition).
TRANSFORMER_SOURCES = ["transformer_ops.hip"]
TRANSFORMER_HEADER = "grl_transformer.h"
TRANSFORMER_LIB_PATH = os.path.join(_HERE, "libgrl_transformer.so")
# (source, extra flags, object suffix): the two MFMA files are compiled a second time as the plain-bf16 variant (one MFMA per
# product instead of three; csrc/grl_common.h GRL_PREC) whose entry points carry the suffix _bf16
# per-source compiler flags.  edge_conv16.hip: its 512-register backward kernel keeps the chain's MFMA results in VGPRs (the default
# selection would put every MFMA result of such a kernel into AGPRs) and pins the weight-gradient tiles to AGPRs itself (asm)
# node_mlp16.hip additionally without SLP vectorisation: beside the MFMAs of its one wave per SIMD plain f32 instructions overlap with the matrix
# pipe, packed ones (v_pk_*) do not (DESIGN.md finding 23); edge_conv16.hip the same (+1 % on the step, docs/history/profiles/r03_ab_edge16_noslp.txt)
FILE_FLAGS = {"edge_conv16.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize"],
              "node_mlp16.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize"],
              # the ConvNeXt forward: plain-f32 GELU as well (0.313 vs 0.330 ms per step; the 16-row edge forward, three waves per SIMD, is
              # FASTER with its packed GELU: 0.48 vs 0.52 ms -- docs/history/profiles/r03_ab_forward_gelu_ld1.txt)
              "node_mlp.hip": ["-fno-slp-vectorize", "-DGRL_GELU4_SCALAR=1"]}
VARIANTS = [("edge_conv.hip", ["-DGRL_PREC=1"], ".bf16"), ("edge_conv16.hip", ["-DGRL_PREC=1"], ".bf16"),
            ("node_mlp.hip", ["-DGRL_PREC=1"], ".bf16"), ("node_mlp16.hip", ["-DGRL_PREC=1"], ".bf16"),
            ("node_ops.hip", ["-DGRL_PREC=1"], ".bf16"), ("weight_images.hip", ["-DGRL_PREC=1"], ".bf16")]


BUILD_INFO = os.path.join(os.path.dirname(_HERE), "BUILD_INFO.json")
BASE_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value"]
HASH_TAG = b"GRL_SOURCE_HASH="
EXPORT_RE = r"\bint\s+(grl_[a-z0-9_]+)\s*\("   # the entry points of include/grl_hip.h: the names the link's version script exports


def _sha(*chunks) -> str:
    import hashlib
    h = hashlib.sha256()
    for c in chunks:
        h.update(c if isinstance(c, bytes) else str(c).encode())
        h.update(b"\0")
    return h.hexdigest()


def _read(path) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def _pkg_paths(root=None):
    """(csrc directory, include/grl_hip.h, isa_lint.py) of the package tree at ``root`` (default: this checkout)."""
    pkg = os.path.join(root, "geometry_rl_amd") if root else _HERE
    return os.path.join(pkg, "csrc"), os.path.join(os.path.dirname(pkg), "include", "grl_hip.h"), os.path.join(pkg, "isa_lint.py")


def source_hash(root=None) -> str:
    """16 hex digits over EVERYTHING libgrl_hip.so is made from: every .hip / .h under csrc/, include/grl_hip.h (the export list), the
    ISA lint's rules and the flag tables of this module.  ``hip.build()`` embeds it in the library (``grl_source_hash``), ``hip.lib()``
    recomputes it from the tree and refuses a library that was built from other sources -- modification times play no part (a tree copied
    to another box has arbitrary ones: VERDICT r5)."""
    import json
    csrc, header, lint = _pkg_paths(root)
    names = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".h")))
    parts = [json.dumps([BASE_FLAGS, SOURCES, FILE_FLAGS, VARIANTS, ATTENTION_SOURCES, TRANSFORMER_SOURCES], sort_keys=True)]
    for n in names:
        parts += [n, _read(os.path.join(csrc, n))]
    parts += ["grl_hip.h", _read(header), "isa_lint.py", _read(lint)]
    return _sha(*parts)[:16]


def embedded_hash(path) -> str:
    """The source hash a built library carries (read from the file's bytes: no dlopen), or "" for a library without one."""
    try:
        m = re.search(HASH_TAG + rb"([0-9a-f]{16})", _read(path))
    except OSError:
        return ""
    return m.group(1).decode() if m else ""


def check_library(path=None, root=None) -> str:
    """Raise unless the library at ``path`` was built from the sources of the tree at ``root``; -> the hash."""
    path = path or LIB_PATH
    want, have = source_hash(root), embedded_hash(path)
    if want != have:
        raise RuntimeError(f"{path} was built from other sources than this tree (library {have or 'carries no source hash'}, tree {want}): "
                           "rebuild the extension (python -c 'import __graft_entry__ as g; g.build()')")
    return want


def build(verbose: bool = True, force: bool = False, root=None) -> str:
    """Compile every HIP source for gfx950 and link libgrl_hip.so in-tree (hipcc cross-compiles without a GPU).  What is rebuilt is decided
    by CONTENT: an object is kept when the hash recorded beside it (its source, every header, its flags, the lint rules) still matches, the
    library when its embedded ``grl_source_hash`` equals ``source_hash()`` of the tree.  Writes BUILD_INFO.json at the repository root
    ("prebuilt" = nothing compiled).  ``root``: build another checkout of this repository (tests)."""
    import json
    import time
    csrc, header, lint_py = _pkg_paths(root)
    lib_path = os.path.join(os.path.dirname(csrc), "libgrl_hip.so") if root else LIB_PATH
    att_path = os.path.join(os.path.dirname(csrc), "libgrl_attention.so") if root else ATTENTION_LIB_PATH
    tf_path = os.path.join(os.path.dirname(csrc), "libgrl_transformer.so") if root else TRANSFORMER_LIB_PATH
    info_path = os.path.join(root, "BUILD_INFO.json") if root else BUILD_INFO
    srcs = [os.path.join(csrc, s) for s in SOURCES if os.path.exists(os.path.join(csrc, s))]
    att_srcs = [os.path.join(csrc, s) for s in ATTENTION_SOURCES]
    tf_srcs = [os.path.join(csrc, s) for s in TRANSFORMER_SOURCES]
    tree_hash = source_hash(root)

    def info(mode, rebuilt, lint=None):
        try:
            with open(info_path, "w") as f:
                json.dump({"build_mode": mode, "objects_rebuilt": rebuilt, "isa_lint": lint, "objects_total": len(srcs) + len(VARIANTS) + len(att_srcs) + len(tf_srcs) + 1,
                           "library": os.path.relpath(lib_path, os.path.dirname(os.path.dirname(csrc))),
                           "library_bytes": os.path.getsize(lib_path) if os.path.exists(lib_path) else None, "abi_version": ABI_VERSION,
                           "source_hash": tree_hash, "library_source_hash": embedded_hash(lib_path),
                           "forced": bool(force), "time": time.strftime("%Y-%m-%dT%H:%M:%S")}, f, indent=1)
        except OSError:
            pass
    if not force and embedded_hash(lib_path) == tree_hash and embedded_hash(att_path) == tree_hash and embedded_hash(tf_path) == tree_hash:
        info("prebuilt (the libraries' embedded source hash equals the tree's: nothing compiled)", [])
        return lib_path
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    from . import isa_lint
    header_bytes = [_read(os.path.join(csrc, h)) for h in sorted(f for f in os.listdir(csrc) if f.endswith(".h"))]   # every header feeds every object
    lint_bytes = _read(lint_py)
    objs, att_objs, tf_objs = [], [], []
    procs = []
    rebuilt = []
    lint_jobs = []   # (label, assembly file, object, its hash file, its hash) of every object compiled NOW from a source with asm MFMAs
    pending = []     # (hash file, hash) of the other objects compiled now: recorded once hipcc has succeeded
    bdir = os.path.join(csrc, "build")
    os.makedirs(bdir, exist_ok=True)
    jobs = [(s, [], "") for s in srcs] + [(os.path.join(csrc, s), fl, sfx) for s, fl, sfx in VARIANTS] + [(s, [], "") for s in att_srcs] + [(s, [], "") for s in tf_srcs]
    for s, flags, sfx in jobs:
        base = os.path.basename(s)
        lint = base in isa_lint.FILES
        # sources with asm MFMAs are compiled with -save-temps into a directory of their own: the assembly the REAL compile leaves behind
        # is what the ISA lint reads (a different hipcc or different flags must not get past the hazard check)
        odir = os.path.join(bdir, base + sfx + ".d") if lint else bdir
        os.makedirs(odir, exist_ok=True)
        o = os.path.join(odir, base + sfx + ".o")
        (att_objs if s in att_srcs else tf_objs if s in tf_srcs else objs).append(o)
        cmd_flags = BASE_FLAGS + FILE_FLAGS.get(base, []) + flags + (["-save-temps=obj"] if lint else [])
        ohash = _sha(_read(s), *header_bytes, " ".join(cmd_flags), lint_bytes if lint else b"")
        hfile = o + ".srchash"
        if not force and os.path.exists(o) and os.path.exists(hfile) and _read(hfile).decode().strip() == ohash:
            continue
        for stale in (o, hfile):   # never leave an object behind whose recorded hash could vouch for it after a failed compile
            if os.path.exists(stale):
                os.remove(stale)
        cmd = [hipcc] + cmd_flags + ["-c", s, "-o", o]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        rebuilt.append(os.path.basename(o))
        if lint:
            lint_jobs.append((base + sfx, os.path.join(odir, os.path.splitext(base)[0] + "-hip-amdgcn-amd-amdhsa-gfx950.s"), o, hfile, ohash, base))
        else:
            pending.append((hfile, ohash))
        procs.append((cmd, subprocess.Popen(cmd, stderr=subprocess.PIPE if not verbose else None)))
    failed = []
    for cmd, p in procs:
        _, err = p.communicate()
        if p.returncode != 0:
            failed.append(" ".join(cmd) + ("\n" + err.decode(errors="replace")[-4000:] if err else ""))
    if failed:
        raise RuntimeError("hipcc failed:\n" + "\n".join(failed))
    for hfile, ohash in pending:
        with open(hfile, "w") as f:
            f.write(ohash)
    # lint EVERY job before judging any: an object's hash file is written only when its assembly passed, and every object that failed is
    # removed -- a later incremental build can neither link an unchecked object nor skip its lint
    lint_report, lint_failed = {}, []
    for label, asm, o, hfile, ohash, base in lint_jobs:
        n, n_asm, bad = isa_lint.lint_assembly(asm, isa_lint.EXPECTED.get(base, ()))
        lint_report[label] = {"kernels": n, "kernels_with_asm_mfma": n_asm, "findings": bad}
        if bad or n_asm == 0:
            if os.path.exists(o):
                os.remove(o)
            lint_failed.append(f"{label}: " + ("; ".join(bad) if bad else "no kernel with asm MFMAs found in the assembly -- the lint saw nothing"))
        else:
            with open(hfile, "w") as f:
                f.write(ohash)
    if lint_failed:
        raise RuntimeError("ISA lint failed (geometry_rl_amd/isa_lint.py): " + " | ".join(lint_failed))
    # exports = exactly the entry points include/grl_hip.h declares (cross-file helpers such as grl_edge16_launch stay internal)
    names = sorted(set(re.findall(EXPORT_RE, open(header).read())))
    vs = os.path.join(bdir, "exports.map")
    with open(vs, "w") as f:
        f.write("{\n  global:\n" + "".join(f"    {n};\n" for n in names) + "  local: *;\n};\n")
    # the tree's source hash, embedded: grl_source_hash() hands it out, embedded_hash() finds it in the file's bytes
    hsrc = os.path.join(bdir, "source_hash.cpp")
    with open(hsrc, "w") as f:
        f.write('// generated by geometry_rl_amd/hip.py build()\n'
                f'static const char grl_hash_tag[] = "{HASH_TAG.decode()}{tree_hash}";\n'
                'extern "C" int grl_source_hash(char* buf, int cap) {\n'
                '  const char* h = grl_hash_tag + %d; int n = 0;\n'
                '  while (h[n] && n + 1 < cap) { buf[n] = h[n]; ++n; }\n'
                '  if (cap > 0) buf[n] = 0;\n  return n;\n}\n' % len(HASH_TAG))
    hobj = os.path.join(bdir, "source_hash.o")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-fPIC", "-c", hsrc, "-o", hobj])
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + vs, "-o", lib_path] + objs + [hobj]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    if embedded_hash(lib_path) != tree_hash:
        raise RuntimeError(f"{lib_path}: the embedded source hash did not survive the link")
    # the attention library: its own objects, its own export list (csrc/grl_attention.h), the same embedded source hash
    att_names = sorted(set(re.findall(EXPORT_RE, open(os.path.join(csrc, ATTENTION_HEADER)).read())))
    avs = os.path.join(bdir, "exports_attention.map")
    with open(avs, "w") as f:
        f.write("{\n  global:\n" + "".join(f"    {n};\n" for n in att_names) + "  local: *;\n};\n")
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + avs, "-o", att_path] + att_objs + [hobj]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    if embedded_hash(att_path) != tree_hash:
        raise RuntimeError(f"{att_path}: the embedded source hash did not survive the link")
    # ... and the transformer actor's library, the same way (csrc/grl_transformer.h)
    tf_names = sorted(set(re.findall(EXPORT_RE, open(os.path.join(csrc, TRANSFORMER_HEADER)).read())))
    tvs = os.path.join(bdir, "exports_transformer.map")
    with open(tvs, "w") as f:
        f.write("{\n  global:\n" + "".join(f"    {n};\n" for n in tf_names) + "  local: *;\n};\n")
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + tvs, "-o", tf_path] + tf_objs + [hobj]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    if embedded_hash(tf_path) != tree_hash:
        raise RuntimeError(f"{tf_path}: the embedded source hash did not survive the link")
    info("compiled from source" if len(rebuilt) == len(objs) + len(att_objs) + len(tf_objs) else "incremental (objects whose recorded source hash still matched were kept)", rebuilt, lint_report)
    return lib_path


# ---- the typed boundary: every entry point's argument types come from include/grl_hip.h ------------------------------------------------
SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "long long": ctypes.c_longlong, "float": ctypes.c_float,
           "double": ctypes.c_double, "hipStream_t": ctypes.c_void_p}
_I4, _I8 = {torch.int32, torch.uint32}, {torch.int64, torch.uint64}
_B1 = {torch.uint8, torch.int8, torch.bool, torch.float8_e4m3fn, torch.float8_e5m2}
# pointee -> (ctypes element type, the tensor dtypes of its kind and width; None: any)
POINTEES = {"float": (ctypes.c_float, {torch.float32}), "double": (ctypes.c_double, {torch.float64}), "grl_bf16": (ctypes.c_ushort, {torch.bfloat16}),
            "int": (ctypes.c_int, _I4), "unsigned": (ctypes.c_uint, _I4), "unsigned int": (ctypes.c_uint, _I4), "long long": (ctypes.c_longlong, _I8),
            "unsigned long long": (ctypes.c_ulonglong, _I8), "unsigned char": (ctypes.c_ubyte, _B1), "char": (ctypes.c_char, _B1), "void": (None, None)}
_PASSED_ON = (type(ctypes.byref(ctypes.c_int())), ctypes.c_void_p, ctypes.c_char_p, ctypes._Pointer)


class Pointer:
    """ctypes argument type of one pointer parameter (one subclass per declared type in CTYPES).  It takes None (NULL); a contiguous device
    tensor of the pointee's kind and width; a ctypes byref / pointer (passed on) or array (its element width checked); and, where the pointee
    is const (the header's HOST arrays), a list or tuple -- of numbers, or for an array of pointers (``inner``: the element's type) of
    tensors, None and integer addresses."""
    decl, elem, dtypes, const, inner = "void*", None, None, False, None

    @classmethod
    def address(cls, t: torch.Tensor) -> int:
        if not t.is_contiguous():
            raise ValueError("non-contiguous tensor passed to a HIP kernel")
        if cls.dtypes is not None and t.dtype not in cls.dtypes:
            raise TypeError(f"{cls.decl} does not point at {t.dtype} elements")
        if not t.is_cuda:
            raise TypeError(f"{cls.decl} points at device memory, the tensor is on {t.device}")
        return t.data_ptr()

    @classmethod
    def from_param(cls, a):
        if isinstance(a, torch.Tensor):
            return ctypes.c_void_p(cls.address(a))
        if a is None or isinstance(a, _PASSED_ON):
            return a
        if isinstance(a, ctypes.Array) and (cls.elem is None or ctypes.sizeof(a._type_) == ctypes.sizeof(cls.elem)):
            return a
        if isinstance(a, (list, tuple)) and cls.const and cls.elem is not None:
            return (cls.elem * len(a))(*[cls.inner.address(e) if cls.inner and isinstance(e, torch.Tensor) else e for e in a])
        what = f"an array of {a._type_.__name__}" if isinstance(a, ctypes.Array) else f"a {type(a).__name__}"
        raise TypeError(f"{cls.decl} takes None, a device tensor, a ctypes array / pointer{' or a list' if cls.const else ''}, not {what}")


CTYPES = dict(SCALARS)   # declared parameter type -> ctypes argument type: the header's whole vocabulary
for _p, (_elem, _dtypes) in POINTEES.items():
    for _c in ("", "const "):
        _t = CTYPES[_c + _p + "*"] = type("Pointer", (Pointer,), dict(decl=_c + _p + "*", elem=_elem, dtypes=_dtypes, const=bool(_c)))
        CTYPES[_c + _p + "* const*"] = type("Pointer", (Pointer,), dict(decl=_c + _p + "* const*", elem=ctypes.c_void_p, dtypes=set(), const=True, inner=_t))


def parse_header(text: str) -> dict:
    """include/grl_hip.h (or a header in its style) -> {entry point: [(declared type, parameter name, ctypes type)]}.  Every statement is a
    typedef or ``int grl_x(...)`` over known types and the names are exactly the exported ones: anything else raises and names it."""
    body = re.sub(r'/\*.*?\*/|^\s*#[^\n]*|extern "C" \{', " ", text, flags=re.S | re.M)
    decls = {}
    for stmt in (" ".join(s.split()) for s in body.split(";")):
        if stmt in ("", "}") or stmt.startswith("typedef "):
            continue
        try:
            name, plist = re.fullmatch(r"int (grl_\w+) ?\((.*)\)", stmt).groups()
            params = [re.fullmatch(r"(.*\W)(\w+)", p.strip()).groups() for p in plist.split(",") if plist != "void"]
            decls[name] = [(t.strip(), n, CTYPES[t.strip()]) for t, n in params]
        except (AttributeError, KeyError) as e:
            raise ValueError(f"cannot bind the declaration '{stmt}' ({e!r})") from None
    if set(re.findall(EXPORT_RE, text)) != set(decls):
        raise ValueError(f"parsed and exported names differ: {sorted(set(re.findall(EXPORT_RE, text)) ^ set(decls))}")
    return decls


def bind(header_text: str, cdll) -> dict:
    """{name: entry point of ``cdll``} for every declaration of the header, ``restype`` and ``argtypes`` set once, here (``fn.params``: the
    header's (declared type, parameter name, ctypes type) list)."""
    entries = {}
    for name, params in parse_header(header_text).items():
        fn = entries[name] = getattr(cdll, name)
        fn.restype, fn.params, fn.argtypes = ctypes.c_int, params, [p[2] for p in params]
    return entries


def invoke(entries: dict, name: str, args) -> int:
    """entries[name](*args), refusing an undeclared name, a wrong argument count and -- in the header's words -- a wrong argument."""
    fn = entries.get(name)
    if fn is None:
        raise AttributeError(f"{name} is not declared in the header (include/grl_hip.h): no entry point is called untyped")
    if len(args) != len(fn.params):   # (ctypes itself lets surplus arguments through)
        raise TypeError(f"{name} takes {len(fn.params)} arguments ({', '.join(p[1] for p in fn.params)}), {len(args)} given")
    try:
        return fn(*args)
    except ctypes.ArgumentError as e:   # ctypes' "argument 3: TypeError: ..." with the header's words for that parameter
        decl, pname, _ = fn.params[int(str(e).split(":")[0].split()[-1]) - 1]
        raise (ValueError if ": ValueError: " in str(e) else TypeError)(f"{name}: '{pname}' ({decl}), {e}") from None


_lib = _bound = None


def lib() -> ctypes.CDLL:
    global _lib, _bound
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension must be built (python -c 'import __graft_entry__ as g; g.build()'). "
                "geometry_rl_amd has no CPU or PyTorch fallback path.")
        cdll = ctypes.CDLL(LIB_PATH)
        # the binary must be the one THESE sources build (an explicitly named debugging library -- GRL_LIB, tools/r0*_ab_libs.sh -- is the
        # caller's business; GRL_ALLOW_STALE_LIB=1 switches the check off for bisecting)
        if "GRL_LIB" not in os.environ and os.environ.get("GRL_ALLOW_STALE_LIB", "0") == "0":
            check_library(LIB_PATH)
        bound = bind(_read(_pkg_paths()[1]).decode(), cdll)
        if cdll.grl_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} reports ABI version {cdll.grl_version()}, this package binds version {ABI_VERSION} "
                               "(include/grl_hip.h GRL_HIP_VERSION): rebuild the extension (__graft_entry__.build())")
        _lib, _bound = cdll, bound
    return _lib


_att_bound = None


def attention_lib() -> dict:
    """The bound entry points of libgrl_attention.so (csrc/grl_attention.h), loaded on first use.  No fallback: a missing or stale
    library raises."""
    global _att_bound
    if _att_bound is None:
        if not os.path.exists(ATTENTION_LIB_PATH):
            raise RuntimeError(
                f"{ATTENTION_LIB_PATH} is missing: the HIP extension must be built (python -c 'import __graft_entry__ as g; g.build()'). "
                "geometry_rl_amd has no CPU or PyTorch fallback path.")
        if "GRL_LIB" not in os.environ and os.environ.get("GRL_ALLOW_STALE_LIB", "0") == "0":
            check_library(ATTENTION_LIB_PATH)
        _att_bound = bind(_read(os.path.join(CSRC, ATTENTION_HEADER)).decode(), ctypes.CDLL(ATTENTION_LIB_PATH))
    return _att_bound


_tf_bound = None


def transformer_lib() -> dict:
    """The bound entry points of libgrl_transformer.so (csrc/grl_transformer.h), loaded on first use.  No fallback: a missing or stale
    library raises."""
    global _tf_bound
    if _tf_bound is None:
        if not os.path.exists(TRANSFORMER_LIB_PATH):
            raise RuntimeError(
                f"{TRANSFORMER_LIB_PATH} is missing: the HIP extension must be built (python -c 'import __graft_entry__ as g; g.build()'). "
                "geometry_rl_amd has no CPU or PyTorch fallback path.")
        if "GRL_LIB" not in os.environ and os.environ.get("GRL_ALLOW_STALE_LIB", "0") == "0":
            check_library(TRANSFORMER_LIB_PATH)
        _tf_bound = bind(_read(os.path.join(CSRC, TRANSFORMER_HEADER)).decode(), ctypes.CDLL(TRANSFORMER_LIB_PATH))
    return _tf_bound


def stream_ptr() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# Optional per-entry-point timing with HIP events recorded on the launch stream (bench.py's roofline leg).
# KERNEL_TIMES maps name -> list of (start_event, end_event); enable with ``hip.KERNEL_TIMES = {}``.
KERNEL_TIMES = None
KERNEL_ROWS = {}   # name -> rows (edge x orientation / node x orientation) handed to the entry point while timing is on


def call(name: str, *args, stream=None, rows: int = 0) -> None:
    """Launch C-ABI entry point ``name`` on the current stream; raises on a refused argument (before the launch) and on a non-zero status."""
    _launch(query, name, args, stream, rows)


def attention_call(name: str, *args, stream=None, rows: int = 0) -> None:
    """``call`` for an entry point of libgrl_attention.so (csrc/grl_attention.h)."""
    _launch(attention_query, name, args, stream, rows)


def transformer_call(name: str, *args, stream=None, rows: int = 0) -> None:
    """``call`` for an entry point of libgrl_transformer.so (csrc/grl_transformer.h)."""
    _launch(transformer_query, name, args, stream, rows)


def transformer_query(name: str, *args) -> int:
    """``query`` for an entry point of libgrl_transformer.so."""
    return invoke(transformer_lib(), name, args)


def attention_query(name: str, *args) -> int:
    """``query`` for an entry point of libgrl_attention.so."""
    return invoke(attention_lib(), name, args)


def _launch(query, name, args, stream, rows) -> None:
    timing = KERNEL_TIMES is not None
    if timing:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    rc = query(name, *args, stream if stream is not None else stream_ptr())
    if timing:
        e1.record()
        KERNEL_TIMES.setdefault(name, []).append((e0, e1))
        KERNEL_ROWS[name] = KERNEL_ROWS.get(name, 0) + rows
    if rc != 0:
        raise RuntimeError(f"{name} failed with status {rc}")


def kernel_time_summary():
    """-> {name: (n_calls, total_ms)} from the recorded events (synchronises)."""
    torch.cuda.synchronize()
    return {k: (len(v), sum(a.elapsed_time(b) for a, b in v)) for k, v in (KERNEL_TIMES or {}).items()}


def kernel_prof_enable(on: bool) -> None:
    """In-library HIP-event timing of the kernels inside multi-kernel entry points (grl_prof_*)."""
    query("grl_prof_enable", int(on))


def kernel_prof_summary():
    """-> {kernel name: (n_launches, total_ms)} from the in-library records (synchronises on each record)."""
    out = {}
    buf = ctypes.create_string_buffer(96)
    ms = ctypes.c_float(0.0)
    for i in range(query("grl_prof_count")):
        if query("grl_prof_get", i, buf, 96, ctypes.byref(ms)) != 0:
            raise RuntimeError("grl_prof_get failed")
        n, t = out.get(buf.value.decode(), (0, 0.0))
        out[buf.value.decode()] = (n + 1, t + ms.value)
    return out


def query(name: str, *args) -> int:
    """Call a pure host-side query entry point (no stream argument)."""
    if _bound is None:
        lib()
    return invoke(_bound, name, args)


def check_f32(*tensors: torch.Tensor):
    for t in tensors:
        if t is not None and (t.dtype != torch.float32 or not t.is_cuda):
            raise TypeError(f"expected a CUDA float32 tensor, got {t.dtype} on {t.device}")


def storage_dtype(prec: str) -> torch.dtype:
    """Storage type of the node latents for an entry-point suffix: "" -> float32, "_bf16" -> bfloat16 (csrc/grl_common.h st_t)."""
    return torch.bfloat16 if prec == "_bf16" else torch.float32


def check_latent(prec: str, *tensors: torch.Tensor):
    want = storage_dtype(prec)
    for t in tensors:
        if t is not None and (t.dtype != want or not t.is_cuda):
            raise TypeError(f"expected a CUDA {want} latent tensor for the '{prec or 'fp32'}' kernels, got {t.dtype} on {t.device}")
