"""ctypes binding of the C-ABI kernel libraries (``LIBRARIES``: libgrl_hip.so, declared in include/grl_hip.h, and the two satellites).

There is NO fallback: if a shared library is missing or a symbol cannot be resolved the first call into it (and therefore every op of
the package that needs it) raises.  Tensors are passed as raw device pointers + the current HIP stream.
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
# (source, extra flags, object suffix): the two MFMA files are compiled a second time as the plain-bf16 variant (one MFMA per
# product instead of three; csrc/grl_common.h GRL_PREC) whose entry points carry the suffix _bf16
VARIANTS = [("edge_conv.hip", ["-DGRL_PREC=1"], ".bf16"), ("edge_conv16.hip", ["-DGRL_PREC=1"], ".bf16"),
            ("node_mlp.hip", ["-DGRL_PREC=1"], ".bf16"), ("node_mlp16.hip", ["-DGRL_PREC=1"], ".bf16"),
            ("node_ops.hip", ["-DGRL_PREC=1"], ".bf16"), ("weight_images.hip", ["-DGRL_PREC=1"], ".bf16")]
# per-source compiler flags.  edge_conv16.hip: its 512-register backward kernel keeps the chain's MFMA results in VGPRs (the default
# selection would put every MFMA result of such a kernel into AGPRs) and pins the weight-gradient tiles to AGPRs itself (asm)
# node_mlp16.hip additionally without SLP vectorisation: beside the MFMAs of its one wave per SIMD plain f32 instructions overlap with the matrix
# pipe, packed ones (v_pk_*) do not (DESIGN.md finding 23); edge_conv16.hip the same (+1 % on the step, docs/history/profiles/r03_ab_edge16_noslp.txt)
FILE_FLAGS = {"edge_conv16.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize"],
              "node_mlp16.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize"],
              # the ConvNeXt forward: plain-f32 GELU as well (0.313 vs 0.330 ms per step; the 16-row edge forward, three waves per SIMD, is
              # FASTER with its packed GELU: 0.48 vs 0.52 ms -- docs/history/profiles/r03_ab_forward_gelu_ld1.txt)
              "node_mlp.hip": ["-fno-slp-vectorize", "-DGRL_GELU4_SCALAR=1"]}


class Library:
    """One kernel library: its file beside this module, the header that declares its entry points (= its export list; relative to this
    package), its plain sources and its variant jobs under csrc/.  Loaded and bound on first use (``load``), never at import."""

    def __init__(self, name, file, header, sources, variants=(), path=None):
        self.name, self.file, self.header, self.sources, self.variants = name, file, header, list(sources), list(variants)
        self.path = path or os.path.join(_HERE, file)   # the file ``load`` opens
        self.cdll = self.entries = None

    def paths(self, root=None):
        """(library file, header) of this checkout, or of the checkout of this repository at ``root``."""
        pkg = os.path.join(root, "geometry_rl_amd") if root else _HERE
        return os.path.join(pkg, self.file) if root else self.path, os.path.normpath(os.path.join(pkg, self.header))

    def load(self) -> dict:
        """{name: bound entry point} of the library, opened on first use.  No fallback: a missing or stale library raises."""
        if self.entries is None:
            if not os.path.exists(self.path):
                raise RuntimeError(
                    f"{self.path} is missing: the HIP extension must be built (python -c 'import __graft_entry__ as g; g.build()'). "
                    "geometry_rl_amd has no CPU or PyTorch fallback path.")
            # the binary must be the one THESE sources build (an explicitly named debugging library -- GRL_LIB, tools/r0*_ab_libs.sh -- is the
            # caller's business; GRL_ALLOW_STALE_LIB=1 switches the check off for bisecting)
            if "GRL_LIB" not in os.environ and os.environ.get("GRL_ALLOW_STALE_LIB", "0") == "0":
                check_library(self.path)
            cdll = ctypes.CDLL(self.path)
            entries = bind(_read(self.paths()[1]).decode(), cdll)
            if "grl_version" in entries and cdll.grl_version() != ABI_VERSION:   # (the satellites carry no version entry)
                raise RuntimeError(f"{self.path} reports ABI version {cdll.grl_version()}, this package binds version {ABI_VERSION} "
                                   "(include/grl_hip.h GRL_HIP_VERSION): rebuild the extension (__graft_entry__.build())")
            self.cdll, self.entries = cdll, entries
        return self.entries


# The EMPN key / query attention kernels and the transformer baseline actor's kernels (encoder forward / backward, post_fc head) are
# libraries of their own: the export list of libgrl_hip.so is exactly include/grl_hip.h, which they leave as it is (ABI 216 names the
# additions).  Same flags, same binder, same ``call`` / ``query``: a name's library is the one whose header declares it.
MAIN = Library("main", "libgrl_hip.so", "../include/grl_hip.h", SOURCES, VARIANTS, path=LIB_PATH)
LIBRARIES = [MAIN, Library("attention", "libgrl_attention.so", "csrc/grl_attention.h", ["attention_ops.hip"]),
             Library("transformer", "libgrl_transformer.so", "csrc/grl_transformer.h", ["transformer_ops.hip"])]


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
    """(csrc directory, isa_lint.py) of the package tree at ``root`` (default: this checkout)."""
    pkg = os.path.join(root, "geometry_rl_amd") if root else _HERE
    return os.path.join(pkg, "csrc"), os.path.join(pkg, "isa_lint.py")


def source_hash(root=None) -> str:
    """16 hex digits over EVERYTHING the libraries are made from: every .hip / .h under csrc/, include/grl_hip.h (the export list), the
    ISA lint's rules and the flag and library tables of this module.  ``hip.build()`` embeds it in every library (``grl_source_hash``),
    ``Library.load`` recomputes it from the tree and refuses a library that was built from other sources -- modification times play no
    part (a tree copied to another box has arbitrary ones: VERDICT r5)."""
    import json
    csrc, lint = _pkg_paths(root)
    names = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".h")))
    parts = [json.dumps([BASE_FLAGS, FILE_FLAGS, [[l.name, l.file, l.header, l.sources, l.variants] for l in LIBRARIES]], sort_keys=True)]
    for n in names:
        parts += [n, _read(os.path.join(csrc, n))]
    parts += ["grl_hip.h", _read(MAIN.paths(root)[1]), "isa_lint.py", _read(lint)]
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
    """Compile every HIP source for gfx950 and link the libraries of ``LIBRARIES`` in-tree (hipcc cross-compiles without a GPU).  What is
    rebuilt is decided by CONTENT: an object is kept when the hash recorded beside it (its source, every header, its flags, the lint rules)
    still matches, the libraries when their embedded ``grl_source_hash`` equals ``source_hash()`` of the tree.  Writes BUILD_INFO.json at
    the repository root ("prebuilt" = nothing compiled); -> the main library's path.  ``root``: build another checkout of this repository
    (tests)."""
    import json
    import time
    csrc, lint_py = _pkg_paths(root)
    lib_paths = {l.name: l.paths(root)[0] for l in LIBRARIES}
    lib_path = lib_paths[MAIN.name]
    top = os.path.dirname(os.path.dirname(csrc))
    jobs = [(l, s, fl, sfx) for l in LIBRARIES for s, fl, sfx in [(s, [], "") for s in l.sources] + l.variants]
    tree_hash = source_hash(root)

    def info(mode, rebuilt, lint=None):
        size = lambda p: os.path.getsize(p) if os.path.exists(p) else None
        try:
            with open(os.path.join(top, "BUILD_INFO.json") if root else BUILD_INFO, "w") as f:
                json.dump({"build_mode": mode, "objects_rebuilt": rebuilt, "isa_lint": lint, "objects_total": len(jobs) + 1,
                           "library": os.path.relpath(lib_path, top), "library_bytes": size(lib_path), "abi_version": ABI_VERSION,
                           "source_hash": tree_hash, "library_source_hash": embedded_hash(lib_path),
                           "libraries": {n: {"path": os.path.relpath(p, top), "bytes": size(p), "source_hash": embedded_hash(p)}
                                         for n, p in lib_paths.items()},
                           "forced": bool(force), "time": time.strftime("%Y-%m-%dT%H:%M:%S")}, f, indent=1)
        except OSError:
            pass
    if not force and all(embedded_hash(p) == tree_hash for p in lib_paths.values()):
        info("prebuilt (the libraries' embedded source hash equals the tree's: nothing compiled)", [])
        return lib_path
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    from . import isa_lint
    header_bytes = [_read(os.path.join(csrc, h)) for h in sorted(f for f in os.listdir(csrc) if f.endswith(".h"))]   # every header feeds every object
    lint_bytes = _read(lint_py)
    objs = {l.name: [] for l in LIBRARIES}
    procs = []
    rebuilt = []
    lint_jobs = []   # (label, assembly file, object, its hash file, its hash) of every object compiled NOW from a source with asm MFMAs
    pending = []     # (hash file, hash) of the other objects compiled now: recorded once hipcc has succeeded
    bdir = os.path.join(csrc, "build")
    os.makedirs(bdir, exist_ok=True)
    for library, base, flags, sfx in jobs:
        s = os.path.join(csrc, base)
        lint = base in isa_lint.FILES
        # sources with asm MFMAs are compiled with -save-temps into a directory of their own: the assembly the REAL compile leaves behind
        # is what the ISA lint reads (a different hipcc or different flags must not get past the hazard check)
        odir = os.path.join(bdir, base + sfx + ".d") if lint else bdir
        os.makedirs(odir, exist_ok=True)
        o = os.path.join(odir, base + sfx + ".o")
        objs[library.name].append(o)
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

    def link(library):
        """Its own objects and the shared source hash; exports = exactly the entry points its header declares (cross-file helpers such
        as grl_edge16_launch stay internal)."""
        out, header = library.paths(root)
        vs = os.path.join(bdir, f"exports_{library.name}.map")
        with open(vs, "w") as f:
            f.write("{\n  global:\n" + "".join(f"    {n};\n" for n in sorted(set(re.findall(EXPORT_RE, open(header).read())))) + "  local: *;\n};\n")
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + vs, "-o", out] + objs[library.name] + [hobj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
        if embedded_hash(out) != tree_hash:
            raise RuntimeError(f"{out}: the embedded source hash did not survive the link")
    for library in LIBRARIES:
        link(library)
    info("compiled from source" if len(rebuilt) == len(jobs) else "incremental (objects whose recorded source hash still matched were kept)", rebuilt, lint_report)
    return lib_path


# ---- the typed boundary: every entry point's argument types come from its library's header ------------------------------------------------
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
        raise AttributeError(f"{name} is not declared in a header of the kernel libraries: no entry point is called untyped")
    if len(args) != len(fn.params):   # (ctypes itself lets surplus arguments through)
        raise TypeError(f"{name} takes {len(fn.params)} arguments ({', '.join(p[1] for p in fn.params)}), {len(args)} given")
    try:
        return fn(*args)
    except ctypes.ArgumentError as e:   # ctypes' "argument 3: TypeError: ..." with the header's words for that parameter
        decl, pname, _ = fn.params[int(str(e).split(":")[0].split()[-1]) - 1]
        raise (ValueError if ": ValueError: " in str(e) else TypeError)(f"{name}: '{pname}' ({decl}), {e}") from None


def entry_index(headers) -> dict:
    """{entry name: owner} over (owner, header text) pairs; a name that two headers declare raises."""
    index = {}
    for owner, text in headers:
        for name in parse_header(text):
            if name in index:
                raise ValueError(f"{name} is declared by two headers: an entry point has one library")
            index[name] = owner
    return index


_index = None   # {entry name: its Library}, from the headers' text on first use (no library is loaded for it)


def query(name: str, *args) -> int:
    """Call entry point ``name`` of the library whose header declares it, as it stands: a pure host-side query takes no stream argument."""
    global _index
    if _index is None:
        _index = entry_index((l, _read(l.paths()[1]).decode()) for l in LIBRARIES)
    library = _index.get(name)
    return invoke(library.load() if library else {}, name, args)


def lib() -> ctypes.CDLL:
    MAIN.load()
    return MAIN.cdll


def stream_ptr() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# Optional per-entry-point timing with HIP events recorded on the launch stream (bench.py's roofline leg).
# KERNEL_TIMES maps name -> list of (start_event, end_event); enable with ``hip.KERNEL_TIMES = {}``.
KERNEL_TIMES = None
KERNEL_ROWS = {}   # name -> rows (edge x orientation / node x orientation) handed to the entry point while timing is on


def call(name: str, *args, stream=None, rows: int = 0) -> None:
    """Launch C-ABI entry point ``name`` (of any library) on the current stream; raises on a refused argument (before the launch) and on a
    non-zero status."""
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
