"""Footprint checks for the kernels behind ``geometry_rl_amd.ops``: every output and workspace on poisoned, guarded memory.  TEST
INFRASTRUCTURE ONLY, a plain module like tests/actor_cases.py; it works on any device (tests/test_footprint_cpu.py shows on CPU tensors
that each check notices what it is for) and changes no production file.

``Guarded(poison)`` swaps the name ``torch`` as seen from inside ``geometry_rl_amd.ops`` and ``geometry_rl_amd.graph`` for a proxy that
forwards every attribute to the real module except ``empty`` and ``empty_like`` (and ``zeros`` / ``zeros_like`` / ``full``, below).  The replacement allocates ``numel + 2 G`` elements,
fills ALL of them with the poison and hands back the middle as a contiguous view of the requested shape and dtype; the ledger keeps
(base, view).  ``guard(t, poison)`` does the same for a tensor the test built itself (an input, an upstream gradient, an index array).
``ledger.check(results, inputs)`` then asserts
  (a) every guard word of every interposed and wrapped buffer kept its bits (a write past either end),
  (b) every wrapped input kept its bits,
  (c) no element of a result still holds the poison's bit pattern and every result is finite (an element nobody wrote, a workspace row
      the fold read but no workgroup wrote, a read past the end of an input that reached the result),
  (d) at least one allocation was interposed (a proxy that silently is not in the path fails the test).

The guard width G is at least 4096 elements and at least one leading-dimension row of the tensor (numel / shape[0]): a stray write of a
whole row, tile or partial row still lands in a guard.  G * itemsize is a multiple of 256 bytes, so the view keeps the alignment a plain
allocation has and the kernels take the same code path.

Two poisons, one per run.  NAN: a quiet NaN with a recognisable payload (fp32 0x7fc0dead, bf16 0x7fdd, fp64 0x7ff80000deadbeef).  HUGE: a
huge finite number (fp32 +3.0e38, its bf16 rounding, fp64 1e300) -- a max, a min or a compare drops a NaN, so a read past the end that
feeds a softmax maximum is invisible under the NaN poison and visible under the finite one.  Integer and byte buffers are filled with a
fixed byte, 0xa5 in the NAN run and 0xc3 in the HUGE run (negative in every signed type: not an index; two bytes, so that a word of a
byte buffer nobody wrote differs between the two runs while a written one does not -- ``unwritten_words``).

Index arrays the test wraps (``guard(t, poison, index_of=v)``) get the VALUE ``v`` in their guard words instead of a poison, chosen so
that a stray read of a guard word, used as an index or a run bound, stays inside the guard regions of the buffers it indexes and lands on
poison there -- nothing may leave the allocations:
  * an array indexing the n rows of a node tensor (``src_*`` / ``dst_*``, the node boundaries ``split_*``): v = n, the first guard row
    behind the tensor (the rule for G guarantees that row exists);
  * ``s2d``, indexing the E rows of the per-edge gradient: v = E;
  * a ``rowptr`` over E edges: v = E + 1, i.e. one phantom edge E whose endpoints are the guard words of the edge arrays.
``guard_edge_set`` applies these to an ``ops.EdgeSet``.

Buffers a kernel updates IN PLACE (optimiser state, running statistics, a destination that is accumulated into) go through
``inout(t, poison)`` / ``ledger.inout(t)``: the value in the middle of a poisoned buffer like ``guard``, but exempt from (b) -- the kernel
is meant to change it.  Its guards are held by (a); the caller lists it among the results, so (c) and the bitwise comparison see it (a
buffer the test STARTS from the poison, ``poisoned(...)``, shows every element nobody wrote).  The proxy also replaces ``zeros``,
``zeros_like`` and ``full``: a guarded allocation whose view holds the requested fill and whose guards hold the poison -- the buffers
kernels write in place are mostly born that way (the flat parameter / gradient / moment buffers, step counters, learning-rate tables).
They count as interposed for (d).

``Plain`` / ``Wrapped`` / ``three_runs`` are the harness the GPU files share: one case run plain, under ``Guarded(NAN)`` and under
``Guarded(HUGE)`` from identical inputs, both ledgers checked, every result of both guarded runs bitwise the plain run's."""
import dataclasses
import math
from math import gcd

import torch

MIN_GUARD = 4096
NAN, HUGE = "nan", "huge"
POISONS = (NAN, HUGE)
INT_BYTE = {NAN: 0xA5, HUGE: 0xC3}
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_NAN_BITS = {torch.float32: 0x7FC0DEAD, torch.bfloat16: 0x7FDD, torch.float64: 0x7FF80000DEADBEEF}
_HUGE = {torch.float32: 3.0e38, torch.bfloat16: 3.0e38, torch.float64: 1e300}


def bits_view(t):
    """``t`` reinterpreted as integers of its element size (NaN-safe bitwise comparisons)."""
    return t.view(_BITS[t.element_size()])


def _signed(v, itemsize):
    """The unsigned bit pattern ``v`` as the value the integer view of that size holds (uint8 stays unsigned)."""
    n = 8 * itemsize
    return v - (1 << n) if itemsize > 1 and v >= 1 << (n - 1) else v


def poison_bits(dtype, poison):
    """The poison's bit pattern for ``dtype`` as the value ``bits_view`` shows."""
    assert poison in POISONS, poison
    size = torch.empty(0, dtype=dtype).element_size()
    if dtype in _NAN_BITS:
        if poison == NAN:
            return _signed(_NAN_BITS[dtype], size)
        return int(bits_view(torch.tensor([_HUGE[dtype]], dtype=torch.float64).to(dtype))[0])
    if dtype.is_floating_point or dtype.is_complex:
        raise TypeError(f"footprint: no poison for {dtype}")
    return _signed(int.from_bytes(bytes([INT_BYTE[poison]]) * size, "little"), size)


def guard_width(shape, dtype):
    shape = tuple(int(s) for s in shape)
    row = math.prod(shape[1:]) if len(shape) > 0 else 1
    size = torch.empty(0, dtype=dtype).element_size()
    unit = 256 // gcd(256, size)
    return (max(MIN_GUARD, row) + unit - 1) // unit * unit


def flatten(x, prefix=""):
    """[(name, tensor)] of a tensor / None / (nested) dict, list or tuple of them."""
    if x is None:
        return []
    if torch.is_tensor(x):
        return [(prefix or "result", x)]
    if isinstance(x, dict):
        return [p for k, v in x.items() for p in flatten(v, f"{prefix}.{k}" if prefix else str(k))]
    if isinstance(x, (list, tuple)):
        return [p for i, v in enumerate(x) for p in flatten(v, f"{prefix}[{i}]")]
    raise TypeError(f"footprint: {type(x)} in the results")


class _Entry:
    __slots__ = ("kind", "base", "view", "G", "numel", "pattern", "orig")


class Ledger:
    """What one guarded run allocated through the proxy (``interposed``) and what the test wrapped itself (``wrapped``)."""

    def __init__(self, poison):
        assert poison in POISONS, poison
        self.poison = poison
        self.entries = []

    @property
    def interposed(self):
        return sum(e.kind == "interposed" for e in self.entries)

    @property
    def wrapped(self):
        """Buffers the test wrapped itself: inputs and in/out buffers."""
        return sum(e.kind in ("wrapped", "inout") for e in self.entries)

    @property
    def inouts(self):
        return sum(e.kind == "inout" for e in self.entries)

    def _buffer(self, kind, shape, dtype, device, pattern, shift=0):
        """``shift``: the view starts this many elements past the 256-byte boundary a plain allocation starts on (a destination that
        is a slice at an odd offset of a larger buffer: the kernels' scalar paths); the front guard is that much wider."""
        shape = tuple(int(s) for s in shape)
        numel, G = math.prod(shape), guard_width(shape, dtype)
        assert 0 <= shift < MIN_GUARD, shift
        base = torch.empty(numel + 2 * G + shift, dtype=dtype, device=device)
        bits_view(base).fill_(pattern)
        assert (G * base.element_size()) % 256 == 0
        G += shift
        view = base[G:G + numel].view(shape)
        assert view.is_contiguous() and view.storage_offset() == G
        e = _Entry()
        e.kind, e.base, e.view, e.G, e.numel, e.pattern, e.orig = kind, base, view, G, numel, pattern, None
        self.entries.append(e)
        return e

    def allocate(self, shape, dtype, device, fill=None):
        """The proxy's ``empty``; with ``fill`` its ``zeros`` / ``full``: the view holds the fill, the guards the poison."""
        view = self._buffer("interposed", shape, dtype, device, poison_bits(dtype, self.poison)).view
        return view if fill is None else view.fill_(fill)

    def guard(self, t, index_of=None):
        """``t`` in the middle of a poisoned buffer of the same layout (detached; the caller sets requires_grad).  ``index_of``: ``t`` is
        an integer index array and its guard words hold this value (module docstring)."""
        t = t.detach().contiguous()
        if index_of is None:
            pattern = poison_bits(t.dtype, self.poison)
        else:
            assert not t.dtype.is_floating_point and int(index_of) >= 0, (t.dtype, index_of)
            pattern = int(index_of)
        e = self._buffer("wrapped", t.shape, t.dtype, t.device, pattern)
        e.view.copy_(t)
        e.orig = t.clone()
        return e.view

    def inout(self, t, shift=0):
        """``t`` in the middle of a poisoned buffer like ``guard``, for a buffer the kernel changes in place: no (b) for it.  The caller
        lists the returned view among the results.  ``shift``: see ``_buffer``."""
        t = t.detach().contiguous()
        e = self._buffer("inout", t.shape, t.dtype, t.device, poison_bits(t.dtype, self.poison), shift)
        e.view.copy_(t)
        return e.view

    def check(self, results, inputs=(), direct=False):
        """(a) .. (d) of the module docstring; ``results``: what the op returned and every gradient it produced (nested dicts / lists
        / tuples, None entries skipped); ``inputs``: wrapped tensors of this ledger the caller wants looked at by name -- every wrapped
        buffer is checked either way, a tensor listed here that the ledger never wrapped is an error.  ``direct``: the test
        called the entry point itself and handed it every buffer, so no allocating wrapper is in the path and (d) asks instead that the
        ledger holds at least one buffer the kernel writes (taken with ``allocate`` or ``inout``)."""
        if direct:
            assert any(e.kind in ("interposed", "inout") for e in self.entries), "(d) the ledger holds no buffer the kernel writes"
        else:
            assert self.interposed >= 1, "(d) no allocation went through the proxy: the interposer is not in the op's path"
        mine = {e.view.data_ptr() for e in self.entries if e.kind in ("wrapped", "inout") and e.numel}
        for name, t in flatten(inputs):
            assert t.numel() == 0 or t.data_ptr() in mine, f"(b) input {name} was not wrapped by this ledger"
        for e in self.entries:
            what = f"{e.kind} buffer of shape {tuple(e.view.shape)}, {e.view.dtype}"
            for side, part in (("front", e.base[:e.G]), ("back", e.base[e.G + e.numel:])):
                bad = bits_view(part) != e.pattern
                if bool(bad.any()):
                    off = int(bad.nonzero()[0])
                    where = f"{e.G - off} element(s) in front of the first" if side == "front" else f"{off} element(s) behind the last"
                    raise AssertionError(f"(a) guard words changed: {what}, {side} guard, first at offset {off} of {e.G} ({where}), "
                                         f"{int(bad.sum())} in all")
            if e.orig is not None and e.numel:
                bad = bits_view(e.view.reshape(-1)) != bits_view(e.orig.reshape(-1))
                if bool(bad.any()):
                    raise AssertionError(f"(b) a wrapped input was modified: {what}, first at element {int(bad.nonzero()[0])}, "
                                         f"{int(bad.sum())} in all")
        for name, t in flatten(results):
            if t.numel() == 0:
                continue
            flat = t.detach().contiguous().reshape(-1)
            if t.dtype.is_floating_point:
                held = bits_view(flat) == poison_bits(t.dtype, self.poison)
                unit = "element"
            else:   # byte and integer results: whole 32-bit words of the fill (a byte image may hold the fill's byte legitimately)
                size = flat.element_size()
                words = flat.view(torch.int32) if size < 4 and (flat.numel() * size) % 4 == 0 and flat.data_ptr() % 4 == 0 else flat
                held = words == poison_bits(words.dtype, self.poison)
                unit = f"{words.element_size()}-byte word"
            if bool(held.any()):
                raise AssertionError(f"(c) result {name} {tuple(t.shape)} {t.dtype} still holds the poison: {int(held.sum())} {unit}(s), "
                                     f"first at {int(held.nonzero()[0])}")
            if t.dtype.is_floating_point and not bool(torch.isfinite(flat).all()):
                bad = ~torch.isfinite(flat)
                raise AssertionError(f"(c) result {name} {tuple(t.shape)} {t.dtype} is not finite: {int(bad.sum())} element(s), "
                                     f"first at {int(bad.nonzero()[0])}")


class _TorchProxy:
    """``torch`` with ``empty`` / ``empty_like`` replaced by guarded, poisoned allocations and ``zeros`` / ``zeros_like`` / ``full`` by
    guarded allocations that hold the requested fill between poisoned guards."""

    def __init__(self, real, ledger):
        self.__dict__["_real"], self.__dict__["_ledger"] = real, ledger

    def __getattr__(self, name):
        return getattr(self.__dict__["_real"], name)

    def _sized(self, name, size, dtype, device, requires_grad, kw, fill=None):
        if kw:
            raise TypeError(f"footprint: torch.{name}({', '.join(kw)}=...) is not interposed")
        if len(size) == 1 and isinstance(size[0], (tuple, list)):   # (torch.Size is a tuple)
            size = tuple(size[0])
        real = self.__dict__["_real"]
        out = self.__dict__["_ledger"].allocate(size, dtype if dtype is not None else real.get_default_dtype(),
                                                real.device(device) if device is not None else real.device("cpu"), fill)
        return out.requires_grad_(True) if requires_grad else out

    def _like(self, name, t, dtype, device, kw, fill=None):
        if kw:
            raise TypeError(f"footprint: torch.{name}({', '.join(kw)}=...) is not interposed")
        return self.__dict__["_ledger"].allocate(t.shape, dtype if dtype is not None else t.dtype, device if device is not None else t.device,
                                                 fill)

    def empty(self, *size, dtype=None, device=None, requires_grad=False, **kw):
        return self._sized("empty", size, dtype, device, requires_grad, kw)

    def empty_like(self, t, dtype=None, device=None, **kw):
        return self._like("empty_like", t, dtype, device, kw)

    def zeros(self, *size, dtype=None, device=None, requires_grad=False, **kw):
        return self._sized("zeros", size, dtype, device, requires_grad, kw, fill=0)

    def zeros_like(self, t, dtype=None, device=None, **kw):
        return self._like("zeros_like", t, dtype, device, kw, fill=0)

    def full(self, size, fill_value, dtype=None, device=None, requires_grad=False, **kw):
        if dtype is None:   # torch.full's own inference from the fill value
            real = self.__dict__["_real"]
            dtype = real.bool if isinstance(fill_value, bool) else real.int64 if isinstance(fill_value, int) else real.get_default_dtype()
        return self._sized("full", (size,), dtype, device, requires_grad, kw, fill=fill_value)


_ACTIVE = []


def default_modules():
    from geometry_rl_amd import graph, ops
    return (ops, graph)


class Guarded:
    """``with Guarded(poison) as ledger:`` -- inside the block ``torch.empty`` / ``empty_like`` / ``zeros`` / ``zeros_like`` / ``full``
    called from ``modules`` (default: geometry_rl_amd.ops and geometry_rl_amd.graph) allocate guarded buffers recorded in ``ledger`` (poisoned,
    or holding the requested fill between poisoned guards); nothing outside those modules sees the proxy, and the real module is back when the block ends, however it ends."""

    def __init__(self, poison, modules=None):
        self.ledger = Ledger(poison)
        self.modules = tuple(modules) if modules is not None else default_modules()
        self._saved = []

    def __enter__(self):
        for m in self.modules:   # (refused before anything is swapped: a block that fails to start leaves no proxy behind)
            assert not isinstance(m.torch, _TorchProxy), f"{m.__name__} is already guarded"
        for m in self.modules:
            real = m.torch
            self._saved.append((m, real))
            m.torch = _TorchProxy(real, self.ledger)
        _ACTIVE.append(self.ledger)
        return self.ledger

    def __exit__(self, *exc):
        _ACTIVE.remove(self.ledger)
        while self._saved:
            m, real = self._saved.pop()
            m.torch = real
        return False


def guard(t, poison, index_of=None):
    """Wrap ``t`` in the ledger of the innermost active ``Guarded`` block (whose poison must be ``poison``)."""
    assert _ACTIVE, "guard() outside a Guarded block"
    assert _ACTIVE[-1].poison == poison, (_ACTIVE[-1].poison, poison)
    return _ACTIVE[-1].guard(t, index_of)


def inout(t, poison):
    """``Ledger.inout`` in the ledger of the innermost active ``Guarded`` block (whose poison must be ``poison``)."""
    assert _ACTIVE, "inout() outside a Guarded block"
    assert _ACTIVE[-1].poison == poison, (_ACTIVE[-1].poison, poison)
    return _ACTIVE[-1].inout(t)


def poisoned(shape, dtype, device, poison):
    """A plain tensor every element of which holds the poison's bit pattern: what a test starts an in/out buffer from when the kernel has
    to write all of it (an overwritten destination) -- an element nobody wrote is then reported by (c)."""
    t = torch.empty(shape, dtype=dtype, device=device)
    bits_view(t).fill_(poison_bits(dtype, poison))
    return t


def guard_edge_set(es, wrap):
    """``ops.EdgeSet`` with every index array wrapped by ``wrap(t, index_of=...)`` (the values of the module docstring)."""
    E = es.n_edges
    new = dict(rowptr_d=wrap(es.rowptr_d, index_of=E + 1), rowptr_s=wrap(es.rowptr_s, index_of=E + 1),
               src_d=wrap(es.src_d, index_of=es.n_src), src_s=wrap(es.src_s, index_of=es.n_src),
               dst_d=wrap(es.dst_d, index_of=es.n_dst), dst_s=wrap(es.dst_s, index_of=es.n_dst))
    if es.s2d is not None:
        new["s2d"] = wrap(es.s2d, index_of=E)
    if es.split_s is not None:
        new["split_s"] = wrap(es.split_s, index_of=es.n_src)
    if es.split_d is not None:
        new["split_d"] = wrap(es.split_d, index_of=es.n_dst)
    return dataclasses.replace(es, **new)


def same_bits(a, b):
    """Names of the results that differ bitwise between two runs (both flattened the same way)."""
    fa, fb = flatten(a), flatten(b)
    assert [n for n, _ in fa] == [n for n, _ in fb], ([n for n, _ in fa], [n for n, _ in fb])
    bad = []
    for (n, x), (_, y) in zip(fa, fb):
        if x.shape != y.shape or x.dtype != y.dtype or (x.numel() and not torch.equal(bits_view(x.detach().contiguous().reshape(-1)),
                                                                                       bits_view(y.detach().contiguous().reshape(-1)))):
            bad.append(n)
    return bad


def unwritten_words(plain, nan_run, huge_run):
    """For a byte buffer whose layout leaves holes on purpose (the weight images are LDS structs: bank padding, unused halves): the three
    runs' buffers as 32-bit words -> the number of words NOBODY wrote.  Asserts that every word either holds the same bits in all three runs
    (written, deterministically) or holds each guarded run's own fill (never written); anything else is a word written from memory the
    producer does not own."""
    a, b, c = (t.detach().contiguous().reshape(-1).view(torch.int32) for t in (plain, nan_run, huge_run))
    assert a.shape == b.shape == c.shape
    hole = (b == poison_bits(torch.int32, NAN)) & (c == poison_bits(torch.int32, HUGE))
    stray = ~hole & ((a != b) | (a != c))
    assert not bool(stray.any()), f"{int(stray.sum())} word(s) are neither the same in all three runs nor unwritten, first at {int(stray.nonzero()[0])}"
    return int(hole.sum())


# ------------------------------------------------------------------------------------------------ the run harness of the GPU files
COUNTS = {}   # op -> [guarded runs, interposed allocations, wrapped buffers] of this process


class Plain:
    """The wrapper of the plain run: fresh copies, plain allocations."""
    poison = None

    def __call__(self, t, index_of=None):
        return t.detach().clone()

    def out(self, shape, dtype, device):
        return torch.zeros(shape, dtype=dtype, device=device)

    def inout(self, t, shift=0):
        """A buffer the kernel changes in place: a fresh copy (``shift`` elements past a plain allocation's start, as the guarded one)."""
        t = t.detach().contiguous()
        out = torch.zeros(t.numel() + shift, dtype=t.dtype, device=t.device)[shift:].view(t.shape)
        return out.copy_(t)

    def fresh(self, shape, dtype, device, shift=0):
        """An in/out buffer the kernel has to write in full (an overwritten destination): any contents do for the plain run."""
        return self.inout(torch.zeros(shape, dtype=dtype, device=device), shift)


class Wrapped:
    """The wrapper of a guarded run: inputs through ``ledger.guard``, buffers the kernel writes through ``ledger.allocate``, buffers it
    changes in place through ``ledger.inout``."""

    def __init__(self, ledger):
        self.ledger, self.poison = ledger, ledger.poison

    def __call__(self, t, index_of=None):
        return self.ledger.guard(t, index_of)

    def out(self, shape, dtype, device):
        return self.ledger.allocate(shape, dtype, device)

    def inout(self, t, shift=0):
        return self.ledger.inout(t, shift)

    def fresh(self, shape, dtype, device, shift=0):
        return self.ledger.inout(poisoned(shape, dtype, device, self.poison), shift)


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def three_runs(op, label, run, image_holes=None, modules=None, direct=False):
    """``run(w)`` -> results (nested dicts / lists of tensors); ``w`` wraps every tensor the run hands to an op.  An entry "images" of the
    results (weight images: byte buffers whose layout has holes on purpose) is held to ``unwritten_words`` and to ``image_holes`` (image
    name -> the layout's own count of never-written words) instead of (c) and the bitwise comparison; what the kernels compute FROM the
    images is among the other results.  ``modules``: those of ``Guarded``; ``direct``: that of ``Ledger.check``.  -> the plain run's
    results."""
    def split(res):
        res = dict(res)
        return res, res.pop("images", None) or {}
    plain, images = split(run(Plain()))
    _sync()
    guarded_images = []
    for poison in POISONS:
        with Guarded(poison, modules) as ledger:
            res, img = split(run(Wrapped(ledger)))
            _sync()
        ledger.check(res, direct=direct)
        bad = same_bits(plain, res)
        assert not bad, f"{op} {label}: under the {poison} poison these results are not bitwise the plain run's: {bad}"
        guarded_images.append(img)
        tot = COUNTS.setdefault(op, [0, 0, 0])
        tot[0], tot[1], tot[2] = tot[0] + 1, tot[1] + ledger.interposed, tot[2] + ledger.wrapped
        print(f"footprint {op} {label} [{poison}]: {ledger.interposed} interposed allocations, {ledger.wrapped} wrapped inputs "
              f"(so far for {op}: {tot[0]} guarded runs, {tot[1]} interposed, {tot[2]} wrapped)")
    for m, v in images.items():
        holes = unwritten_words(v, guarded_images[0][m], guarded_images[1][m])
        print(f"footprint {op} {label}: image {m}: {holes} of {v.numel() // 4} words are never written (padding / unused halves)")
        assert image_holes is not None and holes == image_holes[m], (m, holes)
    plain["images"] = images
    return plain
