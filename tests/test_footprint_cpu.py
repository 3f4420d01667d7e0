"""tests/footprint.py on CPU tensors: small Python stand-ins for a kernel, each with one seeded mistake, and the check of the ledger that
has to report it.  The stand-ins allocate through this module's ``torch.empty`` / ``torch.empty_like`` as the ops do through theirs; the
block guards this module beside the two production modules."""
import sys

import pytest
import torch

import footprint as fp

ROWS, COLS = 6, 8
BOTH = pytest.mark.parametrize("poison", fp.POISONS)


def guarded(poison):
    return fp.Guarded(poison, modules=fp.default_modules() + (sys.modules[__name__],))


def raw(t):
    """The storage behind a guarded view, as a flat tensor, and the view's offset in it (how a kernel sees memory: a pointer)."""
    flat = torch.tensor([], dtype=t.dtype).set_(t.untyped_storage())
    return flat, t.storage_offset()


def select_max(rows):
    """Running maximum by compare-and-select, as a kernel's fmaxf does it: a NaN never wins the compare and is dropped."""
    m = rows[0]
    for r in rows[1:]:
        m = torch.where(r > m, r, m)
    return m


def standin(x, mistake=None, dtype=torch.float32):
    """y[r] = 2 x[r] + sum over the workspace rows (one per input row: x[r] summed over its columns, a "per-workgroup partial");
    -> (y [ROWS, COLS], total [1])."""
    y = torch.empty_like(x, dtype=dtype)
    part = torch.empty(ROWS, 1, dtype=dtype)
    total = torch.empty(1, dtype=dtype)
    n_y = ROWS - 1 if mistake == "last_row_unwritten" else ROWS
    y[:n_y] = 2 * x[:n_y].to(dtype)
    n_p = ROWS - 1 if mistake == "workspace_row_unwritten" else ROWS
    part[:n_p] = x[:n_p].to(dtype).sum(1, keepdim=True)
    total[0] = part.sum()   # the fold reads every row
    if mistake == "one_past_the_end":
        flat, off = raw(y)
        flat[off + y.numel()] = 1.0
    elif mistake == "row_in_front":
        flat, off = raw(y)
        flat[off - COLS:off] = 1.0
    elif mistake in ("sum_reads_guard", "max_reads_guard"):
        flat, off = raw(x)
        rows = flat[off:off + (ROWS + 1) * COLS].view(ROWS + 1, COLS)   # one row too many
        total[0] = rows.to(dtype).sum() if mistake == "sum_reads_guard" else select_max(list(rows.to(dtype).reshape(-1)))
    elif mistake == "modifies_input":
        x[2, 3] += 1
    return y, total


def run(poison, mistake, dtype=torch.float32):
    x = torch.randn(ROWS, COLS, generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(dtype)
    with guarded(poison) as ledger:
        xg = ledger.guard(x)
        res = standin(xg, mistake, dtype)
    assert ledger.interposed == 3 and ledger.wrapped == 1
    return ledger, res, xg


@BOTH
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_a_correct_standin_passes(poison, dtype):
    ledger, res, xg = run(poison, None, dtype)
    ledger.check(res, [xg])
    assert torch.equal(res[0], 2 * xg)


@BOTH
@pytest.mark.parametrize("mistake,side,where", [("one_past_the_end", "back", "0 element\\(s\\) behind the last"),
                                                ("row_in_front", "front", f"{COLS} element\\(s\\) in front of the first")])
def test_a_write_outside_the_output_is_reported_by_the_guard_check(poison, mistake, side, where):
    ledger, res, xg = run(poison, mistake)
    with pytest.raises(AssertionError, match=rf"\(a\) guard words changed: interposed buffer of shape \({ROWS}, {COLS}\), torch.float32, "
                                             rf"{side} guard.*{where}"):
        ledger.check(res, [xg])


@BOTH
def test_an_unwritten_output_row_is_reported_by_the_result_check(poison):
    ledger, res, xg = run(poison, "last_row_unwritten")
    with pytest.raises(AssertionError, match=rf"\(c\) result \[0\].*still holds the poison: {COLS} element\(s\), first at {(ROWS - 1) * COLS}"):
        ledger.check(res, [xg])


@BOTH
def test_an_unwritten_workspace_row_reaches_the_result(poison):
    """The sum over the partial rows reads the poison: NaN under the one, an overflow past every finite value's reach under the other."""
    ledger, res, xg = run(poison, "workspace_row_unwritten")
    with pytest.raises(AssertionError, match=r"\(c\) result \[1\]"):
        ledger.check(res, [xg])
    if poison == fp.HUGE:
        assert float(res[1]) > 1e38


@BOTH
def test_a_sum_over_an_inputs_guard_is_reported(poison):
    ledger, res, xg = run(poison, "sum_reads_guard")
    with pytest.raises(AssertionError, match=r"\(c\) result \[1\]"):
        ledger.check(res, [xg])


def test_a_max_over_an_inputs_guard_needs_the_finite_poison():
    """Why there are two poisons: the compare drops the NaN, so the NaN run sees nothing; the huge finite value wins the max."""
    ledger, res, xg = run(fp.NAN, "max_reads_guard")
    ledger.check(res, [xg])
    assert float(res[1]) == float(xg.max())
    ledger, res, xg = run(fp.HUGE, "max_reads_guard")
    with pytest.raises(AssertionError, match=r"\(c\) result \[1\].*still holds the poison"):
        ledger.check(res, [xg])


@BOTH
def test_a_modified_input_is_reported(poison):
    ledger, res, xg = run(poison, "modifies_input")
    with pytest.raises(AssertionError, match=rf"\(b\) a wrapped input was modified: wrapped buffer.*first at element {2 * COLS + 3}, 1 in all"):
        ledger.check(res, [xg])


@BOTH
def test_an_inactive_proxy_and_an_unwrapped_input_are_reported(poison):
    x = torch.randn(ROWS, COLS)
    with fp.Guarded(poison) as ledger:   # this module is not guarded here: the stand-in allocates plain memory
        res = standin(x)
    with pytest.raises(AssertionError, match=r"\(d\) no allocation went through the proxy"):
        ledger.check(res)
    ledger, res, xg = run(poison, None)
    with pytest.raises(AssertionError, match=r"\(b\) input \[0\] was not wrapped"):
        ledger.check(res, [x])


def test_the_proxy_is_gone_after_the_block_also_after_an_exception():
    from geometry_rl_amd import graph, ops
    me = sys.modules[__name__]
    with guarded(fp.NAN) as ledger:
        assert all(isinstance(m.torch, fp._TorchProxy) for m in (ops, graph, me))
        assert ops.torch.float32 is torch.float32 and ops.torch.autograd is torch.autograd
        t = ops.torch.empty(3, 5, dtype=torch.int32)
        u = graph.torch.empty_like(t, dtype=torch.float64)
        assert ledger.interposed == 2 and t.shape == (3, 5) and t.dtype == torch.int32 and u.dtype == torch.float64 and u.is_contiguous()
    assert ops.torch is torch and graph.torch is torch and me.torch is torch
    with pytest.raises(ZeroDivisionError):
        with guarded(fp.HUGE):
            assert ops.torch is not torch
            1 / 0
    assert ops.torch is torch and graph.torch is torch and me.torch is torch and not fp._ACTIVE
    with pytest.raises(AssertionError, match="outside a Guarded block"):
        fp.guard(torch.zeros(2), fp.NAN)


@BOTH
@pytest.mark.parametrize("dtype,shape", [(torch.float32, (5, 3)), (torch.bfloat16, (3, 16, 64)), (torch.float64, (7,)), (torch.int32, (9,)),
                                         (torch.uint8, (1000,)), (torch.float32, (2, 5000)), (torch.float32, (0, 16, 64)), (torch.float32, ())])
def test_guard_width_alignment_and_fill(poison, dtype, shape):
    ledger = fp.Ledger(poison)
    v = ledger.allocate(shape, dtype, "cpu")
    e = ledger.entries[0]
    row = 1
    for s in shape[1:]:
        row *= s
    assert e.G >= max(4096, row) and (e.G * v.element_size()) % 256 == 0 and e.base.numel() == v.numel() + 2 * e.G
    assert v.shape == shape and v.dtype == dtype and v.is_contiguous() and v.storage_offset() == e.G
    assert bool((fp.bits_view(e.base) == fp.poison_bits(dtype, poison)).all()), "the whole buffer is poisoned, the view included"
    if dtype.is_floating_point:
        assert bool(torch.isnan(e.base).all()) if poison == fp.NAN else bool((e.base.double() > 2.9e38).all() and torch.isfinite(e.base).all())
    else:
        assert dtype == torch.uint8 or bool((e.base < 0).all()), "integer fills are negative: not an index"


def test_index_guards_hold_the_given_value_and_edge_sets_keep_their_arrays():
    from geometry_rl_amd import ops
    ei = torch.tensor([[0, 2, 2, 1, 0], [1, 1, 0, 3, 3]])
    es = ops.build_edge_set(ei, 3, 4)
    with fp.Guarded(fp.NAN) as ledger:
        gs = fp.guard_edge_set(es, lambda t, index_of: fp.guard(t, fp.NAN, index_of))
    assert ledger.wrapped == 7
    for name, want in (("rowptr_d", 6), ("rowptr_s", 6), ("src_d", 3), ("src_s", 3), ("dst_d", 4), ("dst_s", 4), ("s2d", 5)):
        e = next(e for e in ledger.entries if e.view.data_ptr() == getattr(gs, name).data_ptr())
        assert torch.equal(getattr(gs, name), getattr(es, name)) and bool((e.base[:e.G] == want).all()) and bool((e.base[-e.G:] == want).all())
    assert (gs.n_src, gs.n_dst, gs.n_edges) == (3, 4, 5)


def test_unwritten_words_tells_holes_from_strays():
    """A byte image with holes on purpose: written words agree in all three runs, holes keep each guarded run's fill; a word copied from
    memory the producer does not own (here: computed from its own unwritten tail) is neither."""
    def image(poison, stray):
        buf = torch.full((64,), 9, dtype=torch.uint8)   # a plain allocation: whatever was there
        if poison is not None:
            with guarded(poison):
                buf = torch.empty(64, dtype=torch.uint8)
        tail = buf[60:64].clone()
        buf[:32] = torch.arange(32, dtype=torch.uint8)
        if stray:
            buf[40:44] = tail // 2
        return buf

    assert fp.unwritten_words(image(None, False), image(fp.NAN, False), image(fp.HUGE, False)) == 8
    with pytest.raises(AssertionError, match="1 word\\(s\\) are neither the same in all three runs nor unwritten, first at 10"):
        fp.unwritten_words(image(None, True), image(fp.NAN, True), image(fp.HUGE, True))


# ------------------------------------------------------------------------------------------------ in/out buffers, zeros / full
def inplace_standin(state, grad, mistake=None):
    """An optimiser-like stand-in: state[i] += grad[i] in place, and a step counter taken from ``torch.zeros`` advanced by one."""
    step = torch.zeros(1, dtype=torch.int32)
    lr = torch.full((1,), 0.5)
    n = state.numel() - 1 if mistake == "last_unwritten" else state.numel()
    state[:n] = state[:n].nan_to_num(0.0, 0.0, 0.0) * 0 + lr * grad[:n] if mistake == "last_unwritten" else state[:n] + lr * grad[:n]
    step += 1
    flat, off = raw(state)
    if mistake == "one_past_the_end":
        flat[off + state.numel()] = 1.0
    elif mistake == "one_in_front":
        flat[off - 1] = 1.0
    elif mistake == "behind_the_counter":
        sflat, soff = raw(step)
        sflat[soff + 1] = 1
    return step, lr


@BOTH
def test_a_legitimate_in_place_change_of_an_inout_buffer_passes(poison):
    s0, g0 = torch.arange(10.0), torch.ones(10)
    with guarded(poison) as ledger:
        state, grad = fp.inout(s0, poison), fp.guard(g0, poison)
        step, lr = inplace_standin(state, grad)
    assert (ledger.interposed, ledger.wrapped, ledger.inouts) == (2, 2, 1)
    ledger.check({"state": state, "step": step}, [grad, state])
    assert torch.equal(state, s0 + 0.5) and not torch.equal(state, s0), "changed in place, and no (b) for it"
    with pytest.raises(AssertionError, match=r"\(b\) a wrapped input was modified"):   # the same change of a guard()ed buffer is (b)
        with guarded(poison) as other:
            st = other.guard(s0)
            inplace_standin(st, g0)
        other.check({"state": st})


@BOTH
@pytest.mark.parametrize("mistake,where", [("one_past_the_end", "back guard.*0 element\\(s\\) behind the last"),
                                           ("one_in_front", "front guard.*1 element\\(s\\) in front of the first")])
def test_a_write_outside_an_inout_buffer_is_reported_by_the_guard_check(poison, mistake, where):
    with guarded(poison) as ledger:
        state = ledger.inout(torch.arange(10.0))
        step, _ = inplace_standin(state, torch.ones(10), mistake)
    with pytest.raises(AssertionError, match=rf"\(a\) guard words changed: inout buffer of shape \(10,\), torch.float32, {where}"):
        ledger.check({"state": state, "step": step})


@BOTH
def test_an_element_of_an_inout_buffer_nobody_wrote_is_reported_when_it_started_from_the_poison(poison):
    """An overwritten destination: the test starts it from the poison (``fp.poisoned``), the kernel has to write all of it."""
    for mistake in (None, "last_unwritten"):
        with guarded(poison) as ledger:
            state = ledger.inout(fp.poisoned((10,), torch.float32, "cpu", poison))
            assert bool((fp.bits_view(state) == fp.poison_bits(torch.float32, poison)).all())
            step, _ = inplace_standin(state, torch.ones(10), "last_unwritten")
            if mistake is None:
                state[9] = 0.5
        if mistake is None:
            ledger.check({"state": state})
        else:
            with pytest.raises(AssertionError, match=r"\(c\) result state \(10,\) torch.float32 still holds the poison: 1 element\(s\), first at 9"):
                ledger.check({"state": state})


@BOTH
def test_zeros_and_full_get_guards_and_hold_the_requested_fill(poison):
    me = sys.modules[__name__]
    with guarded(poison) as ledger:
        z = me.torch.zeros(3, 5, dtype=torch.int32)
        zl = me.torch.zeros_like(z, dtype=torch.float64)
        f = me.torch.full((7,), 1.5)
        fi = me.torch.full((2, 2), 3)
        zt = me.torch.zeros((4,), requires_grad=True)
        step, lr = inplace_standin(torch.arange(4.0), torch.ones(4), "behind_the_counter")
    assert ledger.interposed == 7 and ledger.wrapped == 0
    assert z.dtype == torch.int32 and z.shape == (3, 5) and bool((z == 0).all()) and zl.dtype == torch.float64 and bool((zl == 0).all())
    assert f.dtype == torch.float32 and bool((f == 1.5).all()) and fi.dtype == torch.int64 and bool((fi == 3).all())
    assert zt.requires_grad and bool((zt == 0).all()) and float(lr) == 0.5 and int(step) == 1
    for e in ledger.entries:
        want = fp.poison_bits(e.view.dtype, poison)
        assert e.G >= 4096 and bool((fp.bits_view(e.base[:e.G]) == want).all())
        assert e is ledger.entries[5] or bool((fp.bits_view(e.base[e.G + e.numel:]) == want).all())
    with pytest.raises(AssertionError, match=r"\(a\) guard words changed: interposed buffer of shape \(1,\), torch.int32, back guard.*"
                                             r"0 element\(s\) behind the last"):
        ledger.check({"z": z, "f": f})
    with guarded(poison) as clean:
        z = me.torch.zeros(3)
    clean.check({"z": z})   # (d): a zero-filled buffer counts as interposed


@BOTH
def test_a_direct_call_needs_a_buffer_the_kernel_writes_in_the_ledger(poison):
    """(d) where the test calls the entry point itself (no allocating wrapper in the path): an output or an in/out buffer of the ledger."""
    with fp.Guarded(poison) as ledger:
        x = ledger.guard(torch.ones(3))
    with pytest.raises(AssertionError, match=r"\(d\) the ledger holds no buffer the kernel writes"):
        ledger.check({"y": torch.ones(3)}, [x], direct=True)
    with fp.Guarded(poison) as ledger:
        state = ledger.inout(torch.ones(3))
        state += 1
    ledger.check({"state": state}, direct=True)
    with pytest.raises(AssertionError, match=r"\(d\) no allocation went through the proxy"):
        ledger.check({"state": state})


def test_modules_passed_to_guarded_are_restored_on_exit_also_after_an_exception():
    from geometry_rl_amd import agent, graph, klpen, ops, policy, ppo, rollout, transforms, trpl, updater
    mods = (ops, graph, updater, trpl, ppo, klpen, agent, policy, transforms, rollout)
    with fp.Guarded(fp.NAN, modules=mods) as ledger:
        assert all(isinstance(m.torch, fp._TorchProxy) for m in mods)
        t = updater.torch.zeros(5)
        u = rollout.torch.full((2,), 7, dtype=torch.int32)
        assert ledger.interposed == 2 and bool((t == 0).all()) and bool((u == 7).all())
    assert all(m.torch is torch for m in mods)
    with pytest.raises(ZeroDivisionError):
        with fp.Guarded(fp.HUGE, modules=mods):
            assert all(m.torch is not torch for m in mods)
            1 / 0
    assert all(m.torch is torch for m in mods) and not fp._ACTIVE
    with pytest.raises(AssertionError, match="is already guarded"):   # a nested block over the same module is refused ...
        with fp.Guarded(fp.NAN, modules=(updater,)):
            with fp.Guarded(fp.NAN, modules=(ops, updater)):
                pass
    assert all(m.torch is torch for m in mods) and not fp._ACTIVE       # ... and leaves nothing behind either


def test_three_runs_on_cpu_tensors_holds_an_inout_buffer_to_the_plain_runs_bits():
    me = sys.modules[__name__]

    def run(w, mistake=None):
        state = w.inout(torch.arange(10.0))
        fresh = w.fresh((10,), torch.float32, "cpu")
        step, _ = inplace_standin(state, w(torch.ones(10)), mistake if w.poison else None)   # (the plain buffer has no room behind it)
        inplace_standin(fresh, w(torch.ones(10)), "last_unwritten")
        fresh[9] = 2.0
        return {"state": state, "fresh": fresh, "step": step}

    plain = fp.three_runs("standin", "cpu", run, modules=(me,))
    assert torch.equal(plain["state"], torch.arange(10.0) + 0.5)
    with pytest.raises(AssertionError, match=r"\(a\) guard words changed: inout buffer"):
        fp.three_runs("standin", "cpu", lambda w: run(w, "one_past_the_end"), modules=(me,))
