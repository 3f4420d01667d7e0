"""The adaptive KL-penalty PPO objective (geometry_rl_amd.klpen.KLPENPPOLoss, grl_klpen_fwd_bwd, grl_klpen_adapt) on the GPU:
  (a) the kernel against the float64 restatement (tests/klpen_ref.py) at every lane width, on guarded buffers;
  (b) the adapt launch on its three branches, on guarded buffers;
  (c) five consecutive PolicyUpdater updates against the KL-penalty oracle, the beta sequence included, recorded from the third on;
  (d) the recorded programs against the step-by-step loop (lanes, one stream, run_minibatches in both multi-step forms), beta changing
      inside one eight-step launch;
  (e) a host write of beta takes effect at the next replay without recording again;
  (f) two data-parallel ranks against one rank on the whole batch, beta after every step;
  (g) the reference loop protocol (loss_module(td), two backward passes, two Adam steps) against PolicyUpdater.step, beta included;
  (h) the running statistics carry the mode's keys.
torchrl is not installed here: the restatement is UNPINNED (tests/klpen_ref.py)."""
import contextlib
import ctypes
import functools

import pytest
import torch

import oracle_cases as oc
from oracle import trpl as otr
from geometry_rl_amd import synthetic as syn
from klpen_ref import KLPenOracleAgent, klpen_loss, thresholds
from oracle_cases import M_TOL, V_TOL
from updater_cases import (DEV, assert_stats_means, dp_case, dp_ref, make_rollout, moments_and_params_after, run_loop_and_launches,
                           run_stats_epoch, run_step_modes, snapshot, spawn_dp)

pytestmark = pytest.mark.gpu

GUARD = 16            # sentinel words around every output
SENT = 0x7F7F7F7F


def bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------------------------------------------------- (a) kernel
ENT_COEF, CRITIC_COEF = 0.01, 0.5


@functools.lru_cache(maxsize=None)
def _kernel_inputs(A, B):
    """Frames 1, 5, 9, ...: new == old EXACTLY (sigma = k / 64, so sigma^2 is a float32); the others: old mean 0.3 away per dimension, old
    variance 2^u times the new one, u in [-2, 2] (up to 4x either way); advantages of both signs; log weights ~ 0.3 N(0, 1)."""
    g = torch.Generator().manual_seed(100 * A + B)
    loc = torch.randn(B, A, generator=g).float()
    sigma = torch.randint(26, 101, (B, A), generator=g).float() / 64
    var = sigma * sigma
    assert bool((var.double() == sigma.double() ** 2).all())
    same = (torch.arange(B) % 4) == 1
    old_loc = torch.where(same[:, None], loc, loc + 0.3 * torch.randn(B, A, generator=g).float())
    u = 4 * torch.rand(B, A, generator=g) - 2
    u[:, 0] = torch.where(torch.arange(B) % 2 == 0, torch.tensor(2.0), torch.tensor(-2.0))   # both extremes present
    old_var = torch.where(same[:, None], var, (var * torch.exp2(u)).float())
    action = (loc.double() + sigma.double() * torch.randn(B, A, generator=g, dtype=torch.float64)).float()
    lw_t = 0.3 * torch.randn(B, generator=g, dtype=torch.float64)
    logp = (otr.mvn_diag_log_prob(action.double(), loc.double(), var.double()) - lw_t).float()
    adv = torch.randn(B, generator=g).float()
    if B > 1:
        adv[0], adv[1] = abs(adv[0]) + 0.1, -abs(adv[1]) - 0.1
    batch = {"action": action, "loc": old_loc, "var": old_var, "sample_log_prob": logp, "advantage": adv,
             "state_value": torch.randn(B, generator=g).float(), "value_target": torch.randn(B, generator=g).float()}
    value = (batch["state_value"] + 0.4 * torch.randn(B, generator=g)).float()
    return loc, sigma, batch, value, same


@functools.lru_cache(maxsize=None)
def _kernel_reference(A, B, beta):
    loc, sigma, batch, value, _ = _kernel_inputs(A, B)
    loc_r, sig_r, val_r = (t.double().requires_grad_(True) for t in (loc, sigma, value))
    ref = klpen_loss(loc_r, sig_r ** 2, {k: v.double() for k, v in batch.items()}, val_r, float(beta), entropy_coef=ENT_COEF,
                     critic_coef=CRITIC_COEF)
    d_loc, d_sig = torch.autograd.grad(ref["loss_objective"] + ref["loss_entropy"], [loc_r, sig_r])
    (d_val,) = torch.autograd.grad(ref["loss_critic"], [val_r])
    return {k: v.detach() for k, v in ref.items()}, d_loc, d_sig, d_val


@functools.lru_cache(maxsize=None)
def _kernel_run(A, B, beta):
    """grl_klpen_fwd_bwd with every output inside sentinel words -> (sums, maxes, dloc, dsigma, dvalue) on the host; the sentinels kept
    their bits."""
    from geometry_rl_amd import hip
    loc, sigma, batch, value, _ = _kernel_inputs(A, B)
    d = {k: v.to(DEV).contiguous() for k, v in batch.items()}
    n_slot = hip.query("grl_trpl_slot_doubles", B)
    sizes = {"dloc": B * A, "dsigma": B * A, "dvalue": B, "maxes": 2, "beta": 1}
    off, pos = {}, GUARD
    for k, n in sizes.items():
        off[k] = pos
        pos += n + GUARD
    host = torch.full((pos,), SENT, dtype=torch.int32)
    host[off["beta"]] = bits(torch.tensor([float(beta)], dtype=torch.float32))[0]
    buf = host.to(DEV)
    dbl = {"sums": 12, "slots": n_slot}
    doff, dpos = {}, GUARD
    for k, n in dbl.items():
        doff[k] = dpos
        dpos += n + GUARD
    dhost = torch.full((dpos,), -7.0, dtype=torch.float64)
    dbuf = dhost.to(DEV)
    p = lambda k: ctypes.c_void_p(buf.data_ptr() + 4 * off[k])
    q = lambda k: ctypes.c_void_p(dbuf.data_ptr() + 8 * doff[k])
    cfg = (ctypes.c_double * 6)(ENT_COEF, CRITIC_COEF, 0.0, 1.0 / B, float(B), 1.0)
    hip.call("grl_klpen_fwd_bwd", cfg, p("beta"), A, loc.to(DEV), sigma.to(DEV), d["action"], d["loc"], d["var"], d["sample_log_prob"],
             d["advantage"], value.to(DEV), d["state_value"], d["value_target"], p("dloc"), p("dsigma"), p("dvalue"), None, q("sums"),
             p("maxes"), q("slots"), B)
    torch.cuda.synchronize()
    out, dout = buf.cpu(), dbuf.cpu()
    covered = torch.zeros(pos, dtype=torch.bool)
    for k, n in sizes.items():
        if k != "beta":
            covered[off[k]:off[k] + n] = True
    assert torch.equal(out[~covered], host[~covered]), "a word outside the outputs (or beta) was written"
    dcov = torch.zeros(dpos, dtype=torch.bool)
    for k, n in dbl.items():
        dcov[doff[k]:doff[k] + n] = True
    assert torch.equal(dout[~dcov], dhost[~dcov]), "a double outside sums / slots was written"
    f = lambda k, shape: out[off[k]:off[k] + sizes[k]].view(torch.float32).reshape(shape).clone()
    return (dout[doff["sums"]:doff["sums"] + 12].clone(), out[off["maxes"]:off["maxes"] + 2].clone(), f("dloc", (B, A)), f("dsigma", (B, A)),
            f("dvalue", (B,)))


@pytest.mark.parametrize("beta", [0.0, 1.0, 4.0])
@pytest.mark.parametrize("B", [1, 16, 89])
@pytest.mark.parametrize("A", [3, 6, 12])
def test_kernel_matches_the_restatement(A, B, beta):
    """Tolerances of the sibling PPO test (the same fp64 kernel arithmetic on float32 inputs and outputs): 1e-5 relative on the means,
    1e-5 of the gradient's largest entry on dloc, dsigma, dvalue."""
    _, _, _, _, same = _kernel_inputs(A, B)
    ref, d_loc, d_sig, d_val = _kernel_reference(A, B, beta)
    s, maxes, dloc, dsigma, dvalue = _kernel_run(A, B, beta)
    n = float(s[10])
    assert n == B
    got = {"loss_objective": float(s[0]) / n, "entropy": float(s[2]) / n, "entropy_col8": float(s[8]) / n, "loss_critic": float(s[3]) / n,
           "kl": float(s[11]) / n}
    want = {"loss_objective": float(ref["loss_objective"]), "entropy": float(ref["entropy"]), "entropy_col8": float(ref["entropy"]),
            "loss_critic": float(ref["loss_critic"]), "kl": float(ref["kl"])}
    for k in got:
        print(f"A={A} B={B} beta={beta} {k}: {got[k]!r} want {want[k]!r}")
        assert abs(got[k] - want[k]) <= 1e-5 * max(1.0, abs(want[k])), (k, got[k], want[k])
    for col in (1, 6, 7, 9):   # trust-region columns stay zero, and both maxes
        assert float(s[col]) == 0.0, col
    assert maxes.tolist() == [0, 0]
    if B > 1:
        assert int(same.sum()) >= 1 and float(ref["kl_f"][same].abs().max()) == 0.0 and float(ref["kl_f"][~same].min()) > 0.0
    for name, a, b in (("dloc", dloc, d_loc), ("dsigma", dsigma, d_sig), ("dvalue", dvalue, d_val)):
        err = float((a.double() - b).abs().max())
        scale = float(b.abs().max())
        print(f"A={A} B={B} beta={beta} {name}: max err {err:.3e} of scale {scale:.3e}")
        assert err <= 1e-5 * scale, (name, err, scale)
    if beta and B > 1:   # new == old: the KL term adds exactly nothing to the gradient; elsewhere beta is in it
        _, _, dloc0, dsigma0, _ = _kernel_run(A, B, 0.0)
        assert torch.equal(dloc[same], dloc0[same]) and torch.equal(dsigma[same], dsigma0[same])
        assert not torch.equal(dloc[~same], dloc0[~same])


# ------------------------------------------------------------------------------------------------------------- (b) adapt
@pytest.mark.parametrize("factor,want", [(2.0, 2.0), (1.0, 1.0), (0.4, 0.5)])
def test_adapt_launch(factor, want):
    """kl = 2x, 1x, 0.4x dtarg -> beta x2, unchanged, x0.5 exactly; no other word of the report or around beta changes."""
    from geometry_rl_amd import ops
    dtarg, beta0 = 0.01, 3.0
    g = torch.Generator().manual_seed(5)
    host = torch.full((14 + 1 + 3 * GUARD,), SENT, dtype=torch.int32)
    rep = torch.randn(14, generator=g)
    rep[5] = factor * dtarg
    host[GUARD:GUARD + 14] = bits(rep)
    ob = 2 * GUARD + 14
    host[ob] = bits(torch.tensor([beta0]))[0]
    buf = host.to(DEV).view(torch.float32)
    ops.klpen_adapt(buf[GUARD:GUARD + 14], buf[ob:ob + 1], dtarg, 2.0, 0.5)
    torch.cuda.synchronize()
    out = bits(buf.cpu())
    assert float(out[ob:ob + 1].view(torch.float32)) == beta0 * want
    keep = torch.ones(host.numel(), dtype=torch.bool)
    keep[ob] = False
    assert torch.equal(out[keep], host[keep])


# ------------------------------------------------------------------------------------------------------------- (c) vs oracle
def _fields(B, A, seed, spread):
    """syn.make_ppo_fields with the old means drawn ``spread`` wide: the old distribution's KL to a fresh policy (mean ~ 0, variance ~ 1)
    grows with spread^2, which is how the steps of one case land on different sides of the thresholds."""
    f = syn.make_ppo_fields(B, A, seed=seed)
    g = torch.Generator().manual_seed(seed + 31)
    loc = spread * f["loc"]
    action = loc + f["var"].sqrt() * torch.randn(B, A, generator=g)
    f.update(loc=loc, action=action, sample_log_prob=otr.mvn_diag_log_prob(action, loc, f["var"]))
    return f


# objective/kl_ppo.yaml: critic_coef 1.0, entropy_coef 0.0; train.py clips the gradient norm
KL_KW = dict(algorithm="kl_ppo", critic_coef=1.0, entropy_coef=0.0, clip_grad_norm=True, max_grad_norm=1.0)
SPREADS = (1.0, 1.0, 0.55, 0.25, 0.25)
# dtarg per case, chosen from the ORACLE's mean KL of the five steps (float32, CPU; printed by oracle_sequence below), so that the first two
# steps lie above 1.5 dtarg, the third between the thresholds and the last two below dtarg / 1.5, each at least 5 % away:
#   rigid_g1 (A = 6)   kl = 3.139, 3.398, 0.997, 0.315, 0.322   thresholds (0.667, 1.5)   nearest margin 34 %
#   cloth    (A = 12)  kl = 6.283, 6.600, 2.122, 0.614, 0.707   thresholds (1.333, 3.0)   nearest margin 29 %
#   empn_g2  (A = 6)   kl = 3.126, 3.317, 1.070, 0.308, 0.353   thresholds (0.667, 1.5)   nearest margin 29 %
# beta: 1 -> 2 -> 4 -> 4 -> 2 -> 1 in every case
DTARG = {"rigid_g1": 1.0, "cloth": 2.0, "empn_g2": 1.0}


def oracle_sequence(name, B, K, dtarg):
    """The oracle's side of (c), CPU only: -> everything the GPU side needs."""
    from geometry_rl_amd import agent
    oc.cap_oracle_threads()
    o_spec, spec, kw, _ = oc.make_case(name, B)
    cfg = agent.AgentConfig(**dict(kw, dtarg=dtarg, **KL_KW))
    o_cfg, a_par, c_par, oracle = oc.make_oracle(o_spec, dict(kw, critic_coef=1.0, entropy_coef=0.0, clip_grad_norm=True), 21, KLPenOracleAgent)
    oracle.dtarg = dtarg
    A = spec.num_actuators * cfg.output_dim_vec * 3
    batches = []
    for i in range(K):
        b = dict(oc.obs_of(name, B, 30 + i))
        b.update(_fields(B, A, 40 + i, SPREADS[i]))
        batches.append(b)
    with torch.no_grad():
        oracle.actor_forward({k: batches[0][k] for k in o_spec.in_features}, calibrate=True)
    calibrated = {k: v.detach().clone() for k, v in oracle.actor.items()}
    steps = [oracle.update(b) for b in batches]
    return o_spec, spec, o_cfg, cfg, a_par, c_par, calibrated, batches, steps, oracle


@pytest.mark.parametrize("name,B,K", [("rigid_g1", 64, 5), ("cloth", 16, 5), ("empn_g2", 32, 5)])
def test_five_updates_match_the_klpen_oracle(name, B, K):
    from geometry_rl_amd import agent
    dtarg = DTARG[name]
    o_spec, spec, o_cfg, cfg, a_par, c_par, calibrated, batches, steps, oracle = oracle_sequence(name, B, K, dtarg)
    hi, lo = thresholds(dtarg)
    kls = [float(ref["kl"]) for ref, _ in steps]
    betas = [ref["beta"] for ref, _ in steps] + [steps[-1][0]["beta_next"]]
    print(f"{name}: oracle kl {kls}, thresholds ({lo}, {hi}), beta {betas}")
    for kl in kls:   # no step within 5 % of a threshold: the float32 decision cannot differ between the two sides
        assert abs(kl - hi) >= 0.05 * hi and abs(kl - lo) >= 0.05 * lo, (kl, lo, hi)
    moves = [b1 / b0 for b0, b1 in zip(betas[:-1], betas[1:])]
    assert 2.0 in moves and 0.5 in moves, moves   # beta rises and falls within the five steps
    pair = oc.Pair(o_spec, spec, o_cfg, cfg, oracle, *oc.make_device(spec, cfg, a_par, c_par, DEV))
    loss = pair.loss
    assert pair.proj is None and loss.algorithm == "kl_ppo"
    oc.adopt_calibration(pair, weights=calibrated)
    upd = agent.PolicyUpdater(loss, lr=cfg.lr, clip_grad_norm=cfg.clip_grad_norm, max_grad_norm=cfg.max_grad_norm, use_graph=True)

    def beta_is(i):   # in front of update i the device holds the beta the oracle ran that update with
        assert float(loss.beta) == steps[i][0]["beta"], (i, float(loss.beta), steps[i][0]["beta"])

    def per_step(i, out, ref):
        assert set(out) >= {"loss_objective", "loss_critic", "kl", "entropy", "loss_entropy"} and "ESS" not in out
        assert float(loss.beta) == ref["beta_next"], (i, float(loss.beta), ref["beta_next"])   # x2 and x0.5 are exact
        for k in ("loss_objective", "loss_critic", "loss_entropy", "entropy", "kl"):
            e = abs(float(out[k]) - float(ref[k]))
            assert e <= 1e-4 * max(1.0, abs(float(ref[k]))), (i, k, e)
        if i + 1 < K:
            beta_is(i + 1)
    beta_is(0)
    g_scale = oc.run_updates(pair, batches, upd, per_step, refs=steps)
    assert upd.mode.startswith("graph") and upd._program is not None
    bad, _ = moments_and_params_after(upd, pair.actor, pair.critic, oracle, cfg, g_scale, K, M_TOL, V_TOL)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------- (d), (e), (h)
# the synthetic rollout's old distribution lies KL ~ 3 from the fresh policy (A = 6, old means ~ N(0, 1)); on the odd time steps the old
# means are drawn 0.1 wide instead (KL ~ 0.2): a minibatch of 8 random rows reports between the two, on either side of the thresholds
ROLLOUT_KW = dict(KL_KW, clip_grad_norm=False, dtarg=1.0)
KEYS = ("loss_objective", "loss_critic", "kl", "entropy", "loss_entropy")


def _make(N, T, seed, **kw):
    r = make_rollout(N, T, seed=seed, **dict(ROLLOUT_KW, **kw))
    r.data["loc"][:, 1::2] *= 0.1
    return r


@contextlib.contextmanager
def _keep_beta(store, mode, r, upd):
    yield
    store[mode] = r.loss.beta.detach().clone()


@pytest.mark.parametrize("form", ["unrolled", "per_step"])
def test_run_minibatches_equals_the_step_loop(form):
    N, T, U = 8, 10, 8
    betas = {}
    res = run_loop_and_launches(lambda: _make(N, T, 33), form, N=N, T=T, ppo_epochs=2, driver_seed=9, unroll=U, keys=KEYS,
                                per_mode=functools.partial(_keep_beta, betas))
    for a, b in zip(res["loop"][:3], res["launches"][:3]):
        assert torch.equal(a, b), (a - b).abs().max().item()
    for k in KEYS:   # the last update's loss dict
        assert torch.equal(res["loop"][3][-1][k], res["launches"][3][-1][k]), k
    assert torch.equal(betas["loop"], betas["launches"]), (betas["loop"], betas["launches"])
    # beta changed INSIDE the first eight-step launch (steps 1 .. 8 of the loop: step 0 runs eagerly), i.e. behind one of its first seven steps
    hi, lo = thresholds(ROLLOUT_KW["dtarg"])
    kls = [float(o["kl"]) for o in res["loop"][3]]
    moved = [j for j in range(1, U) if kls[j] > hi or kls[j] < lo]
    print(f"{form}: kl {kls}, beta changes behind steps {moved} of the first launch, final beta {float(betas['loop'])}")
    assert moved
    assert float(betas["loop"]) != 1.0


def test_recorded_programs_equal_the_eager_loop():
    """Eager steps, the recorded lanes program and the one-stream program over the same four updates: a replayed program is its eager
    form bit for bit, beta included; the one-stream program sums the advantage statistics in another launch (last bits)."""
    betas = {}
    res = run_step_modes(lambda: _make(8, 2, 41), ("eager", "graph", "one_stream", "one_stream_eager"), 4, KEYS,
                         lambda mode: dict(use_graph=mode in ("graph", "one_stream"), overlap_critic=not mode.startswith("one_stream")),
                         per_mode=functools.partial(_keep_beta, betas))
    for a, b in (("eager", "graph"), ("one_stream_eager", "one_stream")):
        for x, y in zip(res[a][:3], res[b][:3]):
            assert torch.equal(x, y), (a, b, (x - y).abs().max().item())
        for oa, ob in zip(res[a][3], res[b][3]):
            for kk in KEYS:
                assert torch.equal(oa[kk], ob[kk]), (a, b, kk)
        assert torch.equal(betas[a], betas[b])
    assert (res["graph"][0] - res["one_stream"][0]).abs().max().item() <= 1e-6
    assert torch.equal(betas["graph"], betas["one_stream"]) and float(betas["graph"]) != 1.0


def test_host_write_of_beta_takes_effect_on_replay():
    from geometry_rl_amd import agent
    N, T = 8, 4
    res = {}
    for mode in ("graph", "eager", "graph_unwritten"):
        r = _make(N, T, 51)
        loss = r.loss
        upd = agent.PolicyUpdater(loss, lr=r.cfg.lr, use_graph=mode != "eager")
        ptr = loss.beta.data_ptr()
        prog = None
        outs, betas = [], []
        for t in range(T):
            if t == 2:
                prog = upd._program
                assert (prog is not None) == (mode != "eager")
                if mode != "graph_unwritten":
                    loss.beta.fill_(0.125)
            outs.append({k: v.clone() for k, v in upd.step({kk: v[:, t].contiguous() for kk, v in r.data.items()}).items() if k in KEYS})
            betas.append(float(loss.beta))
        torch.cuda.synchronize()
        if mode == "graph":
            assert upd._program is prog and loss.beta.data_ptr() == ptr   # replayed, not recorded again
        res[mode] = (upd.flat.detach().clone(), outs, betas)
    assert (res["graph"][0] - res["eager"][0]).abs().max().item() <= 1e-7
    assert res["graph"][2] == res["eager"][2]
    for oa, ob in zip(res["graph"][1], res["eager"][1]):
        for k in KEYS:
            assert abs(float(oa[k]) - float(ob[k])) <= 1e-6 * max(1.0, abs(float(ob[k]))), k
    # the write was read: the replay behind it reports another objective than the replay without it, and beta continues from 0.125
    assert not torch.equal(res["graph"][1][2]["loss_objective"], res["graph_unwritten"][1][2]["loss_objective"])
    assert res["graph"][2][2] in (0.0625, 0.125, 0.25) and res["graph"][2] != res["graph_unwritten"][2]


def test_replacing_the_beta_buffer_records_again():
    from geometry_rl_amd import agent
    r = _make(8, 4, 52)
    upd = agent.PolicyUpdater(r.loss, lr=r.cfg.lr, use_graph=True)
    for t in range(3):
        upd.step({kk: v[:, t].contiguous() for kk, v in r.data.items()})
    prog = upd._program
    assert prog is not None
    r.loss.beta = torch.tensor(0.5, device=DEV)   # a new tensor, not an in-place write
    upd.step({kk: v[:, 3].contiguous() for kk, v in r.data.items()})
    assert upd._program is not prog
    assert float(r.loss.beta) in (0.25, 0.5, 1.0)


def test_statistics_carry_the_modes_keys():
    """track_stats through the multi-step launches: the keys of klpen.report_dict plus loss_objective and loss_critic, their means those
    of the per-step reports, the update bitwise the one without tracking; the iteration log carries train/kl and train/kl_beta."""
    from geometry_rl_amd.rollout import RolloutDriver
    cfg_kw = dict(algorithm="kl_ppo", dtarg=1.0)
    ref_upd, ref_r, _, vals = run_stats_epoch("launches", False, cfg_kw, KEYS)
    upd, r, buf, _ = run_stats_epoch("launches", True, cfg_kw, KEYS)
    assert_stats_means(upd.stats_read(), vals, KEYS)
    for a, b in zip(snapshot(upd, None)[:3], snapshot(ref_upd, None)[:3]):
        assert torch.equal(a, b), float((a - b).abs().max())
    assert torch.equal(r.loss.beta, ref_r.loss.beta)
    log = RolloutDriver(upd, r.spec, ppo_epochs=1).iteration_log(buf)
    assert {f"train/{k}" for k in KEYS} <= set(log) and log["train/kl_beta"] == float(r.loss.beta) and "train/ESS" not in log


# ------------------------------------------------------------------------------------------------------------- (f) data parallel
DP_STEPS = 3
DP_KW = dict(KL_KW, dtarg=1.0)


@contextlib.contextmanager
def _record_beta(case, upd, shard, rank, ret):
    """Around a rank's updates (updater_cases.dp_worker): beta as every step leaves it."""
    betas = []
    step = upd.step

    def recording_step(batch):
        out = step(batch)
        betas.append(float(case.loss.beta))
        return out
    upd.step = recording_step
    yield None
    ret[f"beta{rank}"] = betas


def test_two_ranks_match_single_rank():
    from geometry_rl_amd import agent
    world = 2
    case = dp_case(16, None, cfg_kw=DP_KW)
    upd = agent.PolicyUpdater(case.loss, lr=case.cfg.lr, use_graph=True, clip_grad_norm=True)
    ref_betas = []
    for _ in range(DP_STEPS):
        out = upd.step(case.batch)
        ref_betas.append(float(case.loss.beta))
    ref_losses, ref_flat = {k: float(out[k].detach()) for k in KEYS}, upd.flat.detach().cpu()
    ret = spawn_dp(dp_ref(16, cfg_kw=DP_KW), world, use_graph=True, n_steps=DP_STEPS, keys=KEYS, updater_kw=dict(clip_grad_norm=True),
                   extra=(__name__, "_record_beta"))
    from updater_cases import assert_ranks_match
    assert_ranks_match(ref_losses, ref_flat, ret, world, 1e-5, 2e-6)
    print("beta after every step: one rank", ref_betas, "two ranks", ret["beta0"], ret["beta1"])
    assert ret["beta0"] == ret["beta1"] == ref_betas and ref_betas[-1] != 1.0


# ------------------------------------------------------------------------------------------------------------- (g) reference loop
@pytest.mark.parametrize("model", ["hepi", "transformer"])
def test_reference_loop_protocol_matches_the_updater(model):
    """examples/torchrl/train.py:279-316 with algorithm=kl_ppo on the loss module itself, against PolicyUpdater.step on a copy."""
    from geometry_rl_amd import agent, graph
    B = 32
    spec = graph.rigid_spec()
    kw = dict(model="transformer", output_dim=2, output_dim_vec=2) if model == "transformer" else \
        dict(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2)
    cfg = agent.AgentConfig(**dict(kw, dtarg=1.0, **KL_KW))
    batch = dict(syn.make_rigid_obs(B, seed=61))
    batch.update(syn.make_ppo_fields(B, 6, seed=61))
    batch = {k: v.to(DEV) for k, v in batch.items()}
    sides = []
    for _ in range(2):
        torch.manual_seed(5)
        actor, critic, proj, loss = agent.build_agent(spec, cfg, device=DEV)
        with torch.no_grad():
            actor.forward_diag(*[batch[k] for k in loss.in_features], train=True)   # calibration (HEPi), identical on both sides
        sides.append((actor, critic, loss))
    actor, critic, loss = sides[0]
    a_par = [p for p in actor.parameters() if p.requires_grad]
    c_par = [p for p in critic.parameters() if p.requires_grad]
    a_opt = torch.optim.Adam(a_par, lr=cfg.lr, eps=1e-5)
    c_opt = torch.optim.Adam(c_par, lr=cfg.lr, eps=1e-5)
    ref, ref_betas = [], []
    for _ in range(2):
        out = loss(dict(batch))
        assert set(loss.out_keys) <= set(out.keys()) and "ESS" not in out.keys()
        ref.append({k: float(out[k].detach()) for k in KEYS})
        ref_betas.append(float(loss.beta))
        critic_loss = out["loss_critic"]
        actor_loss = out["loss_objective"]
        actor_loss += out["loss_entropy"]
        actor_loss.backward()
        critic_loss.backward()
        torch.nn.utils.clip_grad_norm_(a_par, cfg.max_grad_norm)
        torch.nn.utils.clip_grad_norm_(c_par, cfg.max_grad_norm)
        a_opt.step()
        c_opt.step()
        a_opt.zero_grad()
        c_opt.zero_grad()
    actor2, critic2, loss2 = sides[1]
    upd = agent.PolicyUpdater(loss2, lr=cfg.lr, clip_grad_norm=True, max_grad_norm=cfg.max_grad_norm)
    got, got_betas = [], []
    for _ in range(2):
        o = upd.step(dict(batch))
        got.append({k: float(o[k]) for k in KEYS})
        got_betas.append(float(loss2.beta))
    for r, g_ in zip(ref, got):
        for k in KEYS:
            assert abs(r[k] - g_[k]) <= 1e-5 * max(1.0, abs(r[k])), (k, r[k], g_[k])
    assert ref_betas == got_betas and ref_betas[-1] != 1.0, (ref_betas, got_betas)
    worst = 0.0
    for (n1, p1), (n2, p2) in zip(list(actor.named_parameters()) + list(critic.named_parameters()),
                                  list(actor2.named_parameters()) + list(critic2.named_parameters())):
        assert n1 == n2
        worst = max(worst, float((p1.detach() - p2.detach()).abs().max()))
    print(f"{model}: max |param(reference loop) - param(updater)| = {worst:.3e}")
    assert worst <= 2e-5
