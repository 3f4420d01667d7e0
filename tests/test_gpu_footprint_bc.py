"""The behaviour-cloning launch (grl_trpl_fwd_bwd in modes 8 / 9 through ops.bc_fwd_bwd) and one eager ``BCUpdater`` update on poisoned,
guarded buffers (tests/footprint.py), as tests/test_gpu_footprint_train.py runs the other objectives: every case three times from identical
inputs -- plain, under ``Guarded(NAN)`` and under ``Guarded(HUGE)`` -- every input wrapped, every output, workspace and scratch from the
ledger.  Asserted: guards untouched, inputs unmodified, no poisoned element in any output (mode 8's dsigma included: it is written, as
zeros) and every result BITWISE the plain run's; the float64 comparisons stay in tests/test_gpu_bc_ops.py, whose cases these are."""
import pytest
import torch

import bc_ref
import footprint as fp
import trpl_cases as tc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, F64, I32 = torch.float32, torch.float64, torch.int32


def out(w, n, dtype=F32):
    return w.out(n if isinstance(n, tuple) else (n,), dtype, DEV)


def run_bc(B, A, mode):
    from geometry_rl_amd import hip, ops
    d = {k: v.to(DEV) for k, v in bc_ref.make_case(B, A).items()}

    def run(w, defer):
        sums, maxes, dloc, dsigma = ops.bc_fwd_bwd(w(d["loc"]), w(d["sigma"]), w(d["action"]), mode=mode, global_batch=B, defer_fold=defer)
        res = {"launch": [maxes, dloc, dsigma] if defer else [sums, maxes, dloc, dsigma]}
        if defer:   # the slots through the fused report and through the fold
            s, m, o14 = out(w, 12, F64), out(w, 2, I32), out(w, 14)
            hip.call("grl_trpl_report", sums.slots, B, s, m, 0.0, o14)
            res["report"] = [s, m, o14]
            sums, maxes = sums()
            res["fold"] = [sums, maxes]
        o14 = out(w, 14)
        hip.call("grl_trpl_loss_values", sums, maxes, 0.0, o14)
        res["values"] = o14
        return res

    for defer in (False, True):
        plain = fp.three_runs("bc_fwd_bwd", f"{mode} B={B} A={A} defer={int(defer)}", lambda w: run(w, defer))
        if mode == "mse":
            assert not bool(plain["launch"][-1].any())


@pytest.mark.parametrize("mode", ("mse", "nll"))
@pytest.mark.parametrize("A", tc.A_SWEEP)
def test_lane_widths(A, mode):
    """A over A_SWEEP at B = 37: three workgroups, the last with five frames, 0 .. 15 padding lanes."""
    run_bc(37, A, mode)


@pytest.mark.parametrize("mode", ("mse", "nll"))
@pytest.mark.parametrize("B", (1, 16, 17, 4097))
def test_batch_and_fold_edges(B, mode):
    run_bc(B, 6, mode)


@pytest.mark.parametrize("objective,clip", [("mse", False), ("nll", False), ("nll", True)])
def test_one_eager_update(objective, clip, monkeypatch):
    """One eager ``BCUpdater.step`` at B = 12 on rigid_tiny from a fresh seeded agent, with the proxy in every module of the update path:
    the flat parameter / gradient / moment buffers, the step counter, the learning rate and the running sums are born guarded."""
    from geometry_rl_amd import agent, bc, graph, hip, ops, policy, synthetic as syn, trpl, updater
    from oracle_cases import make_case
    B = 12
    _, spec, kw, obs = make_case("rigid_tiny", B)
    cfg = agent.AgentConfig(**kw)
    batch = dict(obs)
    batch["action"] = syn.make_ppo_fields(B, spec.num_actuators * cfg.output_dim_vec * 3, seed=B)["action"]
    dbatch = {k: v.to(DEV) for k, v in batch.items()}
    launched = []
    real = hip.call
    monkeypatch.setattr(hip, "call", lambda entry, *a, **k: (launched.append(entry), real(entry, *a, **k))[1])

    def run(w):
        torch.manual_seed(3)
        actor = agent.build_agent(spec, cfg, device=DEV)[0]
        upd = bc.BCUpdater(bc.BCLoss(actor, objective=objective), clip_grad_norm=clip, use_graph=False)
        res = upd.step({k: (w(v) if v.is_floating_point() else v) for k, v in dbatch.items()})
        torch.cuda.synchronize()
        return {"gradient": upd.gflat, "parameters": upd.flat, "exp_avg": upd.exp_avg, "exp_avg_sq": upd.exp_avg_sq,
                "report": {k: v for k, v in res.items() if torch.is_tensor(v)}, "stats": upd.stats, "lr": upd.lr_dev, "steps": upd.step_dev}

    plain = fp.three_runs("eager BC update", f"{objective} clip={int(clip)}", run, modules=(ops, graph, updater, trpl, agent, policy, bc))
    assert bool(plain["gradient"].abs().max() > 0) and bool(plain["exp_avg_sq"].abs().max() > 0) and int(plain["steps"]) == 1
    assert float(plain["stats"][14]) == 1.0 and float(plain["stats"][0]) == float(plain["report"]["loss_bc"])
    names = sorted(set(launched))
    print(f"eager BC update {objective} clip={int(clip)}: entry points launched: {names}")
    for want in ("grl_trpl_fwd_bwd", "grl_stats_accumulate", "grl_clip_coef" if clip else "grl_fold_adam_report_sig"):
        assert want in names, (want, names)
