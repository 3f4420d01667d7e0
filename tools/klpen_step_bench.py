#!/usr/bin/env python3
"""Replayed policy-update step, KL-penalty PPO (KLPENPPOLoss) against clipped PPO (ClipPPOLoss2), rigid_insertion_multi HEPi, in ONE process.

Both updaters are built from the same seed and record their step (lanes program, use_graph=True); then blocks of --steps replays of each are
timed with HIP events on the caller's stream, ALTERNATING (PPO, KL-PPO, PPO, KL-PPO, ...) so that clock and thermal drift hit both alike.
The two steps differ by the mode of the fused loss launch and by ONE single-thread launch per step on the actor's lane (grl_klpen_adapt).
Prints one JSON line per minibatch size: the median and the spread of the per-block ms / step and steps / s of each, KL-PPO / PPO, and the
number of C-ABI entry-point calls the host issues for one step of each while the step is recorded (torch's own launches are not counted;
they are the same on both sides).

  python tools/klpen_step_bench.py --sizes 512 4096 --steps 20 --blocks 7
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(algorithm, B, dev):
    from geometry_rl_amd import agent, graph, synthetic as syn
    spec = graph.rigid_spec()
    cfg = agent.AgentConfig(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2, algorithm=algorithm,   # the bench.py workload
                            dtarg=2.0 if algorithm == "kl_ppo" else None)   # (the fields' mean KL is ~3: all three branches of the rule occur)
    torch.manual_seed(0)
    actor, critic, proj, loss = agent.build_agent(spec, cfg, device=dev)
    batch = dict(syn.make_rigid_obs(B, seed=1))
    batch.update(syn.make_ppo_fields(B, spec.num_actuators * cfg.output_dim_vec * 3, seed=1))
    batch = {k: v.to(dev) for k, v in batch.items()}
    with torch.no_grad():
        actor.forward_diag(*[batch[k] for k in loss.in_features], train=True)   # calibration
    return agent.PolicyUpdater(loss, lr=cfg.lr, use_graph=True), batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--steps", type=int, default=20, help="replays per timed block")
    ap.add_argument("--blocks", type=int, default=7, help="timed blocks per algorithm (alternating)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--kl-first", action="store_true", help="build and time the KL-penalty updater FIRST (the updater built second in a "
                    "process has measured slower at 4096 frames whatever it runs: INTEGRATION.md, entropy control)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for B in a.sizes:
        from geometry_rl_amd import hip
        runs = {alg: make(alg, B, dev) for alg in (("kl_ppo", "ppo") if a.kl_first else ("ppo", "kl_ppo"))}
        calls = {}
        for alg, (upd, batch) in runs.items():
            upd.step(batch)                       # the first step of a size runs eagerly
            n, real = [0], hip.call

            def counting(*args, _n=n, _real=real, **kw):
                _n[0] += 1
                return _real(*args, **kw)
            hip.call = counting
            try:
                upd.step(batch)                   # the step is recorded: every launch of the program is issued once
            finally:
                hip.call = real
            calls[alg] = n[0]
            for _ in range(a.warmup):
                upd.step(batch)
            assert upd._program is not None, "the step was not recorded"
        torch.cuda.synchronize()
        times = {alg: [] for alg in runs}
        for _ in range(a.blocks):
            for alg, (upd, batch) in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.current_stream().wait_stream(upd._critic_stream())
                e0.record()
                for _ in range(a.steps):
                    upd.step(batch)
                torch.cuda.current_stream().wait_stream(upd._critic_stream())
                e1.record()
                e1.synchronize()
                times[alg].append(e0.elapsed_time(e1) / a.steps)
        med = {alg: statistics.median(t) for alg, t in times.items()}
        print(json.dumps({"frames": B, "built_first": next(iter(runs)), "steps_per_block": a.steps, "blocks": a.blocks,
                          **{f"{alg}_ms_per_step": round(med[alg], 4) for alg in med},
                          **{f"{alg}_min_max_ms": [round(min(t), 4), round(max(t), 4)] for alg, t in times.items()},
                          **{f"{alg}_steps_per_s": round(1000.0 / med[alg], 1) for alg in med},
                          **{f"{alg}_entry_point_calls_per_step": calls[alg] for alg in calls},
                          "kl_ppo_over_ppo": round(med["kl_ppo"] / med["ppo"], 4),
                          "kl_ppo_minus_ppo_us": round(1000.0 * (med["kl_ppo"] - med["ppo"]), 2)}), flush=True)


if __name__ == "__main__":
    main()
