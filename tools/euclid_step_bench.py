#!/usr/bin/env python3
"""Replayed TRPL policy-update step with the commutative Wasserstein projection (w2) in its precision-scaled form (scale_prec=True,
kernel code 2) against its Euclidean form (scale_prec=False, code 7), rigid_insertion_multi HEPi, in ONE process (the protocol of
tools/ppo_step_bench.py).

Both updaters are built from the same seed and record their step (lanes program, use_graph=True); then blocks of --steps replays of each are
timed with HIP events on the caller's stream, ALTERNATING (scaled, euclid, scaled, ...) so that clock and thermal drift hit both alike.
Prints one JSON line per minibatch size: the median and the spread of the per-block ms / step of each, and euclid / scaled.

  python tools/euclid_step_bench.py --sizes 512 4096 --steps 20 --blocks 7
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(scale_prec, B, dev):
    from geometry_rl_amd import agent, graph, synthetic as syn
    spec = graph.rigid_spec()
    cfg = agent.AgentConfig(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2, proj_type="w2",
                            scale_prec=scale_prec)   # the bench.py workload
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
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for B in a.sizes:
        runs = {alg: make(flag, B, dev) for alg, flag in (("scaled", True), ("euclid", False))}
        for upd, batch in runs.values():
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
        print(json.dumps({"frames": B, "steps_per_block": a.steps, "blocks": a.blocks,
                          **{f"{alg}_ms_per_step": round(med[alg], 4) for alg in med},
                          **{f"{alg}_min_max_ms": [round(min(t), 4), round(max(t), 4)] for alg, t in times.items()},
                          "euclid_over_scaled": round(med["euclid"] / med["scaled"], 4)}), flush=True)


if __name__ == "__main__":
    main()
