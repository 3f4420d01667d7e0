#!/usr/bin/env python3
"""What ``PolicyUpdater(track_stats=True)`` costs per replayed policy-update step: rigid_insertion_multi HEPi (the bench.py workload), the
recorded lanes program, tracking off and on in ONE process (the protocol of tools/entropy_step_bench.py).

Both updaters are built from the same seed and record their step; blocks of --steps replays of each are timed with HIP events on the
caller's stream (both lanes joined at every block boundary), ALTERNATING and with the order reversed every round (off on | on off | ...),
so that clock and thermal drift hit both alike.  "on" pays one more launch of a single workgroup at the end of each lane
(grl_stats_accumulate).  Prints the box calibration (bench.py's two fixed kernels) and one JSON line per minibatch size: the median and the
spread of the per-block ms / step of each, and on / off -- once with the "off" updater built first and once with the "on" updater built first.

  python tools/track_stats_bench.py --sizes 32 512 4096 --steps 20 --blocks 8
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(track, B, dev):
    from geometry_rl_amd import agent, graph, synthetic as syn
    spec = graph.rigid_spec()
    cfg = agent.AgentConfig(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2)   # the bench.py workload
    torch.manual_seed(0)
    actor, critic, proj, loss = agent.build_agent(spec, cfg, device=dev)
    batch = dict(syn.make_rigid_obs(B, seed=1))
    batch.update(syn.make_ppo_fields(B, spec.num_actuators * cfg.output_dim_vec * 3, seed=1))
    batch = {k: v.to(dev) for k, v in batch.items()}
    with torch.no_grad():
        actor.forward_diag(*[batch[k] for k in loss.in_features], train=True)   # calibration
    return agent.PolicyUpdater(loss, lr=cfg.lr, use_graph=True, track_stats=track), batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[32, 512, 4096])
    ap.add_argument("--steps", type=int, default=20, help="replays per timed block")
    ap.add_argument("--blocks", type=int, default=8, help="timed blocks per setting (alternating, order reversed every round)")
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    import bench
    print(json.dumps({"box_calibration": {k: v for k, v in bench.box_calibration(dev).items() if k != "what"}}), flush=True)
    # (both build orders: tools/entropy_step_bench.py saw the updater built SECOND in a process run 3.6 % slower at 4096 frames whatever it ran)
    for B, first in [(B, first) for B in a.sizes for first in ("off", "on")]:
        runs = {k: make(k == "on", B, dev) for k in ((first, "on") if first == "off" else (first, "off"))}
        plain = runs["off"][0].program_outline()
        for upd, batch in runs.values():
            for _ in range(a.warmup):
                upd.step(batch)
            assert upd._program is not None, "the step was not recorded"
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for r in range(a.blocks):
            for k in (("off", "on") if r % 2 == 0 else ("on", "off")):
                upd, batch = runs[k]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.current_stream().wait_stream(upd._critic_stream())
                e0.record()
                for _ in range(a.steps):
                    upd.step(batch)
                torch.cuda.current_stream().wait_stream(upd._critic_stream())
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.steps)
        means = runs["on"][0].stats_read()
        assert means["updates"] == a.warmup + a.blocks * a.steps, means["updates"]
        med = {k: statistics.median(t) for k, t in times.items()}
        graphs = {k: sum(e.kind == "graph" for e in runs[k][0]._program) for k in runs}
        print(json.dumps({"frames": B, "built_first": first, "steps_per_block": a.steps, "blocks": a.blocks,
                          **{f"{k}_ms_per_step": round(med[k], 4) for k in med},
                          **{f"{k}_min_max_ms": [round(min(t), 4), round(max(t), 4)] for k, t in times.items()},
                          "on_over_off": round(med["on"] / med["off"], 4), "on_minus_off_us": round((med["on"] - med["off"]) * 1e3, 2),
                          "graphs_per_step": graphs, "outline_unchanged_by_tracking": plain == runs["on"][0].program_outline()}), flush=True)


if __name__ == "__main__":
    main()
