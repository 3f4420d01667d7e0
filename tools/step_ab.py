#!/usr/bin/env python3
"""Replayed policy-update step of two named variants, A against B, rigid_insertion_multi HEPi (the bench.py workload), in ONE process.

Both updaters are built from the same seed and record their step (lanes program, use_graph=True); then blocks of --steps replays of each are
timed with HIP events on the caller's stream (both lanes joined at every block boundary), ALTERNATING (A, B, A, B, ...) so that clock and
thermal drift hit both alike.  Prints one JSON line per minibatch size (and build order): the median and the spread of the per-block
ms / step of each (``<variant>_ms_per_step``, ``<variant>_min_max_ms``), B / A (``<b>_over_<a>``) and B - A in microseconds.

  python tools/step_ab.py trpl ppo --sizes 512 4096 --steps 20 --blocks 7
  python tools/step_ab.py ppo kl_ppo --count-calls                    # + C-ABI entry-point calls per recorded step of each
  python tools/step_ab.py trpl track_stats_on --sizes 32 512 4096 --blocks 8 --build-order both --reverse-blocks --graphs --calibration
  python tools/step_ab.py ppo ppo_anneal_on --sizes 32 512 4096 --build-order both --reverse-blocks                    # the per-step program
  python tools/step_ab.py ppo ppo_anneal_on --sizes 32 512 4096 --build-order both --reverse-blocks --launch-steps 8   # the multi-step launch
  python tools/step_ab.py transformer transformer_hip --sizes 64 512 4096 --reverse-blocks --eager --count-calls       # both as eager steps
  python tools/step_ab.py transformer transformer_hip --sizes 64 512 4096 --reverse-blocks                             # the HIP variant replayed
  python tools/step_ab.py hepi_attn hepi_attn_gate_hip --sizes 512 4096 --reverse-blocks --build-order both --calibration --count-calls
  python tools/step_ab.py trpl bc --sizes 4096 --blocks 8 --reverse-blocks --build-order both      # the behaviour-cloning step (bc.BCUpdater)

The updater built SECOND in a process has measured 3.6 % slower at 4096 frames whatever it runs (entropy control): a
difference of that size is read from both build orders (--build-order both) and from blocks whose order is reversed every round."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> keywords on top of the bench.py workload: ``cfg`` for AgentConfig, ``upd`` for PolicyUpdater
VARIANTS = {
    "trpl": {},
    "ppo": dict(cfg=dict(algorithm="ppo")),
    "kl_ppo": dict(cfg=dict(algorithm="kl_ppo", dtarg=2.0)),   # (the fields' mean KL is ~3: all three branches of the rule occur)
    "w2": dict(cfg=dict(proj_type="w2")),                      # (precision-scaled: scale_prec=True, kernel code 2)
    "w2_euclid": dict(cfg=dict(proj_type="w2", scale_prec=False)),   # (kernel code 7)
    "w2_non_com": dict(cfg=dict(proj_type="w2_non_com")),
    # a linear schedule whose bound stays near the policy's entropy level over the run
    "entropy_on": dict(cfg=dict(entropy_schedule="linear", total_train_steps=10 ** 6, target_entropy=8.5)),
    "track_stats_on": dict(upd=dict(track_stats=True)),
    # the per-update schedule of train.py:263-276 over a total no run reaches: lr (yardstick: trpl), lr + clip epsilon (yardstick: ppo)
    "anneal_on": dict(cfg=dict(anneal_lr=True, total_train_steps=10 ** 8)),
    "ppo_anneal_on": dict(cfg=dict(algorithm="ppo", anneal_lr=True, anneal_clip_epsilon=True, total_train_steps=10 ** 8)),
    # the two-agent EMPN update (bench.py's rigid2_empn workload: ``spec`` = rigid_spec / make_rigid_obs keywords, ``base`` replaces the HEPi
    # workload's AgentConfig keywords) without and with the key / query attention of ponita_gcn.yaml's ``attention`` key
    "empn2": dict(spec=dict(G=2), base={}, cfg=dict(model="empn")),
    "empn2_attention": dict(spec=dict(G=2), base={}, cfg=dict(model="empn", attention=True)),
    # BASELINE config 1's transformer actor (rigid, A = 6): stock torch (its step cannot be recorded: it runs eagerly whatever is asked) and
    # on HIP kernels.  Compare them with --eager (both as eager upd.step calls) and once more without (the HIP variant replayed)
    "transformer": dict(base=dict(output_dim=2, output_dim_vec=2), cfg=dict(model="transformer")),
    "transformer_hip": dict(base=dict(output_dim=2, output_dim_vec=2), cfg=dict(model="transformer", transformer_kernels="hip")),
    # hepi_attention.yaml on the bench.py workload: the gate network of the attention convolutions as torch modules (a library GEMM + ReLU
    # under autograd, the accumulate mode of the gradient fold) and inside the softmax-aggregation launches (csrc/grl_gate.h, overwrite mode)
    "hepi_attn": dict(cfg=dict(aggr="AttentionalAggregation")),
    "hepi_attn_gate_hip": dict(cfg=dict(aggr="AttentionalAggregation", attention_gate="hip")),
    # the behaviour-cloning step on the same workload (bc.BCUpdater: the actor's lane alone, no critic, no projection): ``bc`` = BCLoss's objective
    "bc": dict(bc="mse"),
    "bc_nll": dict(bc="nll"),
}
HEPI_BASE = dict(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2)


def make(variant, B, dev, use_graph=True):
    from geometry_rl_amd import agent, graph, synthetic as syn
    spec_kw = VARIANTS[variant].get("spec", {})
    spec = graph.rigid_spec(**spec_kw)
    cfg = agent.AgentConfig(**VARIANTS[variant].get("base", HEPI_BASE), **VARIANTS[variant].get("cfg", {}))
    torch.manual_seed(0)
    actor, critic, proj, loss = agent.build_agent(spec, cfg, device=dev)
    batch = dict(syn.make_rigid_obs(B, seed=1, **spec_kw))
    batch.update(syn.make_ppo_fields(B, spec.num_actuators * cfg.output_dim_vec * 3, seed=1))
    batch = {k: v.to(dev) for k, v in batch.items()}
    with torch.no_grad():
        actor.forward_diag(*[batch[k] for k in loss.in_features], train=True)   # calibration
    if "bc" in VARIANTS[variant]:
        from geometry_rl_amd import bc
        return bc.BCUpdater(bc.BCLoss(actor, objective=VARIANTS[variant]["bc"]), use_graph=use_graph), batch
    return agent.PolicyUpdater(loss, use_graph=use_graph, **dict(agent.updater_kwargs(cfg), **VARIANTS[variant].get("upd", {}))), batch


def launcher(upd, batch, U):
    """-> a callable that issues ONE recorded launch of ``U`` steps (run_minibatches' multi-step form, the critic's lane ungated): the batch
    as a rollout of one time step, every row of the index matrix the whole batch."""
    from geometry_rl_amd.rollout import RolloutBuffer
    buf = RolloutBuffer({k: v.unsqueeze(1) for k, v in batch.items()})
    B = next(iter(batch.values())).shape[0]
    rows = torch.arange(B, device=upd.flat.device).repeat(U, 1)
    key = upd._epoch_key(buf, B, U)
    return lambda: upd._launch_epoch(buf, rows, key, False)


def count_calls(upd, batch):
    """C-ABI entry-point calls the host issues for one step while the step is recorded (every launch of the program is issued once;
    torch's own launches are not counted)."""
    from geometry_rl_amd import hip
    upd.step(batch)                       # the first step of a size runs eagerly
    n, real = [0], hip.call               # the one launch function of every kernel library

    def counting(*args, **kw):
        n[0] += 1
        return real(*args, **kw)
    hip.call = counting
    try:
        upd.step(batch)
    finally:
        hip.call = real
    return n[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a", choices=sorted(VARIANTS))
    ap.add_argument("b", choices=sorted(VARIANTS))
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--steps", type=int, default=20, help="replays per timed block")
    ap.add_argument("--blocks", type=int, default=7, help="timed blocks per variant (alternating)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--build-order", choices=("ab", "ba", "both"), default="ab", help="which updater is built (and timed) first")
    ap.add_argument("--reverse-blocks", action="store_true", help="reverse the order of the two blocks every round (a b | b a | ...)")
    ap.add_argument("--count-calls", action="store_true", help="report the entry-point calls per recorded step of each")
    ap.add_argument("--graphs", action="store_true", help="report the graphs per recorded step of each and whether the outlines are equal")
    ap.add_argument("--calibration", action="store_true", help="print the box calibration (bench.py's two fixed kernels) first")
    ap.add_argument("--launch-steps", type=int, default=0, help="time the multi-step launch of this many steps (a block = --steps launches) "
                    "instead of the per-step program")
    ap.add_argument("--eager", action="store_true", help="time blocks of eager upd.step calls of both variants (nothing recorded)")
    a = ap.parse_args()
    if a.eager and a.launch_steps:
        ap.error("--eager times upd.step calls: no --launch-steps")
    if a.a == a.b:
        ap.error("two different variants")
    dev = torch.device("cuda:0")
    if a.calibration:
        import bench
        print(json.dumps({"box_calibration": {k: v for k, v in bench.box_calibration(dev).items() if k != "what"}}), flush=True)
    orders = {"ab": [(a.a, a.b)], "ba": [(a.b, a.a)], "both": [(a.a, a.b), (a.b, a.a)]}[a.build_order]
    for B, order in [(B, order) for B in a.sizes for order in orders]:
        runs = {v: make(v, B, dev, use_graph=not a.eager) for v in order}
        extra = {}
        if a.count_calls:
            extra.update({f"{v}_entry_point_calls_per_step": count_calls(*runs[v]) for v in order})
        U = max(1, a.launch_steps)
        issue = {}
        for v, (upd, batch) in runs.items():
            upd.step(batch)   # (the first step of a size runs eagerly)
            issue[v] = launcher(upd, batch, U) if a.launch_steps else (lambda upd=upd, batch=batch: upd.step(batch))
            for _ in range(a.warmup):
                issue[v]()
            # (an updater whose mode says "eager" -- asked for with --eager, or the stock-torch transformer actor -- records nothing)
            recorded = upd._epoch if a.launch_steps else (getattr(upd, "_program", None) or getattr(upd, "_programs", None))
            assert not upd.mode.startswith("graph") or recorded, "the step was not recorded"
        torch.cuda.synchronize()
        times = {v: [] for v in order}
        for r in range(a.blocks):
            for v in (order[::-1] if a.reverse_blocks and r % 2 else order):
                upd, batch = runs[v]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                upd.join_lanes()
                e0.record()
                for _ in range(a.steps):
                    issue[v]()
                upd.join_lanes()
                e1.record()
                e1.synchronize()
                times[v].append(e0.elapsed_time(e1) / (a.steps * U))
        for upd, _ in runs.values():
            if getattr(upd, "track_stats", False):
                assert upd.stats_read()["updates"] == upd.steps, (upd.stats_read()["updates"], upd.steps)
        if a.graphs:
            extra["graphs_per_step"] = {v: sum(e.kind == "graph" for e in runs[v][0]._program) for v in order}
            extra["outlines_equal"] = runs[a.a][0].program_outline() == runs[a.b][0].program_outline()
        med = {v: statistics.median(t) for v, t in times.items()}
        print(json.dumps({"frames": B, "built_first": order[0], "steps_per_block": a.steps * U, "steps_per_launch": U, "blocks": a.blocks,
                          **{f"{v}_mode": runs[v][0].mode.split(" ")[0] for v in order},
                          **{f"{v}_ms_per_step": round(med[v], 4) for v in med},
                          **{f"{v}_min_max_ms": [round(min(t), 4), round(max(t), 4)] for v, t in times.items()},
                          # what two identical runs differ by in this process: a variant's even-numbered blocks against its odd-numbered ones
                          **{f"{v}_even_minus_odd_blocks_us": round(1000.0 * (statistics.median(t[0::2]) - statistics.median(t[1::2])), 2)
                             for v, t in times.items() if len(t) > 1},
                          f"{a.b}_over_{a.a}": round(med[a.b] / med[a.a], 4),
                          f"{a.b}_minus_{a.a}_us": round(1000.0 * (med[a.b] - med[a.a]), 2), **extra}), flush=True)


if __name__ == "__main__":
    main()
