#!/usr/bin/env python3
"""Critical path of the data-parallel policy update, measured where only ONE GPU is available.

W ranks (default 2) share cuda:0 and talk over gloo -- the functional stand-in for 8 ranks over RCCL the test-suite uses -- each
updating a 512-frame shard (the per-GPU share of BASELINE's 4096-frame minibatch on 8 GPUs) with the recorded two-lane program
(``PolicyUpdater(use_graph=True, group=...)``).  HIP events (``torch.cuda.Event``) are recorded on the issuing stream immediately
before and after every collective and around the graph segments between them, for ``--steps`` replayed steps.  Output (JSON):

  * per collective: payload bytes, lane (main / critic side lane), whether the main lane waits for it, mean event time and host
    wall time around the call (gloo stages through the host: this is an UPPER bound for a small RCCL all-reduce over xGMI);
  * per graph segment: device time;
  * the step's critical path = main-lane segments + the collectives the main lane waits for, and the prediction this gives for
    8 x MI355X once the gloo numbers are replaced by RCCL's small-message latency (a parameter, ``--rccl-us``).

Ranks sharing one GPU time-slice its CUs, so segment times are taken from rank 0 of a W = 1 run of the same shard (no contention)
unless ``--segments-from-shared`` is given.

  python tools/dp_collective_timing.py --world 2 --steps 20 --out profiles/r02_dp_critical_path.json
"""
import argparse
import json
import os
import socket
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _worker(rank, world, port, args, ret):
    import torch.distributed as dist
    from geometry_rl_amd import agent, graph, synthetic as syn
    group = None
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        group = dist.group.WORLD
    dev = torch.device("cuda:0")
    spec = graph.rigid_spec()
    cfg = agent.AgentConfig(only_upper_hemisphere=True, output_dim=2, output_dim_vec=2)
    torch.manual_seed(0)
    actor, critic, proj, loss = agent.build_agent(spec, cfg, device=dev, group=group)
    B = args.shard
    batch = dict(syn.make_rigid_obs(B, seed=3, env_offset=rank * B))
    batch.update(syn.make_ppo_fields(B, 6, seed=3 + rank))
    batch = {k: v.to(dev) for k, v in batch.items()}
    upd = agent.PolicyUpdater(loss, lr=cfg.lr, group=group, use_graph=True)
    for _ in range(3):
        upd.step(batch)           # eager (+ calibration), record, first replay
    records = []                  # (kind, label, lane, e0, e1, host_s)

    orig_do = upd._do

    def timed_do(entry):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        payload = None
        if entry.kind == "sum":   # evaluate the tensor getter here, for the payload size
            t = entry.item()
            payload = None if t is None else t.numel() * t.element_size()
            entry = entry._replace(item=lambda: t)
        orig_do(entry)
        host = time.perf_counter() - t0
        e1.record()
        records.append((entry.kind, payload, entry.lane, e0, e1, host))

    upd._do = timed_do
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        upd.step(batch)
    torch.cuda.synchronize()
    step_ms = 1e3 * (time.perf_counter() - t0) / args.steps
    per_step = len(records) // args.steps
    rows = []
    for i in range(per_step):
        kind, payload, lane, _, _, _ = records[i]
        ev = [records[s * per_step + i][3].elapsed_time(records[s * per_step + i][4]) for s in range(args.steps)]
        host = [records[s * per_step + i][5] * 1e3 for s in range(args.steps)]
        rows.append({"index": i, "kind": kind, "lane": "critic side lane" if lane == "s" else "main", "payload_bytes": payload,
                     "event_ms_mean": sum(ev) / len(ev), "event_ms_min": min(ev), "host_ms_mean": sum(host) / len(host)})
    ret[rank] = {"step_ms_wall": step_ms, "program": rows}
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shard", type=int, default=512)
    ap.add_argument("--out", default=None, help="write the JSON here (stdout otherwise; c10d warnings may interleave with stdout)")
    ap.add_argument("--rccl-us", type=float, default=25.0, help="assumed latency of one small (<= 1 MB) RCCL all-reduce over xGMI, 8 ranks")
    args = ap.parse_args()
    import torch.multiprocessing as mp
    out = {}
    for world in (1, args.world):
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        ret = mp.Manager().dict()
        mp.spawn(_worker, args=(world, port, args, ret), nprocs=world, join=True)
        out[f"world_{world}"] = dict(ret[0])
    single = out["world_1"]
    multi = out[f"world_{args.world}"]
    colls = [r for r in multi["program"] if r["kind"] not in ("run", "graph")]
    main_wait = [r for r in colls if r["lane"] == "main" and r["kind"] in ("sum", "max")]
    seg_main = sum(r["event_ms_mean"] for r in multi["program"] if r["kind"] == "graph" and r["lane"] == "main")
    pred_ms = single["step_ms_wall"] + len(main_wait) * args.rccl_us * 1e-3
    summary = {
        "what": "rigid HEPi, 512-frame shard per rank (4096-frame minibatch / 8), recorded two-lane program; gloo ranks share ONE GPU",
        "single_rank_step_ms": single["step_ms_wall"],
        f"{args.world}_ranks_on_one_gpu_step_ms": multi["step_ms_wall"],
        "collectives_per_step": len(colls),
        "collectives_the_main_lane_waits_for": [{"kind": r["kind"], "payload_bytes": r["payload_bytes"], "gloo_event_ms": r["event_ms_mean"]} for r in main_wait],
        "side_lane_collectives": [{"kind": r["kind"], "payload_bytes": r["payload_bytes"], "gloo_event_ms": r["event_ms_mean"]} for r in colls if r not in main_wait],
        "main_lane_graph_ms_shared_gpu": seg_main,
        "prediction_8_gpus": {"assumed_rccl_small_allreduce_us": args.rccl_us,
                              "ms_per_step": pred_ms, "steps_per_s": 1e3 / pred_ms,
                              "formula": "single-rank 512-frame step (device-bound, replayed) + (collectives the main lane waits for) x RCCL latency; "
                                         "the side lane's four statistic all-reduces hide behind the actor forward / backward if each stays below ~0.1 ms"},
    }
    text = json.dumps({"summary": summary, "detail": out}, indent=1)
    if args.out:
        open(args.out, "w").write(text)
        print(json.dumps(summary["prediction_8_gpus"]))
    else:
        print(text)


if __name__ == "__main__":
    main()
