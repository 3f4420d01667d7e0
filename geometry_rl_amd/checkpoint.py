"""Saving and resuming a training run bit for bit.  The reference's ``train.py`` saves model weights alone (``agent.reference_checkpoint``);
most of what makes update ``n + 1`` what it is lives outside ``state_dict()``: the flat buffers and both moments, the step counts on the
host and in device memory, the learning rate, the loss module's device scalars, the projection's latched initial entropy, the running
sums, the calibration latches, the training-noise words, the cached kNN topologies, the samplers' generators, the normaliser's and the
episode statistics' state.  Every object that carries some of it has ``state_dict()`` / ``load_state_dict()``; this module puts their
states into ONE file and back:

    checkpoint.save(path, updater=upd, driver=drv, actor=collector, normalizer=norm, episodes=stats)
    ...                                                       # another process: everything built again, with the same settings
    checkpoint.restore(checkpoint.load(path), updater=upd, driver=drv, actor=collector, normalizer=norm, episodes=stats)

A file holds CPU tensors and plain Python values only (``torch.load(..., weights_only=True)`` reads it: nothing in it needs unpickling
code) and is also a model checkpoint: ``agent.load_reference_checkpoint(checkpoint.load(path)["model"], actor, critic)``.  Data parallel:
every rank saves and loads a file of its own (the caller names it per rank); the ranks' files differ in the noise keys and in nothing else.

``python -m geometry_rl_amd.checkpoint FILE`` lists a file's parts, step count, algorithm, tensor shapes and bytes; it needs no GPU.

The helpers below are what the objects' ``state_dict`` methods share."""
import os
from typing import Dict, Optional

import torch

FORMAT = "geometry_rl_amd.training_state"
VERSION = 1


# ------------------------------------------------------------------------------------------------------------- shared by the objects
def check_version(sd: dict, what: str) -> None:
    if not isinstance(sd, dict) or sd.get("version") != VERSION:
        raise ValueError(f"{what}: the state has format version {sd.get('version') if isinstance(sd, dict) else None!r}, this package reads "
                         f"version {VERSION}")


def layout(named_groups, flat: torch.Tensor) -> list:
    """The fingerprint of a flat parameter buffer: [name, shape, offset in ``flat``] per trainable parameter, in the buffer's order.
    ``named_groups``: [(prefix, module)]."""
    out = []
    for prefix, mod in named_groups:
        for name, p in mod.named_parameters():
            if p.requires_grad:
                out.append([prefix + name, list(p.shape), (p.data_ptr() - flat.data_ptr()) // flat.element_size()])
    return out


def module_mismatch(mod, sd: Dict[str, torch.Tensor], what: str) -> Optional[str]:
    """What keeps ``mod.load_state_dict(sd)`` from succeeding (keys or shapes), found WITHOUT writing; None where nothing does."""
    have = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
    want = {k: tuple(v.shape) for k, v in sd.items()}
    if have != want:
        odd = sorted(set(have) ^ set(want)) or sorted(k for k in have if have[k] != want[k])
        return f"{what}: the saved module state does not fit ({len(odd)} entries differ, e.g. {odd[:3]})"
    return None


def data_state(hd) -> dict:
    """A ``HyperData``'s share of the training state: the {seed, draw} words of its training noise and its position-built topologies."""
    seed, draw = hd.noise_state()
    return {"noise": [int(seed), int(draw)], "topology": hd.topology_state()}


def load_data_state(hd, s: dict, device) -> None:
    hd.set_noise_state(*s["noise"])
    hd.load_topology_state(s["topology"], device)


def settle_calibration(actor) -> bool:
    """Behind ``actor.load_state_dict`` (which makes the policy inspect its convolutions' ``callibrated`` latches again at its next training
    forward): inspect them HERE, outside any capture -- reading them synchronises, and the next forward of a live updater may be recorded.
    -> are the convolutions calibrated?  False (a state saved before the first training forward): that forward calibrates, eagerly."""
    gnn = getattr(actor, "gnn", None)
    if getattr(actor, "post_fc", False) or gnn is None or not hasattr(gnn, "calibrated"):
        return True
    actor._calib_checked = bool(gnn.calibrated)
    return actor._calib_checked


def generator_state(gen, seed) -> dict:
    """A sampler's generator: its state once it exists, the seed it will be made from until then."""
    return {"seed": int(seed), "state": None if gen is None else gen.get_state().clone(), "device": None if gen is None else gen.device.type}


def restore_generator(s: dict, device):
    """-> (a NEW generator at the saved state, or None where none existed yet; the seed)."""
    if s["state"] is None:
        return None, s["seed"]
    device = torch.device(device)
    if device.type != s["device"]:
        raise ValueError(f"the saved generator is a '{s['device']}' generator, the sampler draws on '{device.type}'")
    gen = torch.Generator(device=device)
    gen.set_state(s["state"])
    return gen, s["seed"]


def differing(saved: dict, mine: dict) -> list:
    """The keys at which two plain dicts differ (a key one of them lacks differs)."""
    return sorted(k for k in set(saved) | set(mine) if k not in saved or k not in mine or saved[k] != mine[k])


# ------------------------------------------------------------------------------------------------------------- the file
def _networks(parts):
    """(actor, critic) of the first part that reaches a loss module; critic None for a module without one (behaviour cloning)."""
    for p in parts.values():
        m = getattr(p, "loss_module", None)
        if m is None and hasattr(p, "updater"):
            m = getattr(p.updater, "loss_module", None)
        if m is not None and hasattr(m, "actor_network"):
            return m.actor_network, getattr(m, "critic_network", None)
    return None, None


def save(path, *, reward=0.0, env_state=None, **parts) -> dict:
    """Write the ``state_dict()`` of every part (any names: ``updater=..., driver=...``) into one file -> what was written.  ``"model"`` is
    the reference's own checkpoint of the networks the parts reach (``agent.reference_checkpoint``; ``reward`` and ``env_state`` are its
    entries: the simulator's state stays the caller's).  Written to a temporary file next to ``path`` and renamed, so an interrupted save
    leaves the previous file whole."""
    from . import agent, hip
    if not parts:
        raise ValueError("checkpoint.save: no parts")
    state = {"format": FORMAT, "version": VERSION, "abi": hip.ABI_VERSION, "parts": {k: p.state_dict() for k, p in parts.items()}}
    actor, critic = _networks(parts)
    if actor is not None and critic is not None:
        state["model"] = agent.reference_checkpoint(actor, critic, reward=reward, env_state=env_state)
    elif actor is not None:
        state["model"] = {"env": env_state if env_state is not None else {}, "reward": reward,
                          "actor": {agent.ACTOR_PREFIX + k: v.detach().cpu().clone() for k, v in actor.state_dict().items()}}
    else:
        state["model"] = None
    path = os.fspath(path)
    tmp = f"{path}.tmp.{os.getpid()}"
    try:
        torch.save(state, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return state


def load(path) -> dict:
    """Read a training-state file: tensors and plain containers only (``weights_only=True``), everything on the CPU."""
    state = torch.load(path, weights_only=True, map_location="cpu")
    if not isinstance(state, dict) or state.get("format") != FORMAT:
        raise ValueError(f"{path!r} is not a training-state file of this package (format {state.get('format') if isinstance(state, dict) else None!r})")
    check_version(state, os.fspath(path))
    return state


def restore(state: dict, **parts) -> None:
    """``load_state_dict`` of every part from the file's part of the same name.  Refuses -- before any part is touched -- a part the file
    lacks and a part of the file nobody asked for: a run resumed with half its state is another run."""
    if state.get("format") != FORMAT:
        raise ValueError(f"not a training state (format {state.get('format')!r})")
    check_version(state, "checkpoint.restore")
    missing, spare = sorted(set(parts) - set(state["parts"])), sorted(set(state["parts"]) - set(parts))
    if missing:
        raise ValueError(f"the file holds no part {missing} (it holds {sorted(state['parts'])})")
    if spare:
        raise ValueError(f"the file's part(s) {spare} were not asked for: pass every object the run was saved with")
    for k, p in parts.items():
        p.load_state_dict(state["parts"][k])


# ------------------------------------------------------------------------------------------------------------- python -m ... FILE
def _walk(x, prefix=""):
    """(path, tensor) of every tensor below ``x``."""
    if torch.is_tensor(x):
        yield prefix, x
    elif isinstance(x, dict):
        for k, v in x.items():
            yield from _walk(v, f"{prefix}.{k}" if prefix else str(k))
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            yield from _walk(v, f"{prefix}[{i}]")


def contents(state: dict) -> list:
    """The lines ``python -m geometry_rl_amd.checkpoint FILE`` prints."""
    lines = [f"{state['format']} version {state['version']} (kernel ABI {state.get('abi')})"]
    total = 0
    for name, part in list(state["parts"].items()) + [("model", state.get("model") or {})]:
        tensors = list(_walk(part, name))
        nbytes = sum(t.numel() * t.element_size() for _, t in tensors)
        total += nbytes
        head = f"part {name}: {len(tensors)} tensors, {nbytes} bytes" if name != "model" or part else "model: none"
        if isinstance(part, dict):
            if "steps" in part:
                head += f", step count {part['steps']}"
            if isinstance(part.get("algorithm"), dict):
                head += ", algorithm " + " ".join(f"{k}={v}" for k, v in part["algorithm"].items())
            if "rank" in part:
                head += f", rank {part['rank']} of {part['world']}"
        lines.append(head)
        lines += [f"    {p}: {t.dtype} {list(t.shape)}".replace("torch.", "") for p, t in tensors]
    lines.append(f"total: {total} bytes in tensors")
    return lines


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m geometry_rl_amd.checkpoint", description="List what a training-state file holds (no GPU needed).")
    ap.add_argument("file")
    ap.add_argument("--no-tensors", action="store_true", help="one line per part, without the tensor list")
    args = ap.parse_args(argv)
    for line in contents(load(args.file)):
        if not (args.no_tensors and line.startswith("    ")):
            print(line)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
