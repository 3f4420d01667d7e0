"""Programs of ``Entry`` objects (what updater.PolicyUpdater lays a step out as): recording a list of entries into hipGraphs (``capture``,
``record``) and issuing a program, eager or recorded, on its two lanes (``execute``).  Nothing here knows about losses, Adam or rollouts."""
import contextlib
from typing import NamedTuple, Optional

import torch


class Entry(NamedTuple):
    """One entry of a step's program.  "run" entries that follow each other on one lane are recorded into ONE hipGraph (a "graph" entry of the
    recorded program); "sum" is an all-reduce of the tensor the getter returns, on the lane's communicator; "fork": the critic's lane waits
    for the caller's stream, "join": the reverse; "run_host" is host-only bookkeeping (at every eager step; once, when a step is recorded)."""
    kind: str                    # "run" | "graph" | "sum" | "fork" | "join" | "run_host"
    item: object                 # closure | CUDAGraph | tensor getter | None
    lane: str = "m"              # "m": the caller's stream, "s": the critic's
    label: Optional[str] = None
    eager: bool = False          # "run" only: issued as plain launches at every step, never recorded


@contextlib.contextmanager
def _no_gc_while_capturing():
    """Python's cyclic collector must not run while a stream is capturing: if it frees an object that owns device resources -- the hipGraphs
    or events of an updater that went out of use -- their destruction inside the capture is an error raised from a destructor, and the
    process aborts (seen once in six runs of tests/test_gpu_rollout.py: "Fatal Python error: Aborted ... Garbage-collecting" while the
    multi-step launch was recorded; this torch's ``torch.cuda.graph`` no longer collects on entry).  Garbage is collected BEFORE the capture,
    and the collector is held for its duration."""
    import gc
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()


def capture(fns, pool=None, generator=None, stream=None):
    """Record the launches of the closures ``fns`` into one hipGraph (torch.cuda.CUDAGraph) and return it: captured on a side stream
    (``stream``: a recorder of several graphs passes ONE, so that the graphs of a pool reuse each other's freed blocks) that waits for the
    current stream and is waited for, with the collector held.  ``pool``: the allocator pool to share with an earlier graph;
    ``generator``: a torch.Generator whose draws inside the graph advance with every replay."""
    g = torch.cuda.CUDAGraph()
    if generator is not None and hasattr(g, "register_generator_state"):
        g.register_generator_state(generator)
    side = stream if stream is not None else torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    # thread_local: background threads of the process (the collectives' watchdog) may keep issuing event queries
    with _no_gc_while_capturing(), torch.cuda.graph(g, pool=pool, stream=side, capture_error_mode="thread_local"):
        for fn in fns:
            fn()
    torch.cuda.current_stream().wait_stream(side)
    return g


def record(entries, capture=capture):
    """Entries -> the recorded program: "run" entries that follow each other on one lane are recorded into one hipGraph, anything else closes
    the open group; eager runs and collectives are kept, "run_host" entries run once, here.  ``capture``: for a test's stand-in only."""
    program, pools, cur = [], {}, []
    side = torch.cuda.Stream() if torch.cuda.is_available() else None   # ONE capture stream for the whole recording (see ``capture``)

    def close():
        if cur:
            lane = cur[0].lane
            # one allocator pool per lane: graphs of different lanes are replayed concurrently and must not share scratch memory
            g = capture([e.item for e in cur], pool=pools.get(lane), stream=side)
            pools[lane] = g.pool()
            program.append(Entry("graph", g, lane))
            cur.clear()

    for e in entries:
        if e.kind == "run" and not e.eager:
            if cur and cur[0].lane != e.lane:
                close()
            cur.append(e)
            continue
        close()
        if e.kind == "run_host":   # host-only bookkeeping (output dict of views): once, when the step is recorded
            e.item()
        else:
            program.append(e)
    close()
    return program


def execute(program, do, side_stream, span):
    """Run a program: lane "m" is the caller's stream, lane "s" the one ``side_stream()`` returns (asked for when first needed); "fork": the
    side lane waits for the main lane, "join": the reverse, inside ``span(label)`` (the wait is logged); ``do(entry)`` issues the rest."""
    main, side = torch.cuda.current_stream(), None
    for e in program:
        if side is None and (e.lane == "s" or e.kind in ("fork", "join")):
            side = side_stream()
        if e.kind == "fork":
            side.wait_stream(main)
        elif e.kind == "join":
            with span(e.label):
                main.wait_stream(side)
        elif e.lane == "s":
            with torch.cuda.stream(side):
                do(e)
        else:
            do(e)
