"""graph.RigidTasksData / ClothTasksData / RopeTasksData, the kNN kernel and the DeepSets critic against what the REFERENCE's data
classes and its GNNVFNet -> DeepSets.one_step produced (tests/golden/tier3_*.npz, tools/make_golden.py tier3) -- no oracle in between.

The classes are built with the recorded ``observation_dim`` / ``observation_names`` and the keyword arguments the reference classes got.
Node features, raw positions and one-hot columns must be EXACTLY equal to the reference rows of the valid points (gathers, zeros and one
float32 subtraction of two observation values; the actor graph drops the zero-padded points the reference keeps as edgeless nodes,
``GraphBatch.natural`` maps our numbering to the reference's order); edge sets must be equal.  The critic is compared at the DeepSets bars
of tests/test_gpu_actor_ops.py (ops_ref.BARS["deepsets"]: value 1e-5, gradients 4e-5 of the tensor's scale) against the float64 run of
the reference code.  tests/data_fixtures.py lists what no fixture covers."""
import pytest
import torch

import data_fixtures as dfx
import ops_ref
from ops_ref import margin

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def data_class(fx, layout):
    from geometry_rl_amd import graph
    cls = {"rigid": graph.RigidTasksData, "cloth": graph.ClothTasksData, "rope": graph.RopeTasksData}[fx.family]
    return cls(observation_dim=fx.observation_dim, observation_names=fx.observation_names, training_noise=False, **fx.kwargs, **layout)


def build(hd, args, merged):
    """build_data as its own launch, or with the feature role riding in the merged head launch (ops.HeadLaunch: grl_step_head)."""
    from geometry_rl_amd import ops
    if not merged:
        return hd.build_data(*args, train=True)
    assert ops.HEAD is None
    ops.HEAD = ops.HeadLaunch()
    try:
        out = hd.build_data(*args, train=True)
        assert ops.HEAD.feat is not None, "the feature role was not handed to the head launch"
        ops.HEAD.launch()
    finally:
        ops.HEAD = None
    return out


ACTOR_IDS = [(c, t) for c in dfx.CASES for t in dfx.layouts(c) if t != "critic"]


@pytest.mark.parametrize("merged", [False, True], ids=["eager", "head_launch"])
@pytest.mark.parametrize("balance", [True, False], ids=["balanced", "natural"])
@pytest.mark.parametrize("case,tag", ACTOR_IDS)
def test_actor_layout_equals_the_reference(golden_dir, case, tag, balance, merged):
    from geometry_rl_amd import graph as G
    d = dev()
    fx = dfx.Fixture(golden_dir, case)
    old = G.BALANCE_NODE_ORDER
    G.BALANCE_NODE_ORDER = balance
    try:
        hd = data_class(fx, dfx.layouts(case)[tag])
        graph, (s, v) = build(hd, [a.to(d) for a in fx.args()], merged)
        torch.cuda.synchronize()
    finally:
        G.BALANCE_NODE_ORDER = old
    assert graph.node_types == fx.node_types(tag)
    nat = {}
    for t in graph.node_types:
        rows = fx.valid_rows(t)
        assert graph.num_nodes[t] == rows.numel(), t
        nat[t] = graph.natural(t, torch.arange(rows.numel(), device=d)).cpu()
        assert sorted(nat[t].tolist()) == list(range(rows.numel())), t
        ref = lambda what: fx.node(tag, what, t)[rows][nat[t]]
        assert torch.equal(graph.pos[t].cpu(), ref("pos")), t
        assert torch.equal(s[t].cpu(), ref("scalar")), t
        assert torch.equal(v[t].cpu().reshape(rows.numel(), -1), ref("vector")), t
    n_ref = 0
    for et in fx.edge_types(tag):
        want = fx.compact_edge_set(tag, et)
        n_ref += bool(want)
        if not want:
            assert et not in graph.edges, et
            continue
        es = graph.edges[et]
        assert (es.n_src, es.n_dst, es.n_edges) == (graph.num_nodes[et[0]], graph.num_nodes[et[2]], len(want)), et
        for src, dst in ((es.src_d, es.dst_d), (es.src_s, es.dst_s)):   # both CSR orders hold the reference's edges, direction included
            got = sorted(zip(nat[et[0]][src.long().cpu()].tolist(), nat[et[2]][dst.long().cpu()].tolist()))
            assert got == want, et
    assert len(graph.edges) == n_ref                                    # the number of non-empty edge types


@pytest.mark.parametrize("merged", [False, True], ids=["eager", "head_launch"])
@pytest.mark.parametrize("case", list(dfx.CASES))
def test_critic_layout_equals_the_reference(golden_dir, case, merged):
    d = dev()
    fx = dfx.Fixture(golden_dir, case)
    hd = data_class(fx, dfx.CRITIC)
    graph, x = build(hd, [a.to(d) for a in fx.args()], merged)
    assert graph.node_types == fx.node_types("critic")
    assert torch.equal(x.cpu(), fx.critic_dense())


@pytest.mark.parametrize("case", [c for c, f in dfx.CASES.items() if f != "cloth"])
def test_knn_kernel_returns_the_reference_neighbour_sets(golden_dir, case):
    """grl_knn_topology on the fixture's positions and valid counts: per valid point the set it returns is the set of SOURCES the
    reference's ``knn_graph`` call site gives that point as destination (edges [neighbour, centre]); -1 beyond min(k, n - 1)."""
    from geometry_rl_amd import hip
    d = dev()
    fx = dfx.Fixture(golden_dir, case)
    P, k, nv = fx.n_per(fx.main), fx.kwargs["knn_k"], fx.n_valid()
    names, dims = fx.observation_names["position_vectors"], [x[0] for x in fx.observation_dim["position_vectors"]]
    o = sum(dims[:names.index(fx.main)])
    pos = fx.obs["position_vectors"][:, o:o + 3 * P].reshape(fx.B, P, 3).contiguous()
    out = torch.full((fx.B, P, k), -7, device=d, dtype=torch.int32)
    hip.call("grl_knn_topology", pos.to(d), nv.int().to(d), out, fx.B, P, k)
    out = out.cpu()
    want = {}
    for s_, c_ in fx.edge_set("actor", (fx.main, "internal", fx.main)):
        assert s_ // P == c_ // P
        want.setdefault(c_, set()).add(s_ % P)
    for b in range(fx.B):
        for j in range(int(nv[b])):
            got = [int(i) for i in out[b, j] if i >= 0]
            assert len(got) == min(k, int(nv[b]) - 1) and set(got) == want.get(b * P + j, set()), (b, j, got)


@pytest.mark.parametrize("case", dfx.CRITIC_CASES)
def test_critic_equals_the_reference(golden_dir, case):
    """The reference state dict loaded by name; value and every gradient for the 2-D batch and the 3-D [N, T, .] input (the loop over
    time under autograd, ``deepsets_values_groups`` without)."""
    from geometry_rl_amd import policy
    d = dev()
    fx = dfx.Fixture(golden_dir, case)
    z = dfx.load_critic(golden_dir)
    bar_v, bar_g = ops_ref.BARS["deepsets"]
    hd = data_class(fx, dfx.CRITIC)
    d_in = fx.critic_dense().shape[-1]
    net = policy.GNNVFNet(gnn=policy.DeepSets(input_dim_node=d_in, device=d), hyper_data=hd)
    params = {k[len(case) + 7:]: v for k, v in z.items() if k.startswith(case + ".param.")}
    net.load_state_dict(params, strict=True)
    obs3 = [z[f"{case}.obs3.{k}"].to(d) for k in dfx.IN_FEATURES if f"{case}.obs3.{k}" in z]
    for rank, args in (("2d", [a[:, 0].contiguous() for a in obs3]), ("3d", obs3)):
        print(f"{case} {rank}")
        net.zero_grad()
        val = net(*args, train=True)
        margin("state_value", val, z[f"{case}.{rank}.state_value"], bar_v)
        (val * z[f"{case}.{rank}.cotangent"].float().to(d)).sum().backward()
        for k, p in net.named_parameters():
            margin("d " + k, p.grad, z[f"{case}.{rank}.grad.{k}"], bar_g)
    with torch.no_grad():
        val = net(*obs3, train=True)
    print(f"{case} 3d, grouped launches")
    margin("state_value", val, z[f"{case}.3d.state_value"], bar_v)
