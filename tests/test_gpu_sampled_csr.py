"""sgf_sampled_csr_build / sgf_sampled_csr_transpose (csrc/sampled_csr.hip) on the GPU: the CSR a neighbour-sampled batch
carries, and the transpose ops.CSRGraph builds from it at the first backward, equal — bit for bit — what the general
edge-list entries sgf_csr_build / sgf_csr_transpose (called directly here) return for the same batch; the sampled training
step of the 100M recipe (100M/nb-sample.py:27-35) runs without either of the old entries and with one host read per batch,
and computes the same loss and gradients as with SGF_SAMPLED_CSR=0, element for element."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FANOUTS = [[15, 10, 5], [3, 2], [32], [40, 3], [0, 5], [5, 0, 3], [64], [100], [300]]


def _graph():
    from sgformer_amd import synth
    n = 4000
    return synth.synthetic_graph_skewed(n, 14.0, gamma=2.5), n


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, i, a.dtype, b.dtype, a.shape, b.shape)
        if a.dtype == torch.float32:
            a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
        assert torch.equal(a, b), (what, i)


def _check_batch(e, nn, carried: bool):
    """The batch's CSR and transpose (through ops.CSRGraph) against the old entries, called directly."""
    from sgformer_amd import ops
    from sgformer_amd.kernels import HipKernels
    want = HipKernels.csr_build(e, nn)
    assert want[0].dtype == torch.int64 and want[1].dtype == torch.int32 and want[3].dtype == torch.int32
    if carried:
        assert ops.hints_of(e).csr_t_lazy is True
        _same(ops.hints_of(e).csr, want, "carried CSR")
    else:
        assert ops.hints_of(e).csr is None and not ops.hints_of(e).csr_t_lazy
    g = ops.CSRGraph(e, nn)
    if carried:
        assert g.rowptr.data_ptr() == ops.hints_of(e).csr[0].data_ptr()   # adopted, not rebuilt
    _same((g.rowptr, g.colind, g.val, g.deg), want, "CSRGraph")
    t_want = HipKernels.csr_transpose(e, nn, want[3], want[0], want[1])
    t = g.transposed()
    if carried:
        assert g.symmetric is False
    _same(t, t_want[:3], "transpose")          # (a symmetric graph on the old path hands back the forward arrays: equal too)
    assert g.transposed()[0].data_ptr() == t[0].data_ptr()                 # built once
    return g, want, t_want


@pytest.mark.parametrize("fanouts", FANOUTS, ids=lambda f: "-".join(str(k) for k in f))
def test_sampled_batch_carries_the_csr_of_csr_build_bit_for_bit(cuda, fanouts, monkeypatch):
    from sgformer_amd import ops
    from sgformer_amd.sampling import NeighborSampler
    monkeypatch.setenv("SGF_SAMPLED_CSR", "1")
    ei, n = _graph()
    s = NeighborSampler(ei.to(cuda), n, fanouts, seed=1234)
    supported = ops.K.sampled_csr_supported(max(fanouts))
    assert supported or max(fanouts) > 64                                  # [0, 64] at least
    g = torch.Generator().manual_seed(5)
    reads = s.host_reads
    entries = 0
    for b in range(3):
        seeds = torch.randperm(n, generator=g)[:200]
        n_id, e, bs = s.sample(seeds.to(cuda))
        # a fan-out the kernels do not take: the fallback — no CSR attached, ops.CSRGraph builds it with K.csr_build
        _check_batch(e, int(n_id.numel()), carried=supported)
        entries += int(e.shape[1])
    assert s.host_reads - reads == 3
    assert entries > 0 or fanouts[0] == 0


def test_duplicate_stored_edges_stay_in_their_row(cuda, monkeypatch):
    """A parent graph with duplicate stored edges: the sampler draws stored ENTRIES without replacement, so a row of the batch
    can hold the same source twice — both stay, in edge order (large/ours.py:33 does not coalesce)."""
    from sgformer_amd.sampling import NeighborSampler
    monkeypatch.setenv("SGF_SAMPLED_CSR", "1")
    ei, n = _graph()
    ei2 = torch.cat([ei, ei[:, : ei.shape[1] // 2]], dim=1)
    s = NeighborSampler(ei2.to(cuda), n, [15, 10, 5], seed=77)
    g = torch.Generator().manual_seed(6)
    twice = 0
    for b in range(3):
        seeds = torch.randperm(n, generator=g)[:200]
        n_id, e, bs = s.sample(seeds.to(cuda))
        gr, want, _ = _check_batch(e, int(n_id.numel()), carried=True)
        rowptr, colind = want[0].cpu().numpy(), want[1].cpu().numpy()
        row = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
        twice += int(((row[1:] == row[:-1]) & (colind[1:] == colind[:-1])).sum())
    assert twice > 0, "no row held the same source twice: the case was not exercised"


@pytest.mark.parametrize("weighted", [False, True], ids=["star", "star_with_in_edges"])
def test_hub_source_gives_a_long_transposed_row(cuda, monkeypatch, weighted):
    """A star: every seed's only in-neighbour is one hub, fan-out [1], 5000 seeds — the transposed CSR has ONE row of 5000
    entries (> 4096), ordered by target.  In the plain star the hub has no in-edge, so every value is 0 (the nan_to_num rule);
    `star_with_in_edges` makes the long row carry values that differ from entry to entry: the hub is a seed too with two
    stored in-neighbours, every odd seed has a second in-neighbour (the seed before it), fan-out [2] — in-degrees 1 and 2
    alternate along the hub's transposed row, so its values alternate between 1/sqrt(2) and 1/2 and their order is tested."""
    from sgformer_amd import ops
    from sgformer_amd.sampling import NeighborSampler
    monkeypatch.setenv("SGF_SAMPLED_CSR", "1")
    m = 5000
    src, dst = [torch.full((m,), m, dtype=torch.int64)], [torch.arange(m, dtype=torch.int64)]
    if weighted:
        odd = torch.arange(1, m, 2, dtype=torch.int64)
        src += [odd - 1, torch.tensor([0, 1])]
        dst += [odd, torch.tensor([m, m])]
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    s = NeighborSampler(ei.to(cuda), m + 1, [2] if weighted else [1], seed=5)
    n_id, e, bs = s.sample(torch.arange(m + 1 if weighted else m, device=cuda))
    assert int(n_id.numel()) == m + 1 and int(e.shape[1]) == int(ei.shape[1])
    assert torch.equal(n_id.cpu(), torch.arange(m + 1))                    # local ids = global ids here
    gr, _, _ = _check_batch(e, m + 1, carried=True)
    t_rowptr, t_colind, t_val = gr.transposed()
    assert int(t_rowptr[m + 1] - t_rowptr[m]) == m > 4096
    hub_row = slice(int(t_rowptr[m]), int(t_rowptr[m + 1]))
    assert torch.equal(t_colind[hub_row].long().cpu(), torch.arange(m))
    if weighted:
        r = np.sqrt(np.float32(1.0) / np.float32(2.0))          # sqrtf(1.0f / deg), as norm_value forms it
        want = np.where(np.arange(m) % 2 == 1, np.float32(r * r), np.float32(np.float32(1.0) * r)).astype(np.float32)
        assert np.array_equal(t_val[hub_row].cpu().numpy().view(np.uint32), want.view(np.uint32))
    else:
        assert not bool(t_val.any())
    # dX = A^T dY on that row against the same product on the old path's arrays
    x = torch.randn(m + 1, 64, device=cuda)
    fresh = ops.CSRGraph(e.clone(), m + 1)
    assert not fresh._t_lazy
    got, ref = ops.spmm_on(gr, x, True), ops.spmm_on(fresh, x, True)
    assert torch.equal(got, ref) and bool(got[m].any()) == weighted


def _task(cuda, seed=3, feature_dtype=None, fanouts=(15, 10, 5)):
    from sgformer_amd import synth
    from sgformer_amd.sampling import NeighborLoader
    n, f, c = 5000, 24, 9
    ei = synth.synthetic_graph_skewed(n, 12.0, gamma=2.5, seed=4)
    g = torch.Generator().manual_seed(11)

    class Data:
        pass
    data = Data()
    data.x, data.y, data.edge_index = torch.randn(n, f, generator=g), torch.randint(0, c, (n,), generator=g), ei
    loader = NeighborLoader(data, input_nodes=torch.arange(0, 600), num_neighbors=list(fanouts), batch_size=256,
                            shuffle=False, seed=seed, feature_dtype=feature_dtype)
    return loader, f, c


def _model(cuda, f, c, compute_dtype=None):
    from oracle import sgformer_oracle as O
    from sgformer_amd.ours_100m import SGFormer
    d = 64
    cfg = dict(alpha=0.5, trans_num_layers=1, gnn_num_layers=3, gnn_use_init=True, graph_weight=0.8)
    p = O.init_params(cfg, f, d, c, seed=1)
    m = SGFormer(f, d, c, trans_dropout=0.0, gnn_dropout=0.0, compute_dtype=compute_dtype, **cfg)
    m.load_state_dict({**m.state_dict(), **p})
    return m.to(cuda).train()


def _step(m, graph):
    """The trainer's lines (100M/nb-sample.py:27-35)."""
    bs = graph.batch_size
    out = m(graph.x, graph.edge_index)[:bs]
    loss = torch.nn.CrossEntropyLoss()(out.float(), graph.y[:bs])
    m.zero_grad(set_to_none=True)
    loss.backward()
    return loss.detach()


def test_training_step_needs_neither_old_entry_and_reads_the_host_once(cuda, monkeypatch):
    from sgformer_amd import ops
    monkeypatch.setenv("SGF_SAMPLED_CSR", "1")
    ops.graph_cache.clear()
    loader, f, c = _task(cuda)             # (the PARENT graph's CSR is built here, with sgf_csr_build)
    m = _model(cuda, f, c)

    def old_path(*a, **k):
        raise AssertionError("the general edge-list path was called for a sampled batch")
    monkeypatch.setattr(ops.K, "csr_build", old_path)
    monkeypatch.setattr(ops.K, "csr_transpose", old_path)
    calls = {"t": 0}
    real_t = ops.K.sampled_csr_transpose

    def counted(*a, **k):
        calls["t"] += 1
        return real_t(*a, **k)
    monkeypatch.setattr(ops.K, "sampled_csr_transpose", counted)
    reads, batches = loader.sampler.host_reads, 0
    for graph in loader:
        graph = graph.to(cuda)
        assert ops.hints_of(graph.edge_index).csr is not None and ops.hints_of(graph.edge_index).csr_t_lazy
        before = loader.sampler.host_reads
        loss = _step(m, graph)
        assert loader.sampler.host_reads == before
        assert bool(torch.isfinite(loss)) and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
        batches += 1
        assert calls["t"] == batches                                       # once per batch, at its first backward
    assert batches == len(loader) == 3 and loader.sampler.host_reads - reads == batches
    # without autograd nothing asks for the transpose
    with torch.no_grad():
        for graph in loader:
            m(graph.x, graph.edge_index)
    assert calls["t"] == batches
    # the attributes travel with the batch (SampledBatch.to), the CSR to the same device as its edge list
    moved = graph.to("cpu")
    assert ops.hints_of(moved.edge_index).csr_t_lazy and ops.hints_of(moved.edge_index).trusted
    assert all(t.device.type == "cpu" for t in ops.hints_of(moved.edge_index).csr)
    assert all(torch.equal(a, b.cpu()) for a, b in zip(ops.hints_of(moved.edge_index).csr, ops.hints_of(graph.edge_index).csr))


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_same_arithmetic_with_the_switch_on_and_off(cuda, monkeypatch, dtype):
    """Same initial state, same batch: SGF_SAMPLED_CSR=1 and =0 hand the SpMM identical CSR arrays and every kernel on the path
    is deterministic, so the loss and every parameter gradient are torch.equal."""
    from sgformer_amd import ops
    dt = torch.bfloat16 if dtype == "bf16" else None
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("SGF_SAMPLED_CSR", flag)
        ops.graph_cache.clear()
        loader, f, c = _task(cuda, feature_dtype=dt)
        m = _model(cuda, f, c, compute_dtype=dt)
        graph = next(iter(loader))
        assert (ops.hints_of(graph.edge_index).csr is not None) == (flag == "1")
        loss = _step(m, graph)
        res[flag] = (graph.n_id.clone(), graph.edge_index.clone(), loss.clone(),
                     {k: p.grad.detach().clone() for k, p in m.named_parameters()})
    on, off = res["1"], res["0"]
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])       # the same batch
    assert torch.equal(on[2], off[2]), (float(on[2]), float(off[2]))
    assert set(on[3]) == set(off[3]) and len(on[3]) > 0
    for k in on[3]:
        assert torch.equal(on[3][k], off[3][k]), k


def test_switch_off_and_hop_by_hop_batches_carry_no_csr(cuda, monkeypatch):
    from sgformer_amd.sampling import NeighborSampler
    ei, n = _graph()
    seeds = torch.arange(100, 300, device=cuda)
    monkeypatch.setenv("SGF_SAMPLED_CSR", "0")
    s = NeighborSampler(ei.to(cuda), n, [15, 10, 5], seed=9)
    n_id, e, bs = s.sample(seeds)
    _check_batch(e, int(n_id.numel()), carried=False)
    monkeypatch.setenv("SGF_SAMPLED_CSR", "1")
    n_id1, e1, _ = s.sample(seeds, batch_id=0)
    assert torch.equal(e1, e) and torch.equal(n_id1, n_id)                 # the switch does not touch the draw
    _check_batch(e1, int(n_id1.numel()), carried=True)
    # a fan-out of -1 (all neighbours) has no a-priori capacity: the hop-by-hop path, unchanged
    h = NeighborSampler(ei.to(cuda), n, [-1, 4], seed=9)
    n_id2, e2, bs2 = h.sample(seeds)
    assert bs2 == 200 and int(e2.shape[1]) > 0 and h.host_reads > 1
    _check_batch(e2, int(n_id2.numel()), carried=False)
