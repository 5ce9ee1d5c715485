"""Two training steps of the products recipe (bf16, hidden 256, 3 GCN layers with use_init, dropout 0) with the plain SpMM
launches gathering 12-bit coded operand rows (SGF_SPMM_CODED=1, the default) and with the switch off: loss, logits and every
gradient of both steps are equal bit for bit, and the coded launch ran exactly once per step for every launch class
sgformer_amd.graph.CODED_CLASSES names — under the merged policy, and with all five classes (the forward SpMMs of layers 2
and 3, the backward ones of layers 3, 2 and 1) named.  Layer 1's forward keeps its packed copy.  The node threshold
CODED_MIN_NODES is lowered for the test's 20 011 nodes."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 20011
ALL_CLASSES = frozenset({"fwd2", "fwd3", "bwd3", "bwd2", "bwd1"})


def _switch(v):
    from sgformer_amd import _lib
    if v is None:
        os.environ.pop("SGF_SPMM_CODED", None)
    else:
        os.environ["SGF_SPMM_CODED"] = str(v)
    _lib.load().sgf_reload_env()


@pytest.fixture(scope="module")
def task(cuda):
    from sgformer_amd import synth
    _, avg_deg, f, c, d = synth.SHAPES["ogbn-products"]
    ei = synth.synthetic_graph(N, avg_deg, seed=3, device=cuda)
    x, y, train_idx = synth.synthetic_task(N, f, c, seed=3)
    return ei, x.to(cuda), y.to(cuda), train_idx.to(cuda), (f, d, c)


def _two_steps(task, cuda):
    """(per step: loss, logits, gradients by name), (launch class, escaped rows, rows) of every operand that was coded"""
    import torch.nn.functional as F
    from sgformer_amd import coded, ops, synth
    from sgformer_amd.ours import SGFormer
    ei, x, y, train_idx, (f, d, c) = task
    ops.graph_cache.clear()
    torch.manual_seed(5)
    model = SGFormer(f, d, c, trans_dropout=0.0, gnn_dropout=0.0, compute_dtype=torch.bfloat16,
                     **synth.RECIPES["ogbn-products"]).to(cuda)
    model.logits_dtype = torch.float32
    model.train()
    opt = torch.optim.Adam([{"params": model.params1, "weight_decay": 1e-5}, {"params": model.params2, "weight_decay": 1e-5}],
                           lr=0.01)
    coded.escape_log = []
    try:
        out = []
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            logits = model(x, ei)
            loss = F.nll_loss(F.log_softmax(logits.float(), dim=1)[train_idx], y[train_idx])
            loss.backward()
            out.append((loss.detach().clone(), logits.detach().clone(),
                        {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}))
            opt.step()
        torch.cuda.synchronize()
        log = [(cls, int(esc.item()), rows) for cls, esc, rows in coded.escape_log]
    finally:
        coded.escape_log = None
    return out, log


def _policy(graph, classes, min_nodes=1000):
    prev = graph.CODED_CLASSES, graph.CODED_MIN_NODES
    graph.CODED_CLASSES, graph.CODED_MIN_NODES = frozenset(classes), min_nodes
    return prev


@pytest.fixture(scope="module")
def dense_steps(task, cuda):
    """The switch off, with every class named: no coded launch."""
    from sgformer_amd import graph, kernels
    prev = _policy(graph, ALL_CLASSES)
    _switch(0)
    try:
        before = kernels.counters["spmm_coded"]
        out, log = _two_steps(task, cuda)
        assert kernels.counters["spmm_coded"] == before and log == []
    finally:
        _switch(None)
        graph.CODED_CLASSES, graph.CODED_MIN_NODES = prev
    return out


def _same(a, b):
    for (la, ga, da), (lb, gb, db) in zip(a, b):
        assert torch.equal(la, lb) and torch.equal(ga, gb)
        assert da.keys() == db.keys() and len(da) > 10
        for k in da:
            assert torch.equal(da[k], db[k]), k


def test_merged_policy_is_equal(task, cuda, dense_steps, monkeypatch):
    from sgformer_amd import graph, kernels
    assert graph.CODED_CLASSES <= ALL_CLASSES
    monkeypatch.setattr(graph, "CODED_MIN_NODES", 1000)
    _switch(1)
    try:
        before = kernels.counters["spmm_coded"]
        out, log = _two_steps(task, cuda)
    finally:
        _switch(None)
    assert kernels.counters["spmm_coded"] - before == 2 * len(graph.CODED_CLASSES)
    assert sorted(cls for cls, _, _ in log) == sorted(2 * list(graph.CODED_CLASSES))
    _same(out, dense_steps)


def test_all_five_classes_are_equal(task, cuda, dense_steps, monkeypatch):
    from sgformer_amd import graph, kernels
    monkeypatch.setattr(graph, "CODED_CLASSES", ALL_CLASSES)
    monkeypatch.setattr(graph, "CODED_MIN_NODES", 1000)
    before = kernels.counters["spmm_coded"]
    packed_before = kernels.counters["spmm_packed"]
    out, log = _two_steps(task, cuda)
    assert kernels.counters["spmm_coded"] - before == 10
    assert kernels.counters["spmm_packed"] - packed_before == 2          # layer 1's forward keeps its packed copy
    assert [cls for cls, _, _ in log] == 2 * ["fwd2", "fwd3", "bwd3", "bwd2", "bwd1"]
    assert all(rows == N and 0 <= esc <= N for _, esc, rows in log), log
    _same(out, dense_steps)


def test_small_operands_stay_dense(task, cuda, monkeypatch):
    from sgformer_amd import graph, kernels
    monkeypatch.setattr(graph, "CODED_CLASSES", ALL_CLASSES)                 # CODED_MIN_NODES as merged: 65 536 > N
    before = kernels.counters["spmm_coded"]
    _two_steps(task, cuda)
    assert kernels.counters["spmm_coded"] == before
