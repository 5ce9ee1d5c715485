"""Two training steps of the products recipe (bf16, hidden 256, 3 GCN layers with use_init, dropout 0) with the forward GCN
SpMM gathering packed operand rows (SGF_SPMM_PACKED=1, the default) and with the switch off: loss, logits and every gradient
of both steps are equal bit for bit, and the packed launch ran for exactly the layers sgformer_amd.ours.PACKED_SLOT_BYTES
names.  With a slot given to all three layers the operands of layers 2 and 3 overflow their slots (relu(BatchNorm) + x0 is
about three quarters non-zero): those launches fall back to the dense rows on the device — still bit for bit."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 20011


def _switch(v):
    from sgformer_amd import _lib
    if v is None:
        os.environ.pop("SGF_SPMM_PACKED", None)
    else:
        os.environ["SGF_SPMM_PACKED"] = str(v)
    _lib.load().sgf_reload_env()


@pytest.fixture(scope="module")
def task(cuda):
    from sgformer_amd import synth
    _, avg_deg, f, c, d = synth.SHAPES["ogbn-products"]
    ei = synth.synthetic_graph(N, avg_deg, seed=3, device=cuda)
    x, y, train_idx = synth.synthetic_task(N, f, c, seed=3)
    return ei, x.to(cuda), y.to(cuda), train_idx.to(cuda), (f, d, c)


def _two_steps(task, cuda):
    """(per step: loss, logits, gradients by name), (overflow counts of the packed launches)"""
    import torch.nn.functional as F
    from sgformer_amd import ops, synth
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
    overflows, real = [], ops.K.spmm_packed

    def spy(rowptr, colind, val, xx, packed, n_rows, long_segments=0):
        # the launcher's own rule: this call launches k_spmm_row_packed (which gathers the slots while the count is zero)
        assert ops.K.spmm_packed_supported(xx.shape, xx.dtype, packed.slot_bytes)
        overflows.append(packed.overflow)
        return real(rowptr, colind, val, xx, packed, n_rows, long_segments=long_segments)

    ops.K.spmm_packed = spy                     # (an instance attribute over the class's static method)
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
    finally:
        del ops.K.spmm_packed
    torch.cuda.synchronize()
    return out, [int(o.item()) for o in overflows]


@pytest.fixture(scope="module")
def dense_steps(task, cuda):
    from sgformer_amd import kernels
    _switch(0)
    try:
        before = kernels.counters["spmm_packed"]
        out, overflows = _two_steps(task, cuda)
        assert kernels.counters["spmm_packed"] == before and overflows == []
    finally:
        _switch(None)
    return out


def _same(a, b):
    for (la, ga, da), (lb, gb, db) in zip(a, b):
        assert torch.equal(la, lb) and torch.equal(ga, gb)
        assert da.keys() == db.keys() and len(da) > 10
        for k in da:
            assert torch.equal(da[k], db[k]), k


def test_default_layers_are_packed_and_equal(task, cuda, dense_steps):
    from sgformer_amd import kernels, ours
    assert ours.PACKED_SLOT_BYTES == (384, 0, 0)
    _switch(1)
    try:
        before = kernels.counters["spmm_packed"]
        out, overflows = _two_steps(task, cuda)
    finally:
        _switch(None)
    assert kernels.counters["spmm_packed"] - before == 2      # layer 1 of each of the two forwards
    assert overflows == [0, 0]                                # ... and they gathered the slots
    _same(out, dense_steps)


def test_overflowing_layers_fall_back_and_equal(task, cuda, dense_steps, monkeypatch):
    from sgformer_amd import kernels, ours
    monkeypatch.setattr(ours, "PACKED_SLOT_BYTES", (384, 448, 448))
    before = kernels.counters["spmm_packed"]
    out, overflows = _two_steps(task, cuda)
    assert kernels.counters["spmm_packed"] - before == 6
    assert overflows[0] == 0 and overflows[3] == 0
    assert all(o > 0 for i, o in enumerate(overflows) if i % 3)   # layers 2 and 3: some rows hold more than 208 non-zeros
    _same(out, dense_steps)
