"""The host side of dropout under hipGraph replay (sgformer_amd/graphed.py), on the CPU: inside a seed scope
ops.dropout_res takes slots of the seed bank instead of drawing from torch's generator, and graphed.draw_seeds — what
refills a bank before a replay — yields exactly the seeds the eager forwards draw."""
import pytest
import torch


class _Bank:
    """kernels.SeedBank's interface on a host tensor (the real one allocates on the GPU)."""

    def __init__(self, capacity):
        from sgformer_amd import kernels
        self.seeds = torch.zeros(capacity, dtype=torch.int64)
        self.used = 0
        self.take = kernels.SeedBank.take.__get__(self)


@pytest.fixture
def table():
    from sgformer_amd import kernels, ops
    from tests.cpu_kernels_dropout import CpuKernelsDropout
    t = CpuKernelsDropout()
    prev = ops.set_kernels(t)
    yield t
    kernels.end_seed_scope()
    ops.set_kernels(prev)


def _inputs():
    g = torch.Generator().manual_seed(0)
    return torch.rand(6, 8, generator=g) + 0.5, torch.rand(6, 8, generator=g)


def test_a_seed_scope_draws_nothing_and_takes_the_slots_in_order(table):
    from sgformer_amd import kernels, ops
    x, res = _inputs()
    bank = _Bank(8)
    bank.seeds.copy_(torch.arange(100, 108))
    torch.manual_seed(3)
    state = torch.random.get_rng_state()
    kernels.begin_seed_scope(bank)
    xg = x.clone().requires_grad_(True)
    ys = [ops.dropout_res(xg, res if k % 2 else None, 0.5) for k in range(5)]
    kernels.end_seed_scope()
    assert torch.equal(torch.random.get_rng_state(), state)                  # no draw
    assert table.calls == [("dropout_dev", k, 100 + k) for k in range(5)]     # slots 0..4, in call order
    assert bank.used == 5
    # the backward reads the forward's slot (after the scope has ended: the slot travels with the autograd node)
    table.calls.clear()
    ys[3].sum().backward()
    assert table.calls == [("dropout_dev", 3, 103)]
    assert torch.equal(torch.random.get_rng_state(), state)
    assert torch.equal(xg.grad != 0, (ys[3].detach() - res) != 0)


def test_a_full_bank_is_an_error_not_a_wrapped_slot(table):
    from sgformer_amd import kernels, ops
    x, _ = _inputs()
    kernels.begin_seed_scope(_Bank(2))
    ops.dropout_res(x, None, 0.5)
    ops.dropout_res(x, None, 0.5)
    with pytest.raises(RuntimeError, match="dropout calls in one captured step"):
        ops.dropout_res(x, None, 0.5)


@pytest.mark.parametrize("k", [1, 4, 7])
def test_the_refill_draws_what_the_eager_forwards_draw(table, k):
    from sgformer_amd import graphed, ops
    x, res = _inputs()
    torch.manual_seed(11)
    for _ in range(k):
        ops.dropout_res(x, res, 0.2)
    eager = [c[2] for c in table.calls]
    after_eager = torch.random.get_rng_state()
    assert [c[:2] for c in table.calls] == [("dropout", None)] * k
    torch.manual_seed(11)
    host = torch.full((k + 2,), -1, dtype=torch.int64)
    drawn = graphed.draw_seeds(k, host)
    assert drawn.tolist() == eager and host[k:].tolist() == [-1, -1]
    assert torch.equal(torch.random.get_rng_state(), after_eager)            # the generator is where K eager calls leave it
    torch.manual_seed(11)
    assert graphed.draw_seeds(k).tolist() == eager
    assert all(0 <= s < 2 ** 62 for s in eager) and (k == 1 or len(set(eager)) == k)


def test_outside_a_scope_one_draw_per_call(table):
    from sgformer_amd import kernels, ops
    x, res = _inputs()
    assert kernels.seed_scope() is None
    torch.manual_seed(5)
    want = [int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64)) for _ in range(3)]
    torch.manual_seed(5)
    state = torch.random.get_rng_state()
    ys = []
    for _ in range(3):
        ys.append(ops.dropout_res(x, res, 0.5))
        now = torch.random.get_rng_state()
        assert not torch.equal(now, state)
        state = now
    assert table.calls == [("dropout", None, s) for s in want]
    torch.manual_seed(5)
    assert torch.equal(ops.dropout_res(x, res, 0.5), ys[0])


def test_eligibility_follows_the_switch_the_table_and_the_width(monkeypatch):
    """graphed._eligible's dropout clause in isolation: both branches' sites must take the fused kernel, the table must have
    dropout_dev, and SGF_GRAPH_DROPOUT=0 restores 'active dropout means eager'."""
    from types import SimpleNamespace as NS
    from sgformer_amd import graphed
    lin = lambda d: [NS(out_features=d)]
    assert graphed._fused_dropout_sites(NS(fcs=lin(64))) and not graphed._fused_dropout_sites(NS(fcs=lin(66)))
    assert not graphed._fused_dropout_sites(NS())
    monkeypatch.delenv("SGF_GRAPH_DROPOUT", raising=False)
    default = graphed.graph_dropout()
    monkeypatch.setenv("SGF_GRAPH_DROPOUT", "0")
    assert not graphed.graph_dropout()
    monkeypatch.setenv("SGF_GRAPH_DROPOUT", "1")
    assert graphed.graph_dropout()
    assert default == (graphed.GRAPH_DROPOUT_DEFAULT != "0")       # unset: the measured default
    model = NS(trans_conv=NS(dropout=0.5), graph_conv=NS(dropout=0.2))
    assert graphed._drop_state(model) == (0.5, 0.2)
    model.graph_conv.dropout = 0.3
    assert graphed._drop_state(model) == (0.5, 0.3)
