"""The head on selected rows on the GPU (csrc/head_rows.hip through sgformer_amd/head_rows.py): exact-arithmetic parity of
both entries on small integers, the cross-entropy form against fp64, and the neighbour-sampled trainer's two lines on the
100M model with SGF_SEED_HEAD on and off.

Exact arithmetic: x1, x2 integers in [-4, 4], (a, b) = (0.5, 0.5) — every z is a multiple of 0.5 of magnitude <= 4, which
bf16 holds exactly — W, bias and dlogits integers in [-2, 2].  A logit is a sum of at most 256 products of magnitude <= 8 plus
a bias: below 2^11 + 2, a multiple of 0.5; a dX element a sum of at most 256 products <= 4, halved; a dW element a sum of at
most 1000 products <= 8.  All of them are multiples of 0.25 below 2^14: exact in fp32 in ANY order of summation, so the kernels
must give the fp64 formula bit for bit (dX: rounded once to the storage dtype)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N = 4099                                 # the zero fill ends mid-tile
ROW_FORMS = [("prefix", 1), ("prefix", 31), ("prefix", 33), ("prefix", 1000), ("index", 257)]
DTYPES = [torch.float32, torch.bfloat16]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


_cache = {}


def _exact_operands(d, c):
    """Integer operands, made once per shape and shared (never written)."""
    key = (d, c)
    if key not in _cache:
        g = torch.Generator().manual_seed(1000 * d + c)
        x1 = torch.randint(-4, 5, (N, d), generator=g).double()
        x2 = torch.randint(-4, 5, (N, d), generator=g).double()
        w = torch.randint(-2, 3, (c, d), generator=g).double()
        bias = torch.randint(-2, 3, (c,), generator=g).double()
        idx = torch.randperm(N, generator=g)[:257]
        dl = torch.randint(-2, 3, (1000, c), generator=g).double()
        _cache[key] = (x1, x2, w, bias, idx, dl)
    return _cache[key]


def _exact_reference(d, c, form, m, with_x2, dtype):
    """(sel, logits, dx1, dx2, dw, db) of the fp64 formula; dx rounded once to the storage dtype."""
    x1, x2, w, bias, idx, dl = _exact_operands(d, c)
    sel = torch.arange(m) if form == "prefix" else idx[:m]
    z = 0.5 * x1[sel] + (0.5 * x2[sel] if with_x2 else 0.0)
    logits = z @ w.t() + bias
    g = dl[:m]
    dx = g @ w
    dx1 = torch.zeros(N, d, dtype=torch.float64)
    dx1[sel] = 0.5 * dx
    return sel, z, logits, dx1.float().to(dtype), g.t() @ z, g.sum(0)


@pytest.mark.parametrize("d", [32, 128, 256])
@pytest.mark.parametrize("c", [2, 47, 64, 65, 172, 256])
def test_exact_reference_is_exactly_representable(d, c):
    """On the CPU: the fp64 reference of these inputs holds nothing fp32 (or, for z and the operands, bf16) would round, so
    `torch.equal` below cannot hide a case."""
    x1, x2, w, bias, idx, dl = _exact_operands(d, c)
    for t in (x1, x2, w, bias, dl):
        assert torch.equal(t.bfloat16().double(), t)
    for form, m in ROW_FORMS:
        for with_x2 in (True, False):
            sel, z, logits, dx1, dw, db = _exact_reference(d, c, form, m, with_x2, torch.float32)
            assert torch.equal(z.bfloat16().double(), z) and float(z.abs().max()) <= 4
            assert sel.unique().numel() == m
            for t in (logits, dw, db):
                assert torch.equal(t.float().double(), t) and float(t.abs().max()) < 2 ** 14
                assert torch.equal((4 * t).round(), 4 * t)
            assert float(logits.abs().max()) < 2 ** 11 + 2
            full = torch.zeros(N, d, dtype=torch.float64)
            full[sel] = 0.5 * (dl[:m] @ w)
            assert torch.equal(dx1.double(), full)                  # fp32 holds dX exactly (bf16 rounds it, once)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("d", [32, 128, 256])
@pytest.mark.parametrize("c", [2, 47, 64, 65, 172, 256])
def test_exact_parity_of_both_entries(cuda, dtype, d, c):
    from sgformer_amd.head_rows import _Hip
    x1, x2, w, bias, idx, dl = _exact_operands(d, c)
    gx1, gx2 = x1.to(dtype).to(cuda), x2.to(dtype).to(cuda)
    gw, gb, gidx, gdl = w.float().to(cuda), bias.float().to(cuda), idx.to(cuda), dl.float().to(cuda)
    assert _Hip.head_rows_supported(d, c, dtype)
    for form, m in ROW_FORMS:
        for with_x2 in (True, False):
            sel, z, logits, dx1, dw, db = _exact_reference(d, c, form, m, with_x2, dtype)
            tag = (form, m, with_x2)
            ix = None if form == "prefix" else gidx[:m].contiguous()
            got = _Hip.head_rows_fwd(gx1, 0.5, gx2 if with_x2 else None, 0.5, gw, gb, ix, m)[0]
            assert got.shape == (m, c) and torch.equal(got.cpu().double(), logits), tag
            r1, r2, rw, rb = _Hip.head_rows_bwd(gx1, 0.5, gx2 if with_x2 else None, 0.5, gw, ix, m, dlogits=gdl[:m].contiguous())
            assert torch.equal(r1.cpu(), dx1), tag
            assert (r2 is None) == (not with_x2), tag
            if with_x2:
                assert torch.equal(r2.cpu(), dx1), tag                   # b == a
            off = torch.ones(N, dtype=torch.bool)
            off[sel] = False
            assert int(r1[off.to(cuda)].count_nonzero()) == 0, tag
            assert torch.equal(rw.cpu().double(), dw) and torch.equal(rb.cpu().double(), db), tag


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_exact_parity_through_autograd_with_unequal_weights_and_strided_rows(cuda, dtype):
    """(a, b) = (0.5, 0.25) — dx2 differs from dx1 — on column slices of wider tensors, through head_rows.logits."""
    from sgformer_amd import head_rows
    d, c, m = 128, 47, 33
    x1, x2, w, bias, idx, dl = _exact_operands(d, c)
    wide = torch.zeros(N, 2 * d, dtype=dtype)
    wide[:, :d], wide[:, d:] = x1.to(dtype), x2.to(dtype)
    wide = wide.to(cuda).requires_grad_(True)
    gw, gb = w.float().to(cuda).requires_grad_(True), bias.float().to(cuda).requires_grad_(True)
    out = head_rows.logits(wide[:, :d], wide[:, d:], gw, gb, 0.5, 0.25, m)
    z = 0.5 * x1[:m] + 0.25 * x2[:m]
    assert torch.equal(out.detach().cpu().double(), z @ w.t() + bias)
    (out * dl[:m].float().to(cuda)).sum().backward()
    dx = dl[:m] @ w
    want = torch.zeros(N, 2 * d, dtype=torch.float64)
    want[:m, :d], want[:m, d:] = 0.5 * dx, 0.25 * dx
    assert torch.equal(wide.grad.cpu(), want.float().to(dtype))
    assert torch.equal(gw.grad.cpu().double(), dl[:m].t() @ z) and torch.equal(gb.grad.cpu().double(), dl[:m].sum(0))


# ------------------------------------------------------------------------------------------------
# the cross-entropy form
# ------------------------------------------------------------------------------------------------
def _ce_operands(d, c):
    """x1, x2 multiples of 1/8 in [-4, 4) — (x1 + x2) / 2 and x1 / 2 are then exact in bf16 and fp32 alike, so the reference's
    z is the kernel's — and W, bias of unit scale; made once per shape and shared (never written)."""
    key = ("ce", d, c)
    if key not in _cache:
        g = torch.Generator().manual_seed(7000 * d + c)
        x1 = torch.randint(-32, 32, (N, d), generator=g).double() / 8
        x2 = torch.randint(-32, 32, (N, d), generator=g).double() / 8
        w = torch.randn(c, d, generator=g)
        bias = torch.randn(c, generator=g)
        idx = torch.randperm(N, generator=g)[:257]
        labels = torch.randint(0, c, (1000,), generator=g)
        _cache[key] = (x1, x2, w, bias, idx, labels)
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("d", [32, 128, 256])
@pytest.mark.parametrize("c", [2, 47, 64, 65, 172, 256])
def test_cross_entropy_form(cuda, dtype, d, c):
    """The kernel cases of the exact test — every row form, x2 present and absent — with logits of about 3 randn (as
    tests/test_gpu_kernels.py::test_fused_loss) and its bars: loss within 2e-6 |ref| + 1e-6 of fp64, every gradient within 2e-6
    (fp32) / 5e-3 (bf16) in relative norm, counts equal to torch's integer counts on the kernel's own logits.  W is rounded to
    the storage dtype for bf16, as the entry documents.  Where the selection has at least 8 rows, three labels are outside
    [0, C): -100, C and -1."""
    from sgformer_amd import head_rows
    from sgformer_amd.head_rows import _Hip
    x1, x2, w0, bias, idx, labels0 = _ce_operands(d, c)
    g1, g2, gb = x1.to(dtype).to(cuda), x2.to(dtype).to(cuda), bias.to(cuda)
    bar = 2e-6 if dtype == torch.float32 else 5e-3
    for form, m in ROW_FORMS:
        for with_x2 in (True, False):
            tag = (form, m, with_x2)
            # var(x) = 5.33: z = (x1 + x2) / 2 has variance 2.67, z = x1 / 2 has 1.33; logits ~ 3 randn either way
            w = w0 * 3 / (d * (2.67 if with_x2 else 1.33)) ** 0.5
            sel = torch.arange(m) if form == "prefix" else idx[:m]
            labels = labels0[:m].clone()
            if m >= 8:
                labels[0], labels[5], labels[m - 1] = -100, c, -1
            ok = (labels >= 0) & (labels < c)
            wr = (w.to(dtype) if dtype == torch.bfloat16 else w).double()
            leaves = [t.clone().requires_grad_(True) for t in ((x1, x2, wr, bias.double()) if with_x2 else (x1, wr, bias.double()))]
            l1, l2, lw, lb = leaves if with_x2 else (leaves[0], None, leaves[1], leaves[2])
            z = 0.5 * l1[sel] + 0.5 * l2[sel] if with_x2 else 0.5 * l1[sel]
            ref = F.cross_entropy(z @ lw.t() + lb, torch.where(ok, labels, torch.tensor(-100)))
            ref.backward()

            t1 = g1.clone().requires_grad_(True)
            t2 = g2.clone().requires_grad_(True) if with_x2 else None
            tw, tb = w.to(cuda).requires_grad_(True), gb.clone().requires_grad_(True)
            rows = m if form == "prefix" else sel.to(cuda)
            glabels = labels.to(cuda)
            loss = head_rows.cross_entropy(t1, t2, tw, tb, 0.5, 0.5, rows, glabels)
            loss.backward()
            err = abs(float(loss.detach()) - float(ref.detach()))
            print(f"{tag} loss {float(loss.detach()):.8f} ref {float(ref.detach()):.8f} diff {err:.2e}")
            assert err <= 2e-6 * abs(float(ref.detach())) + 1e-6, tag
            pairs = [("dx1", t1.grad, l1.grad), ("dw", tw.grad, lw.grad), ("db", tb.grad, lb.grad)]
            if with_x2:
                pairs.append(("dx2", t2.grad, l2.grad))
            for name, got, want in pairs:
                r = _rel(got.cpu(), want)
                print(f"  {name} {r:.2e}")
                assert r <= bar, (tag, name, r)
            off = torch.ones(N, dtype=torch.bool)
            off[sel] = False
            assert int(t1.grad[off.to(cuda)].count_nonzero()) == 0, tag
            if m >= 8:
                assert int(t1.grad[sel[0]].count_nonzero()) == 0, tag          # an ignored label: a zero gradient row
            # the forward entry itself: logits, lse, summed loss and counts of one launch
            ix = None if form == "prefix" else rows.contiguous()
            lg, lse, loss_sum, counts = _Hip.head_rows_fwd(t1.detach(), 0.5, None if t2 is None else t2.detach(), 0.5,
                                                           tw.detach(), tb.detach(), ix, m, glabels)
            lg = lg.cpu()
            hits = (lg.argmax(1) == labels) & ok
            assert counts.tolist() == [int(ok.sum()), int(hits.sum())], tag
            # lse = max + log(sum of exp), in fp32: the maximum is exact, expf / logf and the two sums round a few times at
            # the scale of the logits — 4 ulps there; the maximum and the log can cancel, so the bound is absolute, not relative
            scale = max(1.0, float(lg.abs().max()))
            assert float((lse.cpu().double() - torch.logsumexp(lg.double(), 1)).abs().max()) <= 2.0 ** -22 * scale, tag
            assert abs(float(loss_sum) / int(ok.sum()) - float(ref.detach())) <= 2e-6 * abs(float(ref.detach())) + 1e-6, tag
            assert torch.equal(loss_sum[0] / counts[0].float(), loss.detach()), tag     # deterministic: the same bits again


@pytest.mark.gpu
def test_no_rows_and_all_labels_ignored_on_the_device(cuda):
    from sgformer_amd import head_rows
    d, c = 64, 7
    g = torch.Generator().manual_seed(0)
    for dtype in DTYPES:
        ins = [torch.randn(50, d, generator=g).to(dtype).to(cuda).requires_grad_(True) for _ in range(2)]
        ins += [torch.randn(c, d, generator=g).to(cuda).requires_grad_(True), torch.randn(c, generator=g).to(cuda).requires_grad_(True)]
        for rows, labels in ((0, torch.zeros(0, dtype=torch.int64)), (3, torch.tensor([-100, c, -5]))):
            for t in ins:
                t.grad = None
            loss = head_rows.cross_entropy(*ins, 0.8, 0.2, rows, labels.to(cuda))
            assert torch.isnan(loss)
            loss.backward()
            assert all(t.grad is not None and int(t.grad.count_nonzero()) == 0 for t in ins)
        _, _, loss_sum, counts = head_rows._Hip.head_rows_fwd(ins[0].detach(), 0.8, ins[1].detach(), 0.2, ins[2].detach(),
                                                              ins[3].detach(), None, 0, torch.zeros(0, dtype=torch.int64, device=cuda))
        assert float(loss_sum) == 0.0 and counts.tolist() == [0, 0]
        assert head_rows.logits(*ins, 0.8, 0.2, 0).shape == (0, c)


# ------------------------------------------------------------------------------------------------
# the model: the trainer's lines on a sampled batch
# ------------------------------------------------------------------------------------------------
F_IN, HIDDEN, SEEDS = 32, 128, 64


@pytest.fixture(scope="module")
def batch(cuda):
    """One NeighborLoader batch of a synthetic 20 000-node parent, fan-outs [5, 3], 64 seeds: a few thousand nodes."""
    from oracle import sgformer_oracle as O
    from sgformer_amd.sampling import NeighborLoader
    n = 20000
    torch.manual_seed(0)

    class Data:
        pass
    data = Data()
    data.x, data.y, data.edge_index = torch.randn(n, F_IN), torch.randint(0, 47, (n,)), O.synthetic_graph(n, 10.0, seed=6)
    loader = NeighborLoader(data, input_nodes=torch.arange(0, SEEDS), num_neighbors=[5, 3], batch_size=SEEDS, seed=5)
    graph = next(iter(loader)).to(cuda)
    assert graph.batch_size == SEEDS and graph.edge_index._sgf_seed_count == SEEDS and 500 < graph.x.shape[0] < 10000
    return graph


@pytest.fixture
def hook():
    from sgformer_amd import launch
    launch.patch_ce_loss()
    yield
    launch.unpatch_ce_loss()


def _build(c, layers, cuda, compute_dtype=None):
    from oracle import sgformer_oracle as O
    from sgformer_amd.ours_100m import SGFormer
    cfg = dict(alpha=0.5, trans_num_layers=layers, gnn_num_layers=layers, gnn_use_init=True, graph_weight=0.8)
    p = O.init_params(cfg, F_IN, HIDDEN, c, seed=2)
    m = SGFormer(F_IN, HIDDEN, c, trans_dropout=0.0, gnn_dropout=0.0, compute_dtype=compute_dtype, **cfg)
    m.load_state_dict({**m.state_dict(), **p})
    return cfg, p, m.to(cuda).train()


def _trainer_step(m, graph, y):
    """100M/nb-sample.py:27-33 in this test's own words."""
    bs = graph.batch_size
    m.zero_grad(set_to_none=True)
    output = m(graph.x, graph.edge_index)[:bs]
    loss = torch.nn.CrossEntropyLoss()(output, y[:bs])
    loss.backward()
    return output, loss.detach(), {k: prm.grad.detach().clone() for k, prm in m.named_parameters() if prm.grad is not None}


def _oracle_step(cfg, p, graph, y):
    from oracle import sgformer_oracle as O
    bs = graph.batch_size
    p64 = {k: v.double().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in p.items()}
    ref = O.sgformer_forward(p64, graph.x.double().cpu(), graph.edge_index.cpu(), cfg, training=True)[:bs]
    O_loss = F.cross_entropy(ref, y[:bs].cpu())
    O_loss.backward()
    return ref.detach(), float(O_loss), {k: v.grad for k, v in p64.items() if v.grad is not None}


@pytest.mark.gpu
@pytest.mark.parametrize("c", [172, 47])
@pytest.mark.parametrize("layers", [1, 2])
def test_trainer_lines_fp32_against_the_oracle(cuda, batch, hook, monkeypatch, c, layers):
    """fp32 storage, the bars of tests/test_gpu_kernels.py::test_fp32_module_runs_without_a_library_gemm: logits within 1e-4,
    every parameter gradient within 5e-4 |g| + 1e-6 gmax.  Then the switch at 0 against a batch that carries no seed count:
    the same bits.  That shows the switch is inert at 0 — both runs are this code; that the head's arithmetic is the one from
    before the lazy head existed is what the oracle and golden tests of the full head (tests/test_gpu_golden.py,
    tests/test_gpu_sampler.py) pin, not this test."""
    from sgformer_amd import graph as G
    from sgformer_amd.head_rows import LazyHead
    cfg, p, m = _build(c, layers, cuda)
    y = (batch.y % c).contiguous()
    ref, ref_loss, ref_g = _oracle_step(cfg, p, batch, y)
    monkeypatch.setenv("SGF_SEED_HEAD", "1")
    output, loss, grads = _trainer_step(m, batch, y)
    assert type(output) is LazyHead and output.shape == (SEEDS, c)
    logits = output.float()                                   # the rows' values, computed now
    assert type(logits) is torch.Tensor
    assert float((logits.detach().double().cpu() - ref).abs().max()) <= 1e-4
    assert abs(float(loss) - ref_loss) <= 1e-5
    gmax = max(float(g.norm()) for g in ref_g.values())
    assert set(grads) == set(ref_g)
    for k, g in ref_g.items():
        assert float((grads[k].double().cpu() - g).norm()) <= 5e-4 * float(g.norm()) + 1e-6 * gmax, k
    # SGF_SEED_HEAD=0 on the marked batch == an unmarked batch with the switch unset: the switch does nothing at 0
    monkeypatch.setenv("SGF_SEED_HEAD", "0")
    out0, loss0, grads0 = _trainer_step(m, batch, y)
    bare = batch.edge_index.clone()
    G.hints_of(batch.edge_index).attach(bare)
    assert not hasattr(bare, "_sgf_seed_count")
    monkeypatch.delenv("SGF_SEED_HEAD")
    m.zero_grad(set_to_none=True)
    out1 = m(batch.x, bare)[:SEEDS]
    loss1 = torch.nn.CrossEntropyLoss()(out1, y[:SEEDS])
    loss1.backward()
    assert type(out0) is torch.Tensor and torch.equal(out0, out1) and torch.equal(loss0, loss1.detach())
    for k, prm in m.named_parameters():
        if prm.grad is not None:
            assert torch.equal(grads0[k], prm.grad), k


@pytest.mark.gpu
@pytest.mark.parametrize("c", [172, 47])
@pytest.mark.parametrize("layers", [1, 2])
def test_trainer_lines_bf16_no_worse_than_twice_the_existing_path(cuda, batch, hook, monkeypatch, c, layers):
    """bf16 storage: per tensor, the error of the new path against the fp64 oracle is at most 2 x the error of the switch-off
    path on the same inputs + 1e-6 gmax (the project's 2x rule).  Both errors are printed."""
    cfg, p, m = _build(c, layers, cuda, torch.bfloat16)
    m.logits_dtype = torch.float32
    y = (batch.y % c).contiguous()
    ref, ref_loss, ref_g = _oracle_step(cfg, p, batch, y)
    gmax = max(float(g.norm()) for g in ref_g.values())
    monkeypatch.setenv("SGF_SEED_HEAD", "1")
    out_on, loss_on, g_on = _trainer_step(m, batch, y)
    lg_on = out_on.float().detach().double().cpu()
    monkeypatch.setenv("SGF_SEED_HEAD", "0")
    out_off, loss_off, g_off = _trainer_step(m, batch, y)
    lg_off = out_off.float().detach().double().cpu()
    e_on, e_off = float((lg_on - ref).norm()), float((lg_off - ref).norm())
    print(f"C={c} layers={layers} logits: on {e_on:.3e} off {e_off:.3e} | loss on {abs(float(loss_on) - ref_loss):.3e} "
          f"off {abs(float(loss_off) - ref_loss):.3e}")
    assert e_on <= 2 * e_off + 1e-6 * float(ref.norm())
    assert set(g_on) == set(ref_g)
    for k, g in ref_g.items():
        a_on, a_off = float((g_on[k].double().cpu() - g).norm()), float((g_off[k].double().cpu() - g).norm())
        print(f"  {k}: on {a_on:.3e} off {a_off:.3e} |g| {float(g.norm()):.3e}")
        assert a_on <= 2 * a_off + 1e-6 * gmax, k


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [None, torch.bfloat16], ids=["f32", "bf16"])
def test_evaluation_lines_and_full_materialisation(cuda, batch, hook, monkeypatch, dtype):
    """100M/nb-sample.py:39-45 (`model.eval()`, no_grad, `[:k].argmax(-1) == y[:k]`): the same hit count with the switch on and
    off; a lazy head that is read in full after its rows were used is the existing logits."""
    c = 172
    _, _, m = _build(c, 1, cuda, dtype)
    m.logits_dtype = torch.float32
    m.eval()
    y = (batch.y % c).contiguous()
    k = batch.batch_size
    with torch.no_grad():
        monkeypatch.setenv("SGF_SEED_HEAD", "0")
        full_off = m(batch.x, batch.edge_index)
        hits_off = int((full_off[:k].argmax(dim=-1) == y[:k]).sum())
        monkeypatch.setenv("SGF_SEED_HEAD", "1")
        lazy = m(batch.x, batch.edge_index)
        rows = lazy[:k]
        hits_on = int((rows.argmax(dim=-1) == y[:k]).sum())
        assert hits_on == hits_off
        assert torch.equal(lazy + 0.0, full_off)
        # the explicit interface: an index and a mask give the rows of the full result to the kernel's rounding
        idx = torch.randperm(batch.x.shape[0], generator=torch.Generator().manual_seed(1))[:100].to(cuda)
        mask = torch.zeros(batch.x.shape[0], dtype=torch.bool, device=cuda)
        mask[idx] = True
        tol = 1e-4 if dtype is None else 2e-2
        assert float((m.forward_rows(batch.x, batch.edge_index, idx) - full_off[idx]).abs().max()) <= tol
        assert float((m.forward_rows(batch.x, batch.edge_index, mask) - full_off[mask]).abs().max()) <= tol


@pytest.mark.gpu
def test_forward_rows_on_a_reordered_graph(cuda):
    """A graph whose cached view carries a node permutation (re-order mode 'always'): the branches run in the view's order and
    forward_rows maps the caller's rows through the inverse permutation.  fp32, eval mode: every form of `rows` gives the
    rows of forward's result to fp32 summation order (1e-4, the logits bar above; two different rows differ by O(1)), and
    cross_entropy_rows the trainer's loss and gradients on them."""
    from oracle import sgformer_oracle as O
    from sgformer_amd import ops
    from sgformer_amd.loss import cross_entropy_rows
    from sgformer_amd.ours_100m import SGFormer
    n, c = 3000, 47
    cfg = dict(alpha=0.5, trans_num_layers=1, gnn_num_layers=2, gnn_use_init=True, graph_weight=0.8)
    torch.manual_seed(3)
    x, ei = torch.randn(n, F_IN).to(cuda), O.synthetic_graph(n, 8.0, seed=9).to(cuda)
    y = torch.randint(0, c, (n, 1)).to(cuda)
    m = SGFormer(F_IN, HIDDEN, c, trans_dropout=0.0, gnn_dropout=0.0, **cfg)
    m.load_state_dict({**m.state_dict(), **O.init_params(cfg, F_IN, HIDDEN, c, seed=5)})
    m = m.to(cuda).train()
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(2))[:129].to(cuda)
    mask = torch.zeros(n, dtype=torch.bool, device=cuda)
    mask[idx[:40]] = True
    prev = ops.set_reorder_mode("always")
    try:
        ops.graph_cache.clear()
        full = m(x, ei)
        view = ops.graph_cache.get(ei, n).view()
        assert view.perm is not None and not torch.equal(view.perm.long(), torch.arange(n, device=cuda))
        for rows, want in ((idx, full[idx]), (70, full[:70]), (mask, full[mask])):
            got = m.forward_rows(x, ei, rows)
            assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-4
        ref = F.cross_entropy(full[idx], y.squeeze(1)[idx])
        m.zero_grad(set_to_none=True)
        ref.backward()
        want_g = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
        m.zero_grad(set_to_none=True)
        loss = cross_entropy_rows(m, x, ei, y, idx)
        loss.backward()
        assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-5
        gmax = max(float(g.norm()) for g in want_g.values())
        for k, p in m.named_parameters():
            if p.grad is not None:
                assert float((p.grad - want_g[k]).norm()) <= 5e-4 * float(want_g[k].norm()) + 1e-6 * gmax, k
    finally:
        ops.set_reorder_mode(prev)
        ops.graph_cache.clear()
