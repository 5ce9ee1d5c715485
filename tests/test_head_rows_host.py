"""The head on selected rows (sgformer_amd/head_rows.py, include/sgf.h block N6) without a GPU: the two autograd Functions
against fp64 torch on a CPU kernel table (tests/cpu_kernels_head_rows.py), the fallback, SGFormer.forward_rows, the lazy head
of the unchanged trainer with its F.cross_entropy hook, and what the two call sites hand libsgf (a recording stand-in, pinned
against tests/golden/head_rows_calls.json).

`python tests/test_head_rows_host.py --write` regenerates the golden file from the code as it stands.
"""
import contextlib
import copy
import json
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.cpu_kernels_head_rows import CpuKernelsHeadRows  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "head_rows_calls.json")

# One bf16 rounding is a relative error of at most 2^-9.  The fp64 reference below keeps the stored operands and rounds
# nothing; the op rounds z, W, the gradient operand of dX and dX itself: four roundings in the longest chain, 4 * 2^-9 < 8e-3.
# fp32: sums of at most 256 products at 2^-24 each.
TOL = {torch.float32: 2e-5, torch.bfloat16: 8e-3}


@pytest.fixture
def table():
    from sgformer_amd import ops
    CpuKernelsHeadRows.calls = {}
    prev = ops.set_kernels(CpuKernelsHeadRows())
    yield CpuKernelsHeadRows
    ops.set_kernels(prev)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _operands(n, d, c, dtype, with_x2=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn(n, d, generator=g).to(dtype)
    x2 = torch.randn(n, d, generator=g).to(dtype) if with_x2 else None
    w = torch.randn(c, d, generator=g) / d ** 0.5
    bias = torch.randn(c, generator=g)
    return x1, x2, w, bias


def _rows_forms(n, form):
    if form == "prefix":
        return 13, torch.arange(13)
    if form == "index":
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:17]
        return idx, idx
    mask = torch.zeros(n, dtype=torch.bool)
    mask[torch.tensor([0, 5, 6, 21, n - 1])] = True
    return mask, mask.nonzero().view(-1)


def _ref_logits(x1, x2, w, bias, a, b, sel):
    """fp64, the stored operands as they are: (leaves, logits of the rows sel)"""
    leaves = [t.double().requires_grad_(True) if t is not None else None for t in (x1, x2, w, bias)]
    l1, l2, lw, lb = leaves
    z = a * l1[sel] if l2 is None else a * l1[sel] + b * l2[sel]
    return leaves, z @ lw.t() + lb


def _grads(leaves):
    return [None if t is None else (t.grad if t.grad is not None else torch.zeros_like(t)) for t in leaves]


def _check_grads(got, want, tol, what):
    for name, g, r in zip(("x1", "x2", "w", "bias"), got, want):
        if r is None:
            assert g is None, (what, name)
            continue
        assert g is not None and g.shape == r.shape, (what, name)
        if float(r.norm()) == 0.0:
            assert float(g.double().abs().max()) == 0.0, (what, name)
        else:
            assert _rel(g, r) <= tol, (what, name, _rel(g, r))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("form", ["prefix", "index", "mask"])
@pytest.mark.parametrize("c,with_x2", [(2, True), (47, True), (172, True), (47, False)])
def test_logits_function_matches_fp64(table, dtype, form, c, with_x2):
    from sgformer_amd import head_rows
    n, d, a, b = 40, 32, 0.8, 0.2
    x1, x2, w, bias = _operands(n, d, c, dtype, with_x2)
    rows, sel = _rows_forms(n, form)
    ins = [t.clone().requires_grad_(True) if t is not None else None for t in (x1, x2, w, bias)]
    out = head_rows.logits(ins[0], ins[1], ins[2], ins[3], a, b, rows)
    assert out.dtype == torch.float32 and out.shape == (sel.numel(), c)
    wgt = torch.randn(out.shape, generator=torch.Generator().manual_seed(5))
    (out * wgt).sum().backward()
    leaves, ref = _ref_logits(x1, x2, w, bias, a, b, sel)
    (ref * wgt.double()).sum().backward()
    assert _rel(out, ref) <= TOL[dtype]
    _check_grads([t.grad if t is not None else None for t in ins], _grads(leaves), TOL[dtype], (form, c))
    off = torch.ones(n, dtype=torch.bool)
    off[sel] = False
    assert int(ins[0].grad[off].count_nonzero()) == 0
    assert table.calls["head_rows_fwd"] == [sel.numel()] and table.calls["head_rows_bwd"] == [sel.numel()]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("form", ["prefix", "index", "mask"])
@pytest.mark.parametrize("c,with_x2", [(2, True), (47, True), (172, True), (47, False)])
def test_cross_entropy_function_matches_fp64(table, dtype, form, c, with_x2):
    """Labels with ignore_index (-100) and with a class outside [0, C): neither adds to the loss, the count or the gradient."""
    from sgformer_amd import head_rows
    n, d, a, b = 40, 32, 0.5, 0.5
    x1, x2, w, bias = _operands(n, d, c, dtype, with_x2, seed=1)
    rows, sel = _rows_forms(n, form)
    m = sel.numel()
    labels = torch.randint(0, c, (m,), generator=torch.Generator().manual_seed(7))
    labels[1], labels[3] = -100, c + 3
    ins = [t.clone().requires_grad_(True) if t is not None else None for t in (x1, x2, w, bias)]
    loss = head_rows.cross_entropy(ins[0], ins[1], ins[2], ins[3], a, b, rows, labels)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    (loss * 1.5).backward()
    leaves, ref = _ref_logits(x1, x2, w, bias, a, b, sel)
    ref_labels = labels.clone()
    ref_labels[3] = -100
    ref_loss = F.cross_entropy(ref, ref_labels)
    (ref_loss * 1.5).backward()
    assert abs(float(loss) - float(ref_loss)) <= TOL[dtype] * abs(float(ref_loss)) + 1e-6
    _check_grads([t.grad if t is not None else None for t in ins], _grads(leaves), TOL[dtype], (form, c))
    assert table.calls == {"head_rows_ce": [m], "head_rows_bwd": [m]}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_no_rows_and_all_labels_ignored(table, dtype):
    from sgformer_amd import head_rows
    x1, x2, w, bias = _operands(20, 32, 7, dtype)
    ins = [t.clone().requires_grad_(True) for t in (x1, x2, w, bias)]
    out = head_rows.logits(*ins, 0.5, 0.5, 0)
    assert out.shape == (0, 7)
    out.sum().backward()
    assert all(int(t.grad.count_nonzero()) == 0 for t in ins)
    for rows, labels in ((0, torch.zeros(0, dtype=torch.int64)), (4, torch.tensor([-100, -100, 9, -1]))):
        ins = [t.clone().requires_grad_(True) for t in (x1, x2, w, bias)]
        loss = head_rows.cross_entropy(*ins, 0.5, 0.5, rows, labels)
        assert torch.isnan(loss)                       # 0 / 0, as F.cross_entropy on no (unignored) rows
        ignored = torch.where((labels >= 0) & (labels < 7), labels, torch.tensor(-100))
        assert torch.isnan(F.cross_entropy(torch.zeros(rows, 7), ignored))
        loss.backward()
        assert all(int(t.grad.count_nonzero()) == 0 for t in ins)          # exact zeros, not nan


def test_repeated_rows_take_the_fallback_and_accumulate(table):
    from sgformer_amd import head_rows
    x1, x2, w, bias = _operands(20, 32, 7, torch.float32)
    idx = torch.tensor([1, 3, 3, 7])
    labels = torch.tensor([0, 6, 2, 5])
    ins = [t.clone().requires_grad_(True) for t in (x1, x2, w, bias)]
    loss = head_rows.cross_entropy(*ins, 0.8, 0.2, idx, labels)
    loss.backward()
    leaves, ref = _ref_logits(x1, x2, w, bias, 0.8, 0.2, idx)
    F.cross_entropy(ref, labels).backward()
    assert abs(float(loss) - float(F.cross_entropy(ref, labels))) <= 1e-5
    _check_grads([t.grad for t in ins], _grads(leaves), 2e-5, "repeated")
    assert float(ins[0].grad[3].abs().sum()) > 0
    assert not any(k.startswith("head_rows") for k in table.calls)
    out = head_rows.logits(x1, x2, w, bias, 0.8, 0.2, idx)
    assert _rel(out, ref) <= 2e-5 and not any(k.startswith("head_rows") for k in table.calls)


@pytest.mark.parametrize("what", ["cat", "bf16_d48", "wide", "f64"])
def test_unsupported_shapes_take_the_fallback_with_an_equal_result(table, what):
    from sgformer_amd import head_rows
    dtype = torch.bfloat16 if what == "bf16_d48" else torch.float64 if what == "f64" else torch.float32
    n, d, c = 30, {"bf16_d48": 48, "wide": 260}.get(what, 32), 5
    x1, x2, w, bias = _operands(n, d, c, torch.float32)
    x1, x2 = x1.to(dtype), x2.to(dtype)
    if what == "cat":
        w = torch.randn(c, 2 * d, generator=torch.Generator().manual_seed(2)) / d ** 0.5
    if what == "f64":
        w, bias = w.double(), bias.double()
    rows, labels = 9, torch.arange(9) % c
    ins = [t.clone().requires_grad_(True) for t in (x1, x2, w, bias)]
    loss = head_rows.cross_entropy(*ins, 0.8, 0.2, rows, labels)
    loss.backward()
    l1, l2, lw, lb = [t.double().requires_grad_(True) for t in (x1, x2, w, bias)]
    ref = (torch.cat([l1[:9], l2[:9]], 1) if what == "cat" else 0.8 * l1[:9] + 0.2 * l2[:9]) @ lw.t() + lb
    ref_loss = F.cross_entropy(ref, labels)
    ref_loss.backward()
    tol = TOL[torch.bfloat16] if what == "bf16_d48" else 2e-5
    assert abs(float(loss) - float(ref_loss)) <= tol * abs(float(ref_loss)) + 1e-6
    _check_grads([t.grad for t in ins], [l1.grad, l2.grad, lw.grad, lb.grad], tol, what)
    assert _rel(head_rows.logits(x1, x2, w, bias, 0.8, 0.2, rows), ref) <= tol
    assert not any(k.startswith("head_rows") for k in table.calls)


def test_second_derivatives_raise(table):
    from sgformer_amd import head_rows
    x1, x2, w, bias = _operands(20, 32, 7, torch.float32)
    x1.requires_grad_(True)
    loss = head_rows.cross_entropy(x1, x2, w, bias, 0.5, 0.5, 6, torch.arange(6))
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(loss, x1, create_graph=True)
    out = head_rows.logits(x1, x2, w, bias, 0.5, 0.5, 6)
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(out.sum(), x1, create_graph=True)


def test_rows_argument_errors(table):
    from sgformer_amd import head_rows
    x1, x2, w, bias = _operands(20, 32, 7, torch.float32)
    with pytest.raises(IndexError):
        head_rows.logits(x1, x2, w, bias, 0.5, 0.5, 21)
    with pytest.raises(IndexError):
        head_rows.logits(x1, x2, w, bias, 0.5, 0.5, torch.tensor([0, 20]))
    with pytest.raises(TypeError):
        head_rows.logits(x1, x2, w, bias, 0.5, 0.5, torch.tensor([0, 2], dtype=torch.int32))
    with pytest.raises(TypeError):
        head_rows.logits(x1, x2, w, bias, 0.5, 0.5, True)
    with pytest.raises(ValueError):
        head_rows.cross_entropy(x1, x2, w, bias, 0.5, 0.5, 4, torch.arange(5))


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
def _model(c=7, aggregate="add", use_graph=True, hidden=32, seed=0):
    from sgformer_amd.ours_100m import SGFormer
    torch.manual_seed(seed)
    return SGFormer(8, hidden, c, trans_dropout=0.0, gnn_dropout=0.0, use_graph=use_graph, aggregate=aggregate)


def _same_param_grads(model, got):
    """Per parameter |g - r| <= 1e-4 |r| + 1e-6 gmax, gmax the largest gradient norm of the model: a bias in front of a
    BatchNorm has a gradient that is zero but for rounding, which only an absolute term can bound."""
    want = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert set(got) == set(want)
    gmax = max(float(r.norm()) for r in want.values())
    for n, r in want.items():
        assert float((got[n].double() - r.double()).norm()) <= 1e-4 * float(r.norm()) + 1e-6 * gmax, n


def _graph(n=60, e=300, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 8, generator=g), torch.randint(0, n, (2, e), generator=g)


@pytest.mark.parametrize("aggregate,use_graph", [("add", True), ("cat", True), ("add", False)])
def test_forward_rows_equals_the_rows_of_forward(table, aggregate, use_graph):
    model = _model(aggregate=aggregate, use_graph=use_graph).eval()
    x, ei = _graph()
    with torch.no_grad():
        full = model(x, ei)
        idx = torch.tensor([5, 0, 59, 17])
        mask = torch.zeros(60, dtype=torch.bool)
        mask[[2, 3, 40]] = True
        for rows, want in ((11, full[:11]), (idx, full[idx]), (mask, full[mask]), (0, full[:0])):
            got = model.forward_rows(x, ei, rows)
            assert got.shape == want.shape and got.dtype == want.dtype
            assert torch.allclose(got, want, rtol=1e-5, atol=1e-5)
    with pytest.raises(TypeError):
        model.forward_rows(x, ei, None)


def test_cross_entropy_rows_equals_the_trainer_lines(table):
    from sgformer_amd.loss import cross_entropy_rows
    model = _model().train()
    x, ei = _graph()
    y = torch.randint(0, 7, (60, 1), generator=torch.Generator().manual_seed(4))
    k = 16
    loss = cross_entropy_rows(model, x, ei, y, k)
    loss.backward()
    got = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad()
    ref = torch.nn.CrossEntropyLoss()(model(x, ei)[:k], y.squeeze(1)[:k])
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5
    _same_param_grads(model, got)
    assert table.calls["head_rows_ce"] == [k]
    idx = torch.tensor([3, 9, 27])
    assert abs(float(cross_entropy_rows(model, x, ei, y, idx)) - float(F.cross_entropy(model(x, ei)[idx], y.squeeze(1)[idx]))) <= 1e-5


# ------------------------------------------------------------------------------------------------
# the unchanged trainer: LazyHead and the F.cross_entropy hook
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def seed_head(table, monkeypatch):
    from sgformer_amd import launch
    monkeypatch.setenv("SGF_SEED_HEAD", "1")
    launch.unpatch_ce_loss()             # (a launcher test that ran earlier in the process may have left the hook installed)
    orig = F.cross_entropy
    launch.patch_ce_loss()
    yield table
    launch.unpatch_ce_loss()
    assert F.cross_entropy is orig


def _sampled(k=12):
    x, ei = _graph()
    ei._sgf_seed_count = k
    return x, ei, k


def _count_full_heads(model, monkeypatch):
    calls = []
    head = model._head
    monkeypatch.setattr(model, "_head", lambda *a, **kw: (calls.append(1), head(*a, **kw))[1])
    return calls


def test_switch_off_and_unmarked_batches_get_todays_logits(table, monkeypatch):
    from sgformer_amd.head_rows import LazyHead
    model = _model().eval()
    x, ei, k = _sampled()
    monkeypatch.delenv("SGF_SEED_HEAD", raising=False)
    assert type(model(x, ei)) is torch.Tensor                       # the default is off
    monkeypatch.setenv("SGF_SEED_HEAD", "0")
    assert type(model(x, ei)) is torch.Tensor
    monkeypatch.setenv("SGF_SEED_HEAD", "1")
    assert type(model(x, ei)) is LazyHead
    assert type(model(*_graph())) is torch.Tensor                   # no seed count with the edge list: not a sampled batch


def test_lazy_rows_and_cross_entropy_run_the_fused_op_once_and_never_the_full_head(seed_head, monkeypatch):
    from sgformer_amd.head_rows import LazyHead
    model = _model().train()
    x, ei, k = _sampled()
    y = torch.randint(0, 7, (60,), generator=torch.Generator().manual_seed(4))
    full = _count_full_heads(model, monkeypatch)
    out = model(x, ei)
    assert type(out) is LazyHead and out.shape == (60, 7) and out.dtype == torch.float32 and out.requires_grad
    output = out[:k]                                               # 100M/nb-sample.py:29
    assert type(output) is LazyHead and output.shape == (k, 7)
    loss = torch.nn.CrossEntropyLoss()(output, y[:k])              # 100M/nb-sample.py:30
    loss.backward()
    assert seed_head.calls == {"head_rows_ce": [k], "head_rows_bwd": [k]} and full == []
    got = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad()
    monkeypatch.setenv("SGF_SEED_HEAD", "0")
    ref = torch.nn.CrossEntropyLoss()(model(x, ei)[:k], y[:k])
    ref.backward()
    assert full == [1] and abs(float(loss) - float(ref)) <= 1e-5
    _same_param_grads(model, got)


def test_lazy_rows_argmax_computes_the_seed_rows_only(seed_head, monkeypatch):
    model = _model().eval()
    x, ei, k = _sampled()
    full = _count_full_heads(model, monkeypatch)
    with torch.no_grad():
        pred = model(x, ei)[:k].argmax(dim=-1)                      # 100M/nb-sample.py:41-43
        assert seed_head.calls == {"head_rows_fwd": [k]} and full == []
        monkeypatch.setenv("SGF_SEED_HEAD", "0")
        assert torch.equal(pred, model(x, ei)[:k].argmax(dim=-1))


def test_every_other_use_of_the_lazy_head_equals_the_existing_path(seed_head, monkeypatch):
    model = _model().eval()
    x, ei, k = _sampled()
    with torch.no_grad():
        monkeypatch.setenv("SGF_SEED_HEAD", "0")
        want = model(x, ei)
        monkeypatch.setenv("SGF_SEED_HEAD", "1")
        idx = torch.tensor([4, 4, 50])
        uses = {
            "sum": (lambda t: t.sum()), "index": (lambda t: t[idx]), "past_the_seeds": (lambda t: t[:k + 1]),
            "float": (lambda t: t.float()), "log_softmax": (lambda t: F.log_softmax(t, 1)),
            "stepped": (lambda t: t[:k:2]), "offset": (lambda t: t[1:k]), "add": (lambda t: t + 1.0),
        }
        for name, use in uses.items():
            seed_head.calls.clear()
            got = use(model(x, ei))
            assert type(got) is torch.Tensor and torch.equal(got, use(want)), name
            assert "head_rows_fwd" not in seed_head.calls and "head_rows_ce" not in seed_head.calls, name
        # rows first, then the whole object: the full logits are still the existing path's
        lazy = model(x, ei)
        rows = lazy[:k]
        assert torch.allclose(rows.float(), want[:k], rtol=1e-5, atol=1e-5)
        assert torch.equal(lazy + 0.0, want)
        assert lazy.shape == want.shape and lazy.dtype == want.dtype and lazy.device == want.device and lazy.dim() == 2
    copy.deepcopy(model)                                            # 100M/nb-sample.py:197 keeps the best model this way
    assert torch.equal(copy.deepcopy(lazy), want)


def test_cross_entropy_hook_third_party_calls(seed_head):
    """Callers that are not the reference's trainer: everything but the trainer's exact call reaches the original — on lazy
    rows with their real values — and plain tensors never notice the hook."""
    model = _model().eval()
    x, ei, k = _sampled()
    orig = F.cross_entropy._sgf_orig
    g = torch.Generator().manual_seed(9)
    y = torch.randint(0, 7, (k,), generator=g)
    with torch.no_grad():
        want_rows = model.forward_rows(x, ei, k)
        cw = torch.rand(7, generator=g)
        prob = torch.softmax(torch.randn(k, 7, generator=g), 1)
        cases = {
            "class_weights": dict(weight=cw), "label_smoothing": dict(label_smoothing=0.1), "sum": dict(reduction="sum"),
            "none": dict(reduction="none"), "ignore_index": dict(ignore_index=int(y[0])), "legacy_reduce": dict(reduce=True),
        }
        for name, kw in cases.items():
            seed_head.calls.clear()
            got = F.cross_entropy(model(x, ei)[:k], y, **kw)
            assert type(got) is torch.Tensor and torch.allclose(got, orig(want_rows, y, **kw), rtol=1e-5, atol=1e-6), name
            assert "head_rows_ce" not in seed_head.calls, name
        seed_head.calls.clear()
        got = F.cross_entropy(model(x, ei)[:k], prob)                   # probability targets
        assert torch.allclose(got, orig(want_rows, prob), rtol=1e-5, atol=1e-6) and "head_rows_ce" not in seed_head.calls
        got = F.cross_entropy(model(x, ei)[:k], y.to(torch.int32).long()[:, None].expand(k, 1)[:, 0])
        assert abs(float(got) - float(orig(want_rows, y))) <= 1e-5         # the trainer's form: served
        assert seed_head.calls.get("head_rows_ce") == [k]
        # lazy rows somebody has read already: their values are there, the original takes them
        seed_head.calls.clear()
        rows = model(x, ei)[:k]
        rows.sum()
        F.cross_entropy(rows, y)
        assert "head_rows_ce" not in seed_head.calls
    # plain tensors (CPU ones here), parameters and 3-D inputs
    seed_head.calls.clear()
    a = torch.randn(6, 7, generator=g, requires_grad=True)
    t = torch.randint(0, 7, (6,), generator=g)
    assert torch.equal(F.cross_entropy(a, t), orig(a, t))
    assert torch.equal(torch.nn.CrossEntropyLoss(weight=cw)(a, t), orig(a, t, weight=cw))
    b3 = torch.randn(2, 7, 5, generator=g)
    t3 = torch.randint(0, 7, (2, 5), generator=g)
    assert torch.equal(F.cross_entropy(b3, t3, ignore_index=1), orig(b3, t3, ignore_index=1))
    assert seed_head.calls == {}


def test_cross_entropy_hook_is_idempotent_and_unpatch_restores():
    from sgformer_amd import launch
    launch.unpatch_ce_loss()
    orig = F.cross_entropy
    try:
        assert launch.patch_ce_loss() is orig
        first = F.cross_entropy
        assert launch.patch_ce_loss() is orig and F.cross_entropy._sgf_orig is orig and F.cross_entropy is not orig
        assert first._sgf_orig is orig
    finally:
        launch.unpatch_ce_loss()
    assert F.cross_entropy is orig
    launch.unpatch_ce_loss()
    assert F.cross_entropy is orig


@pytest.mark.parametrize("mode,patched", [([], True), (["--sgf-patches", "minimal"], False), (["--sgf-aten-loss", "1"], False)],
                         ids=["all", "minimal", "aten_loss"])
def test_launcher_modes_install_or_skip_the_hook(tmp_path, monkeypatch, mode, patched):
    from sgformer_amd import launch
    tdir = tmp_path / "100M"
    tdir.mkdir()
    trainer = tdir / "nb-sample.py"
    trainer.write_text("import json, sys, torch.nn.functional as F\n"
                       "json.dump({'ce': F.cross_entropy.__module__}, open(sys.argv[1], 'w'))\n")
    for name in ("patch_100m_data_utils", "patch_prologue", "patch_neighbor_loader", "patch_nll_loss", "patch_bce_loss",
                 "patch_adam", "patch_eval_metrics"):
        monkeypatch.setattr(launch, name, lambda *a, **kw: None)
    monkeypatch.setitem(sys.modules, "ours", None)
    monkeypatch.setattr(sys, "argv", list(sys.argv))
    monkeypatch.setattr(sys, "path", list(sys.path))
    launch.unpatch_ce_loss()
    orig = F.cross_entropy
    out = tmp_path / "out.json"
    try:
        launch.main(mode + [str(trainer), str(out)])
        seen = json.load(open(out))["ce"]
        assert seen == ("sgformer_amd.launch" if patched else "torch.nn.functional")
        assert (F.cross_entropy is not orig) == patched
    finally:
        launch.unpatch_ce_loss()
    assert F.cross_entropy is orig


def test_sampler_records_the_seed_count_beside_the_hints():
    """The seed count travels as an attribute of the edge list, not as a field of the hint record (whose fields
    tests/test_graph_trace_host.py pins), and SampledBatch.to() carries it to the moved list."""
    import dataclasses
    from sgformer_amd import graph, sampling
    assert "seed" not in " ".join(f.name for f in dataclasses.fields(graph.EdgeHints))
    ei = sampling._seed_rows(graph.EdgeHints(trusted=True).attach(torch.zeros(2, 3, dtype=torch.int64)), 5)
    assert ei._sgf_seed_count == 5 and graph.hints_of(ei).trusted
    batch = sampling.SampledBatch(torch.zeros(4, 2), ei, None, 5, torch.arange(4))
    moved = batch.to("meta")
    assert moved.edge_index is not ei and moved.edge_index._sgf_seed_count == 5


# ------------------------------------------------------------------------------------------------
# the ABI and what the two call sites hand the library
# ------------------------------------------------------------------------------------------------
ENTRIES = ("sgf_head_rows_supported", "sgf_head_rows_fwd_workspace_bytes", "sgf_head_rows_bwd_workspace_bytes",
           "sgf_head_rows_fwd", "sgf_head_rows_bwd")


def test_entries_are_in_the_header_the_binding_and_not_in_the_kernel_table():
    from sgformer_amd import _lib, kernels
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgf.h")).read(), flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "head_rows" not in open(kernels.__file__).read()
    assert not [n for n in vars(kernels.HipKernels) if "head_rows" in n]
    assert os.path.basename("sgformer_amd/csrc/head_rows.hip") in open(os.path.join(ROOT, "Makefile")).read()


def test_supported_query_on_the_host():
    from sgformer_amd import _lib
    if not _lib.available():
        pytest.skip("libsgf.so not built (run `make`)")
    lib = _lib.load()
    q = lib.sgf_head_rows_supported
    assert q(128, 172, _lib.SGF_BF16) == 1 and q(256, 256, _lib.SGF_BF16) == 1 and q(32, 1, _lib.SGF_BF16) == 1
    assert q(48, 7, _lib.SGF_BF16) == 0 and q(48, 7, _lib.SGF_F32) == 1 and q(6, 7, _lib.SGF_F32) == 0
    assert q(288, 7, _lib.SGF_BF16) == 0 and q(128, 257, _lib.SGF_F32) == 0 and q(128, 0, _lib.SGF_F32) == 0
    assert q(128, 47, _lib.SGF_F32_BF16X3) == 0
    assert lib.sgf_head_rows_fwd_workspace_bytes(1000) >= 32 * 12
    assert lib.sgf_head_rows_bwd_workspace_bytes(1000, 128, 172) >= 1000 * 172 * 4 + 8 * 172 * 129 * 4
    # argument errors name the entry and come before any HIP call
    assert lib.sgf_head_rows_fwd(None, 128, 0.5, None, 0, 0.5, None, None, 10, 128, 300, _lib.SGF_BF16, None, 4, None, 300,
                                 None, None, None, None, None, 0, None) == _lib.SGF_E_UNSUPPORTED
    assert b"sgf_head_rows_fwd" in lib.sgf_last_error()
    assert lib.sgf_head_rows_bwd(None, 128, 0.5, None, 0, 0.5, None, 1 << 31, 128, 7, _lib.SGF_BF16, None, 4, None, 7, None, 0,
                                 None, None, None, 1.0, None, 128, None, 0, None, None, None, 0, None) < 0
    assert b"sgf_head_rows_bwd" in lib.sgf_last_error()


def record_calls():
    """{case: {"calls": [[entry, [normalised arguments]], ...], "returns": ...}} for the call sites of head_rows._Hip, in the
    recording style (and with the stand-in library) of tests/test_kernel_table_host.py."""
    from types import SimpleNamespace as NS
    from sgformer_amd import _lib, head_rows, kernels
    from tests.test_kernel_table_host import STREAM, B, L, Recorder, _describe, _flatten, _normalise
    from tests.test_kernel_table_host import F as F32
    hip = head_rows._Hip
    cases = {
        "fwd[bf16_prefix]": lambda: (hip.head_rows_fwd, (B(9, 64), 0.8, B(9, 64), 0.2, F32(7, 64), F32(7), None, 4)),
        "fwd[f32_views_idx_labels]": lambda: (hip.head_rows_fwd, (F32(9, 24)[:, :8], 0.5, F32(9, 24)[:, 8:16], 0.5, F32(5, 8), F32(5),
                                                                  L(3), 3, L(3))),
        "fwd[no_x2_labels]": lambda: (hip.head_rows_fwd, (B(9, 32), 1.0, None, 0.0, F32(7, 32), F32(7), None, 4, L(4))),
        "bwd[generic_prefix]": lambda: (hip.head_rows_bwd, (B(9, 64), 0.8, B(9, 64), 0.2, F32(7, 64), None, 4, F32(4, 7))),
        "bwd[ce_idx_views]": lambda: (hip.head_rows_bwd, (F32(9, 24)[:, :8], 0.5, F32(9, 24)[:, 8:16], 0.5, F32(5, 8), L(3), 3, None,
                                                          F32(3, 5), F32(3), L(3), F32(1), 1.0)),
        "bwd[no_x2]": lambda: (hip.head_rows_bwd, (B(9, 32), 1.0, None, 0.0, F32(7, 32), None, 4, F32(4, 7))),
        "supported[bf16]": lambda: (hip.head_rows_supported, (64, 7, torch.bfloat16)),
        "supported[f16]": lambda: (hip.head_rows_supported, (64, 7, torch.float16)),
    }
    rec, out = Recorder(), {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_lib, "_lib", rec.library(_lib.SIGNATURES))
        mp.setattr(torch.cuda, "current_stream", lambda device=None: NS(cuda_stream=STREAM))
        mp.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
        mp.setattr(torch.cuda, "current_device", lambda: 0)
        try:
            for cid, build in cases.items():
                kernels._workspaces.clear()
                rec.calls, rec.keep, rec.results = [], [], {}
                fn, args = build()
                ins = _flatten(list(args), [])
                ret = fn(*args)
                rets, others = _flatten(ret, []), {}
                out[cid] = {"calls": [[name, [_normalise(r, ins, rets, kernels._workspaces, others) for r in raw]]
                                      for name, raw in rec.calls], "returns": _describe(ret)}
        finally:
            kernels._workspaces.clear()
    return json.loads(json.dumps(out))


def test_call_sites_match_the_golden_file():
    import ctypes
    from sgformer_amd import _lib
    recorded = record_calls()
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert list(recorded) == list(golden), set(recorded) ^ set(golden)
    wrong = [cid for cid in golden if recorded[cid] != golden[cid]]
    assert not wrong, (wrong, json.dumps(recorded[wrong[0]]), json.dumps(golden[wrong[0]]))
    launches = 0
    for cid, entry in recorded.items():
        for name, args in entry["calls"]:
            res, argtypes = _lib.SIGNATURES[name]
            if res is ctypes.c_int32 and argtypes and argtypes[-1] is ctypes.c_void_p and not name.endswith("_supported"):
                assert args[-1] == "stream", (cid, name)          # the stream goes last ...
                launches += 1
            assert "stream" not in args[:-1], (cid, name)         # ... and nowhere else
            assert not [a for a in args if isinstance(a, list) and a[0] == "tmp"], (cid, name)   # no pointer unaccounted for
    assert launches == 6
    fwd = dict(recorded["fwd[f32_views_idx_labels]"]["calls"])["sgf_head_rows_fwd"]
    assert fwd[0] == ["in", 0, 0] and fwd[1] == 24 and fwd[3] == ["in", 1, 0] and fwd[4] == 24      # views keep their stride
    assert fwd[14] == ["ret", 0, 0] and fwd[15] == 5 and fwd[20][:2] == ["ws", "head_rows_fwd"]
    bwd = dict(recorded["bwd[ce_idx_views]"]["calls"])["sgf_head_rows_bwd"]
    assert bwd[13] is None and bwd[21] == ["ret", 0, 0] and bwd[22] == 8 and bwd[23] == ["ret", 1, 0] and bwd[24] == 8
    assert bwd[27][:2] == ["ws", "head_rows_bwd"]
    nox2 = dict(recorded["bwd[no_x2]"]["calls"])["sgf_head_rows_bwd"]
    assert nox2[3] is None and nox2[23] is None and nox2[24] == 0


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_head_rows_host.py --write")
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in record_calls().items()) + "\n}\n")
    print(f"wrote {os.path.relpath(GOLDEN, ROOT)}")
