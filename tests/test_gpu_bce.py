"""The multi-label loss on the MI355X: sgf_bce_fwd / sgf_bce_bwd (csrc/bce.hip, include/sgf.h block N4b) against
torch.nn.functional.binary_cross_entropy_with_logits in float64 on the CPU, on the same stored logits; the trainers' loss
lines as written under launch.patch_bce_loss; and the ogbn-proteins recipe's model with this loss, end to end.

Bounds of the kernel checks, from the project's NLL tests (tests/test_gpu_kernels.py::test_fused_loss,
::test_trainer_loss_lines_in_one_pass) — the arithmetic has the same structure (fp32 terms, per-block partials, one sum):
    loss           |d| <= 2e-6 |ref| + 1e-6
    fp32 gradient  max|d| <= 1e-6 max|g_ref|
    bf16 gradient  max|d| <= (2^-8 + 1e-6) max|g_ref|     (2^-8: bf16's unit round-off, for the one rounding of the store)
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import sgformer_oracle as O

pytestmark = pytest.mark.gpu

LOSS_REL, LOSS_ABS = 2e-6, 1e-6
GRAD_F32 = 1e-6
GRAD_BF16 = 2.0 ** -8 + 1e-6


def _logits(n, c, seed, dtype=torch.float32):
    """randn * 3 with a few entries planted at +-60 (l must not overflow, sigmoid must saturate) and at exactly 0."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, generator=g) * 3
    flat = x.view(-1)
    flat[::17] = 60.0
    flat[5::23] = -60.0
    flat[7::29] = 0.0
    return x.to(dtype)


def _target(kind, n, c, seed):
    g = torch.Generator().manual_seed(seed + 1000)
    if kind == "f32":
        t = torch.rand(n, c, generator=g)                      # soft targets
        t.view(-1)[::3] = 1.0
        t.view(-1)[1::3] = 0.0
        return t
    if kind == "i64":
        return torch.randint(0, 2, (n, c), generator=g)
    t = torch.randint(0, c, (n,), generator=g)                 # class indices ...
    if n >= 8:
        t[1], t[4], t[6] = -1, c, 2 ** 40                      # ... some of them outside [0, c): all-zero rows
    return t


def _dense_target(target, n, c):
    if target.dim() == 2:
        return target.double()
    return (target[:, None] == torch.arange(c)[None, :]).double()


def _reference(logits, target, rows):
    """float64 torch on the CPU: (sum-normalised) mean loss over rows x C and its [n, c] gradient."""
    n, c = logits.shape
    x = logits.detach().double().requires_grad_(True)
    if rows.numel() == 0:
        return torch.zeros((), dtype=torch.float64), torch.zeros(n, c, dtype=torch.float64)
    loss = F.binary_cross_entropy_with_logits(x[rows], _dense_target(target, n, c)[rows])
    loss.backward()
    return loss.detach(), x.grad


def _check(what, loss, grad, lref, gref, bf16):
    lerr = abs(float(loss) - float(lref))
    gerr = float((grad.double().cpu() - gref).abs().max())
    gmax = float(gref.abs().max())
    print(f"{what}: loss {float(loss):.9g} ref {float(lref):.9g} |d|={lerr:.3e} (bound {LOSS_REL * abs(float(lref)) + LOSS_ABS:.3e}); "
          f"grad max|d|={gerr:.3e} = {gerr / max(gmax, 1e-300):.3e} of max|g_ref|={gmax:.3e}")
    assert lerr <= LOSS_REL * abs(float(lref)) + LOSS_ABS
    assert gerr <= (GRAD_BF16 if bf16 else GRAD_F32) * gmax


SHAPES = [(300, 1, 120), (5000, 2, 3100), (4000, 7, 1500), (3000, 47, 2000), (3000, 64, 1100), (30000, 112, 10000),
          (2500, 172, 900), (700, 300, 333), (600, 112, 0)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["f32", "i64", "class"])
@pytest.mark.parametrize("n,c,m", SHAPES)
def test_kernel_parity(cuda, n, c, m, kind, dtype):
    """Row form, through the kernel table, for every storage dtype x target kind x shape; rows outside idx: exact zeros."""
    from sgformer_amd import ops
    if kind == "class" and c == 1:
        kind = "i64"                              # (class indices need C > 1: a one-column head holds 0 / 1 labels)
    logits = _logits(n, c, n + c, dtype)
    target = _target(kind, n, c, n + c)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(m + 1))[:m]
    lg, tg, ix = logits.to(cuda), target.to(cuda), idx.to(cuda)
    inv = 1.0 / (max(m, 1) * c)
    loss = ops.K.bce_fwd(lg, tg, ix) * inv
    gout = torch.ones(1, device=cuda)
    grad = ops.K.bce_bwd(lg, tg, ix, gout, inv)
    torch.cuda.synchronize()
    assert grad.dtype == dtype and grad.shape == (n, c) and loss.dtype == torch.float32
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())
    lref, gref = _reference(logits, target, idx)
    _check(f"n={n} c={c} m={m} {kind}", loss, grad, lref, gref, dtype == torch.bfloat16)
    off = torch.ones(n, dtype=torch.bool)
    off[idx] = False
    assert int(torch.count_nonzero(grad.cpu()[off])) == 0
    if m == 0:
        assert float(loss) == 0.0 and int(torch.count_nonzero(grad)) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["f32", "i64", "class"])
@pytest.mark.parametrize("n,c", [(4000, 2), (3000, 7), (2000, 112), (1500, 47)])
def test_dense_form_equals_row_form_bit_for_bit_and_is_deterministic(cuda, n, c, kind, dtype):
    from sgformer_amd import ops
    logits = _logits(n, c, 5 * n + c, dtype).to(cuda)
    target = _target(kind, n, c, 5 * n + c).to(cuda)
    rows = torch.arange(n, device=cuda)
    gout = torch.full((1,), 0.75, device=cuda)
    inv = 1.0 / (n * c)
    dense = ops.K.bce_fwd(logits, target, None), ops.K.bce_bwd(logits, target, None, gout, inv)
    row = ops.K.bce_fwd(logits, target, rows), ops.K.bce_bwd(logits, target, rows, gout, inv)
    again = ops.K.bce_fwd(logits, target, rows), ops.K.bce_bwd(logits, target, rows, gout, inv)
    torch.cuda.synchronize()
    assert torch.equal(dense[0], row[0]) and torch.equal(dense[1].view(torch.uint8), row[1].view(torch.uint8))
    assert torch.equal(again[0], row[0]) and torch.equal(again[1].view(torch.uint8), row[1].view(torch.uint8))
    lref, gref = _reference(logits.cpu(), target.cpu(), torch.arange(n))
    _check(f"dense n={n} c={c} {kind}", dense[0] * inv, dense[1].double() / 0.75, lref, gref, dtype == torch.bfloat16)


def test_determinism_of_a_gathered_launch(cuda):
    from sgformer_amd import ops
    n, c, m = 30000, 112, 19000
    logits = _logits(n, c, 77).to(cuda)
    target = _target("i64", n, c, 77).to(cuda)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(9))[:m].to(cuda)
    gout = torch.ones(1, device=cuda)
    a = ops.K.bce_fwd(logits, target, idx).clone(), ops.K.bce_bwd(logits, target, idx, gout, 1.0 / (m * c))
    b = ops.K.bce_fwd(logits, target, idx).clone(), ops.K.bce_bwd(logits, target, idx, gout, 1.0 / (m * c))
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_strided_and_unaligned_operands(cuda):
    """Logits with a leading dimension (a column slice of a wider matrix, rows not 16-byte aligned): the one-element path."""
    from sgformer_amd import ops
    n, c, m = 1200, 112, 500
    wide = torch.zeros(n, c + 3)
    wide[:, 1:c + 1] = _logits(n, c, 13)
    logits = wide.to(cuda)[:, 1:c + 1]
    assert logits.stride() == (c + 3, 1)
    target = _target("f32", n, c, 13)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(4))[:m]
    loss = ops.bce_loss_rows(logits.requires_grad_(True), target.to(cuda), idx.to(cuda))
    grad, = torch.autograd.grad(loss, logits)
    lref, gref = _reference(wide[:, 1:c + 1], target, idx)
    _check("strided", loss.detach(), grad, lref, gref, False)


@pytest.fixture
def patched(cuda):
    from sgformer_amd import launch
    launch.unpatch_bce_loss()                    # (whatever an earlier test left behind)
    bce0 = F.binary_cross_entropy_with_logits
    launch.patch_bce_loss(min_elements=0)        # every size: the cases below drive the one-pass form with small inputs
    try:
        yield bce0
    finally:
        launch.unpatch_bce_loss()
    assert F.binary_cross_entropy_with_logits is bce0


@pytest.mark.parametrize("route", ["proteins", "one_hot"])
def test_trainer_loss_lines_as_written(cuda, patched, monkeypatch, route):
    """large/main.py:130-137 unchanged, under patch_bce_loss: the criterion's element-wise part runs once through sgf_bce_fwd
    (dense form) and gives what the same lines give un-patched, and what loss.bce_with_logits_rows gives on the same inputs."""
    from sgformer_amd import loss as L
    from sgformer_amd import ops
    if route == "proteins":
        n, c = 6000, 112
        label = _target("i64", n, c, 3).to(cuda)                          # dataset.label: int64 [N, 112]
        true_label = label                                                # large/main.py:135
        rows_target = label
    else:
        n, c = 9000, 2
        label = torch.randint(0, c, (n, 1), generator=torch.Generator().manual_seed(4)).to(cuda)     # int64 [N, 1]
        label[0, 0], label[1, 0] = 0, c - 1
        true_label = F.one_hot(label, label.max() + 1).squeeze(1)         # large/main.py:133
        rows_target = label                                               # the class indices themselves
    out0 = _logits(n, c, 21)
    train_idx = torch.randperm(n, generator=torch.Generator().manual_seed(6))[: int(0.65 * n)].to(cuda)
    calls = []
    real = ops.K.bce_fwd
    monkeypatch.setattr(ops.K, "bce_fwd", staticmethod(lambda *a: (calls.append(1), real(*a))[1]))

    out = out0.to(cuda).requires_grad_(True)
    criterion = nn.BCEWithLogitsLoss()
    loss = criterion(out[train_idx], true_label.squeeze(1)[train_idx].to(torch.float))
    loss.backward()
    assert len(calls) == 1

    ref_out = out0.to(cuda).requires_grad_(True)                          # the same lines, un-patched, in fp32
    ref = patched(ref_out[train_idx], true_label.squeeze(1)[train_idx].to(torch.float))
    ref.backward()
    assert len(calls) == 1
    lerr = abs(float(loss.detach()) - float(ref.detach()))
    gerr = float((out.grad - ref_out.grad).abs().max())
    gmax = float(ref_out.grad.abs().max())
    print(f"{route}: patched {float(loss):.9g} ATen {float(ref):.9g} |d|={lerr:.3e}; grad {gerr / gmax:.3e} of max")
    assert lerr <= LOSS_REL * abs(float(ref)) + LOSS_ABS
    assert gerr <= GRAD_F32 * gmax

    rows_out = out0.to(cuda).requires_grad_(True)
    fused = L.bce_with_logits_rows(rows_out, rows_target, train_idx)
    fused.backward()
    assert len(calls) == 2
    assert abs(float(fused.detach()) - float(loss.detach())) <= LOSS_REL * abs(float(loss.detach())) + LOSS_ABS
    assert float((rows_out.grad - ref_out.grad).abs().max()) <= GRAD_F32 * gmax
    # ... and both against float64
    lref, gref = _reference(out0, label.cpu() if route == "proteins" else label.view(-1).cpu(), train_idx.cpu())
    _check(f"{route} lines", loss.detach(), out.grad, lref, gref, False)
    _check(f"{route} rows", fused.detach(), rows_out.grad, lref, gref, False)


def test_default_patch_by_size(cuda, monkeypatch):
    """patch_bce_loss() as the launcher installs it: the trainers' lines at the ogbn-proteins full-graph size (132 534 x 112,
    65 % training rows = 9.6 M elements >= launch.BCE_PATCH_MIN_ELEMENTS) run sgf_bce_fwd once and meet the bounds; at the
    mini-batch size (10 000 x 112) the call stays on ATen and gives its very bits."""
    from sgformer_amd import launch, ops
    launch.unpatch_bce_loss()
    bce0 = F.binary_cross_entropy_with_logits
    calls = []
    real = ops.K.bce_fwd
    monkeypatch.setattr(ops.K, "bce_fwd", staticmethod(lambda *a: (calls.append(1), real(*a))[1]))
    launch.patch_bce_loss()
    try:
        for n, taken in ((10000, False), (132534, True)):
            c = 112
            label = _target("i64", n, c, 8).to(cuda)
            out0 = _logits(n, c, 9)
            train_idx = torch.randperm(n, generator=torch.Generator().manual_seed(2))[: int(0.65 * n)].to(cuda)
            assert (train_idx.numel() * c >= launch.BCE_PATCH_MIN_ELEMENTS) == taken
            out = out0.to(cuda).requires_grad_(True)
            before = len(calls)
            loss = nn.BCEWithLogitsLoss()(out[train_idx], label.squeeze(1)[train_idx].to(torch.float))
            loss.backward()
            assert len(calls) == before + int(taken)
            ref_out = out0.to(cuda).requires_grad_(True)
            ref = bce0(ref_out[train_idx], label.squeeze(1)[train_idx].to(torch.float))
            ref.backward()
            if taken:
                lref, gref = _reference(out0, label.cpu(), train_idx.cpu())
                _check(f"default patch n={n}", loss.detach(), out.grad, lref, gref, False)
            else:
                assert torch.equal(loss.detach(), ref.detach()) and torch.equal(out.grad, ref_out.grad)
    finally:
        launch.unpatch_bce_loss()
    assert F.binary_cross_entropy_with_logits is bce0


# large/run.sh:8-12 (ogbn-proteins recipe; its dropout is 0): 2 GCN layers with use_weight and without use_init, 1 attention
# layer, graph_weight 0.5
PROTEINS = dict(trans_num_layers=1, trans_num_heads=1, trans_use_bn=True, trans_use_residual=True, trans_use_weight=True,
                trans_use_act=False, gnn_num_layers=2, gnn_use_bn=True, gnn_use_residual=True, gnn_use_weight=True,
                gnn_use_init=False, gnn_use_act=True, graph_weight=0.5, aggregate="add")


def _proteins_problem():
    n, f, d, c = 4000, 8, 64, 112
    torch.manual_seed(11)
    x = torch.randn(n, f)
    ei = O.synthetic_graph(n, 8.0, seed=3)
    target = torch.randint(0, 2, (n, c))
    idx = torch.arange(0, n, 2)
    return n, f, d, c, x, ei, target, idx


def _proteins_model(cuda, f, d, c, compute_dtype=None):
    from sgformer_amd.ours import SGFormer
    p = O.init_params(PROTEINS, f, d, c, seed=0)
    m = SGFormer(f, d, c, trans_dropout=0.0, gnn_dropout=0.0, **PROTEINS)
    m.load_state_dict({**m.state_dict(), **p})
    m = m.to(cuda).train()
    if compute_dtype is not None:
        m.compute_dtype = compute_dtype
    return m, p


def test_proteins_recipe_end_to_end_fp32(cuda):
    """Forward through sgformer_amd.ours.SGFormer, loss.bce_with_logits_rows, backward — against the float64 oracle followed by
    torch's BCE in float64, at the bounds of the fp32 model-parity tests and smoke(): 1e-4 absolute on the logits, 5e-4
    relative Frobenius on every parameter gradient."""
    from sgformer_amd import loss as L
    n, f, d, c, x, ei, target, idx = _proteins_problem()
    m, p = _proteins_model(cuda, f, d, c)
    logits = m(x.to(cuda), ei.to(cuda))
    assert logits.shape == (n, c)
    loss = L.bce_with_logits_rows(logits, target.to(cuda), idx.to(cuda))
    loss.backward()
    torch.cuda.synchronize()
    p64 = {k: v.double().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in p.items()}
    ref = O.sgformer_forward(p64, x.double(), ei, PROTEINS, training=True)
    lref = F.binary_cross_entropy_with_logits(ref[idx], target.double()[idx])
    lref.backward()
    err = float((logits.detach().double().cpu() - ref.detach()).abs().max())
    gerr = max(float((prm.grad.double().cpu() - p64[k].grad).norm() / p64[k].grad.norm())
               for k, prm in m.named_parameters() if p64[k].grad is not None and float(p64[k].grad.norm()) > 1e-10)
    print(f"proteins fp32: loss {float(loss):.7f} oracle {float(lref):.7f} max|logits-oracle|={err:.2e} max rel grad err={gerr:.2e}")
    assert err <= 1e-4 and gerr <= 5e-4
    assert abs(float(loss) - float(lref)) <= 1e-4 * abs(float(lref))


def test_proteins_recipe_end_to_end_bf16(cuda):
    """The same step in bf16 activation storage (compute_dtype=torch.bfloat16), bounded the way
    tests/test_gpu_model.py::test_bf16_activation_mode bounds bf16 — its constants, not new ones: 3e-2 relative on logits and
    loss, 0.12 relative on the three large, well-conditioned gradients — here against the fp32 run of the same model (which
    the test above ties to the oracle).  Every gradient is finite and fp32.  Measured on an MI355X: logits 6.1e-3, loss
    3.2e-6, gradients 2.6e-3 (fc.weight), 4.4e-2 (graph_conv.convs.1.W.weight), 4.0e-2 (graph_conv.fcs.0.weight) — the
    existing constants transfer to the 112-column head with room."""
    from sgformer_amd import loss as L
    n, f, d, c, x, ei, target, idx = _proteins_problem()
    runs = {}
    for name, cd in (("f32", None), ("bf16", torch.bfloat16)):
        m, _ = _proteins_model(cuda, f, d, c, cd)
        logits = m(x.to(cuda), ei.to(cuda))
        loss = L.bce_with_logits_rows(logits, target.to(cuda), idx.to(cuda))
        loss.backward()
        torch.cuda.synchronize()
        runs[name] = (logits.detach().double().cpu(), float(loss), {k: v.grad for k, v in m.named_parameters()})
    (lg32, l32, g32), (lg16, l16, g16) = runs["f32"], runs["bf16"]
    rel = float((lg16 - lg32).norm() / lg32.norm())
    print(f"proteins bf16 vs fp32: logits rel {rel:.3e}, loss {l16:.7f} vs {l32:.7f} ({abs(l16 - l32) / abs(l32):.3e})")
    assert rel <= 3e-2
    assert abs(l16 - l32) <= 3e-2 * abs(l32)
    for k, g in g16.items():
        assert g is not None and g.dtype == torch.float32 and bool(torch.isfinite(g).all()), k
    for k in ["fc.weight", "graph_conv.convs.1.W.weight", "graph_conv.fcs.0.weight"]:
        e = float((g16[k].double() - g32[k].double()).norm() / g32[k].double().norm())
        print(f"  {k}: rel grad err {e:.3e}")
        assert e <= 0.12, k
