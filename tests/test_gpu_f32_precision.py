"""The fp32 path under torch.set_float32_matmul_precision('high'): every entry that takes SGF_F32_BF16X3 (csrc/linear_f32x.hip,
csrc/gram_f32x.hip), called through kernels.HipKernels, against fp64 within the split-bf16 bound:

    |C - C64| <= 2^-14 (|A|^T |B|)_ij + 5e-6 max|C64|

(the second term: the fp32 accumulation allowance of the exact-path tests, tests/test_gpu_kernels.py).  For n >= 4097 some
element differs bitwise from the 'highest' result: the split path ran.  Then whole modules on the golden fixtures, no state
leaking between settings, and a captured mini-batch step that is never replayed under another setting."""
import contextlib
import glob
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -14
ACC = 5e-6
NS = [1, 31, 4097, 100003]
WIDTHS = [4, 60, 64, 128, 256, 48]


@contextlib.contextmanager
def precision(p):
    torch.set_float32_matmul_precision(p)
    try:
        yield
    finally:
        torch.set_float32_matmul_precision("highest")


def _check(out, ref, p, what):
    err = (out.double() - ref).abs()
    tol = BOUND * p + ACC * float(ref.abs().max()) + 1e-30
    bad = err > tol
    assert not bool(bad.any()), (what, float(err.max()), int(bad.sum()))


def _strided(t, pad=4):
    """t as a column slice of a wider tensor (leading dimension = width + pad)."""
    big = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=t.dtype, device=t.device)
    big[:, : t.shape[1]] = t
    return big[:, : t.shape[1]]


def _both(fn):
    with precision("highest"):
        exact = fn()
    with precision("high"):
        high = fn()
    return exact, high


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("n", NS)
def test_linear_entries(cuda, n, d):
    from sgformer_amd import ops
    K = ops.K
    g = torch.Generator(device=cuda).manual_seed(n + d)
    d_out = 60 if d == 256 else d               # one non-square shape
    a = _strided(torch.randn(n, d, generator=g, device=cuda))
    w = torch.randn(d_out, d, generator=g, device=cuda) / d ** 0.5
    bias = torch.randn(d_out, generator=g, device=cuda)
    shift = torch.randn(d_out, generator=g, device=cuda) * 0.1
    a64, w64 = a.double(), w.double()
    # y = a W^T + b with the BatchNorm column sums (STATS)
    (y0, _), (y, st) = _both(lambda: K.gcn_epilogue_stats(a, w, bias, shift, want_stats=True))
    _check(y, a64 @ w64.t() + bias.double(), a64.abs() @ w64.abs().t(), "stats")
    v = y.double() - shift.double()
    tol = 2e-6 * torch.cat([v.abs().sum(0), (v * v).sum(0)]).clamp_min(1e-3)
    assert bool(((st.double() - torch.cat([v.sum(0), (v * v).sum(0)])).abs() <= tol).all())
    # dX = dY W
    gy = _strided(torch.randn(n, d_out, generator=g, device=cuda))
    dx0, dx = _both(lambda: K.gcn_epilogue_dx(gy, w))
    _check(dx, gy.double() @ w64, gy.double().abs() @ w64.abs(), "dx")
    # two-operand form [a | a2] W^T + b (sgf_gcn_epilogue_partial + _stats_add)
    a2 = torch.randn(n, d_out, generator=g, device=cuda)
    wc = torch.randn(d_out, d + d_out, generator=g, device=cuda) / (d + d_out) ** 0.5
    (yc0, _), (yc, _) = _both(lambda: K.gcn_epilogue_cat(a, a2, wc, bias, shift, want_stats=True))
    ac = torch.cat([a, a2], 1).double()
    _check(yc, ac @ wc.double().t() + bias.double(), ac.abs() @ wc.double().abs().t(), "cat")
    # the Gram (every dW, G = h^T h) with the column sums of A
    (c0, cs0), (c, cs) = _both(lambda: K.gram(gy, a))
    _check(c, gy.double().t() @ a64, gy.double().abs().t() @ a64.abs(), "gram")
    assert bool(((cs.double() - gy.double().sum(0)).abs() <= ACC * gy.double().abs().sum(0) + 1e-6).all())
    if n >= 4097:
        for hi_, ex_ in ((y, y0), (dx, dx0), (yc, yc0), (c, c0)):
            assert not torch.equal(hi_, ex_)


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("n", NS)
def test_dual_head(cuda, n, d):
    """logits = (a x1 + b x2) W^T + bias and its backward, 47 classes padded to 48 (what ops.combine_fc does)."""
    from sgformer_amd import ops
    K = ops.K
    g = torch.Generator(device=cuda).manual_seed(3 * n + d)
    c = 48
    x1 = _strided(torch.randn(n, d, generator=g, device=cuda))
    x2 = torch.randn(n, d, generator=g, device=cuda)
    w = torch.randn(c, d, generator=g, device=cuda) / d ** 0.5
    w[47] = 0
    bias = torch.randn(c, generator=g, device=cuda)
    bias[47] = 0
    a, b = 0.7, 0.3
    l0, l = _both(lambda: K.combine_fc_fwd(x1, a, x2, b, w, bias))
    xc = a * x1.double() + b * x2.double()
    _check(l, xc @ w.double().t() + bias.double(), (a * x1.double().abs() + b * x2.double().abs()) @ w.double().abs().t(),
           "head fwd")
    gl = torch.randn(n, c, generator=g, device=cuda)
    (d10, d20), (d1, d2) = _both(lambda: K.combine_fc_bwd(gl, w, a, b, torch.float32))
    gw, pw = gl.double() @ w.double(), gl.double().abs() @ w.double().abs()
    _check(d1, a * gw, a * pw, "head bwd dx1")
    _check(d2, b * gw, b * pw, "head bwd dx2")
    if n >= 4097:
        assert not torch.equal(l, l0) and not torch.equal(d1, d10)


def test_non_finite_inputs_propagate(cuda):
    from sgformer_amd import ops
    K = ops.K
    n, d = 5000, 64
    g = torch.Generator(device=cuda).manual_seed(9)
    a = torch.randn(n, d, generator=g, device=cuda)
    a[10, 3], a[20, 5], a[30, 7] = float("inf"), float("-inf"), float("nan")
    w = torch.randn(d, d, generator=g, device=cuda)
    b = torch.randn(n, d, generator=g, device=cuda)
    (y0, _), (y, _) = _both(lambda: K.gcn_epilogue_stats(a, w, None))
    (c0, _), (c, _) = _both(lambda: K.gram(a, b))
    for ex, hi_ in ((y0, y), (c0, c)):
        nf = ~torch.isfinite(ex)
        assert bool(nf.any()) and bool((~torch.isfinite(hi_[nf])).all())
        assert torch.equal(torch.isnan(ex), torch.isnan(ex) & torch.isnan(hi_))


GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))


class _Data:
    def __init__(self, x, ei):
        self.graph = {"node_feat": x, "edge_index": ei, "num_nodes": x.shape[0]}


def _module(meta, z):
    f, d, c, cfg = meta["f"], meta["d"], meta["c"], meta["cfg"]
    if meta["variant"] == "medium":
        from sgformer_amd import ours_medium as M
        gnn = M.GCN(f, d, d, num_layers=meta["gcn_layers"], dropout=0.0, use_bn=True)
        m = M.SGFormer(f, d, c, dropout=0.0, gnn=gnn, **cfg)
    elif meta["variant"] == "100M":
        from sgformer_amd.ours_100m import SGFormer
        m = SGFormer(f, d, c, trans_dropout=0.0, gnn_dropout=0.0, **cfg)
    else:
        from sgformer_amd.ours import SGFormer
        m = SGFormer(f, d, c, trans_dropout=0.0, gnn_dropout=0.0, **cfg)
    sd = m.state_dict()
    params = {k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param/")}
    m.load_state_dict({k: v.to(sd[k].dtype) for k, v in params.items()})
    return m


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_module_under_high_matches_reference_fixture(cuda, path):
    """The fixtures tests/test_gpu_golden.py runs in fp32, under 'high': logits within 2e-4 absolute of the reference's,
    every parameter gradient within 5e-3 relative (Frobenius)."""
    z = np.load(path, allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    medium = meta["variant"] == "medium"
    with precision("high"):
        m = _module(meta, z).to(cuda).train()
        x = torch.from_numpy(z["x"]).float().to(cuda)
        ei = torch.from_numpy(z["edge_index"]).to(cuda)
        y = torch.from_numpy(z["y"]).to(cuda)
        idx = torch.from_numpy(z["train_idx"]).to(cuda)
        logits = m(_Data(x, ei)) if medium else m(x, ei)
        loss = F.nll_loss(torch.log_softmax(logits, dim=1)[idx], y[idx])
        loss.backward()
        torch.cuda.synchronize()
    lerr = float(np.abs(logits.detach().double().cpu().numpy() - z["logits_train"]).max())
    # relative Frobenius error per gradient; a gradient that vanishes in the reference (e.g. the bias of a Linear followed by
    # BatchNorm) is held to the absolute floor tests/test_gpu_golden.py uses, 1e-6 of the largest gradient norm.  5e-3, not
    # 1e-3: dW of the input stem sums dY (columns summing to ~0 behind a BatchNorm) against uncentred features, so |dY|^T |X|
    # exceeds |dY^T X| by ~30x and the per-product bound 2^-14 |dY|^T |X| allows ~2e-3 (products_d256: 2.1e-3 measured)
    gmax = max(float(np.linalg.norm(z[k])) for k in z.files if k.startswith("grad/"))
    worst, n_grad = (-1.0, ""), 0
    for k, prm in m.named_parameters():
        if "grad/" + k not in z.files or prm.grad is None:
            continue
        g_ref = z["grad/" + k]
        num = float(np.linalg.norm(prm.grad.double().cpu().numpy() - g_ref))
        assert num <= 5e-3 * float(np.linalg.norm(g_ref)) + 1e-6 * gmax, (k, num, float(np.linalg.norm(g_ref)))
        worst = max(worst, (num / max(float(np.linalg.norm(g_ref)), 1e-6 * gmax), k))
        n_grad += 1
    print(f"\n{os.path.basename(path)}: 'high' max|logits - ref| = {lerr:.3e}, max rel grad err = {worst[0]:.3e} ({worst[1]})")
    assert lerr <= 2e-4
    assert n_grad >= 10


def _step(m, x, ei, y):
    m.zero_grad(set_to_none=True)
    out = m(x, ei)
    F.nll_loss(F.log_softmax(out, dim=1), y).backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def test_no_state_leaks_between_settings(cuda):
    """'highest' -> 'high' -> 'highest' on one model: both 'highest' steps are bit-identical, the 'high' one is not."""
    from sgformer_amd import synth
    from sgformer_amd.ours import SGFormer
    n, f, c, d = 20000, 64, 40, 256
    ei = synth.synthetic_graph(n, 10.0, seed=3).to(cuda)
    x, y, _ = synth.synthetic_task(n, f, c, seed=3)
    x, y = x.to(cuda), y.to(cuda)
    torch.manual_seed(1)
    m = SGFormer(f, d, c, trans_dropout=0.0, gnn_dropout=0.0, **synth.RECIPES["ogbn-arxiv"]).to(cuda).train()
    with precision("highest"):
        l1, g1 = _step(m, x, ei, y)
    with precision("high"):
        l2, g2 = _step(m, x, ei, y)
    with precision("highest"):
        l3, g3 = _step(m, x, ei, y)
    assert torch.equal(l1, l3) and all(torch.equal(g1[k], g3[k]) for k in g1)
    assert not torch.equal(l1, l2)
    assert float((l1 - l2).abs().max()) <= 1e-2 * float(l1.abs().max())


def test_graphed_step_is_not_replayed_under_another_setting(cuda, monkeypatch):
    """Mini-batch steps of one size: 'highest' for steps 0-2 (eager, capture, replay), then 'high' for steps 3-4.  Step 3
    must be a fresh capture under 'high' (equal, bit for bit, to the all-eager run under the same switch), never the
    replay of the 'highest' graphs."""
    from sgformer_amd import batching, graphed, ops, synth
    from sgformer_amd.ours import SGFormer

    def run(graphs):
        monkeypatch.setenv("SGF_BATCH_GRAPH", "1" if graphs else "0")
        n, f, c, d, mb = 30000, 100, 47, 64, 6144
        ei = synth.synthetic_graph(n, 14.0, seed=11)
        x, y, _ = synth.synthetic_task(n, f, c, seed=11)
        x, y = x.to(cuda), y.to(cuda)
        torch.manual_seed(5)
        model = SGFormer(f, d, c, trans_dropout=0.0, gnn_dropout=0.0, **synth.RECIPES["ogbn-products"]).to(cuda)
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
        gen = torch.Generator().manual_seed(17)
        before = dict(graphed.counters)
        logits = []
        batching._parents.clear()
        try:
            for step in range(5):
                torch.set_float32_matmul_precision("highest" if step < 3 else "high")
                idx = torch.randperm(n, generator=gen)[:mb]
                ei_i, _ = batching.subgraph(idx, ei, num_nodes=n, relabel_nodes=True)
                model.train()
                opt.zero_grad()
                out = model(x[idx.to(cuda)], ei_i)
                logits.append(out.detach().float().clone())
                F.nll_loss(F.log_softmax(out.float(), dim=1), y[idx.to(cuda)]).backward()
                opt.step()
            torch.cuda.synchronize()
        finally:
            torch.set_float32_matmul_precision("highest")
            ops.graph_cache.clear()
        return logits, {k: graphed.counters[k] - before[k] for k in before}

    eager, used_e = run(False)
    graph, used_g = run(True)
    assert used_e == {"captures": 0, "replays": 0}
    assert used_g["captures"] >= 1 and used_g["replays"] >= 1, used_g
    for i, (a, b) in enumerate(zip(eager, graph)):
        assert torch.equal(a, b), f"step {i}: max |diff| {float((a - b).abs().max())}"
