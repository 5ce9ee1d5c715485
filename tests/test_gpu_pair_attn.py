"""All-pair sigmoid attention on the GPU (csrc/pair_attn.hip through sgformer_amd/pair_attn.py).

The reference arithmetic is the project's own difformer._dense_attention, run in fp64 on the CPU on the operands as rounded to
the storage dtype.  The random operands are generated bf16-representable, so both storage dtypes see the same values and one
reference per shape serves both.

Bars.  Forward, elementwise: fp32 |out - ref| <= 1e-4 max|v| (the fp32 logits bar of test_difformer_parity); bf16 <= 2^-7
max|v|: rounding S to bf16 moves the weights of the convex combination by at most 2^-8 relative about their mean, and the
output rounding adds 2^-8 |out|, together 2^-7 max|v|.  Backward, per gradient: ||err|| <= tol (||ref|| + 1e-2 gmax)
with tol = 1e-3 (fp32) / 8e-2 (bf16), the gradient bars of test_difformer_parity.  rowsum: 1e-5 relative in fp32; 2^-9
relative in bf16 (the kernel sums S in fp32 before the operand is rounded).  Each check prints `PAIR_RATIO <name> <error / bar>` before it asserts
(pytest -s shows them; profiles/pair_attn_probe.md records the worst)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
SHAPES = [(1, 1), (31, 33), (33, 31), (70, 193), (257, 255), (1031, 1031)]
ULP = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7}        # spacing of the storage type relative to a power of two
FWD_BAR = {torch.float32: 1e-4, torch.bfloat16: 2.0 ** -7}
GRAD_TOL = {torch.float32: 1e-3, torch.bfloat16: 8e-2}
RS_BAR = {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -9}


def _ratio(name, err, bar):
    r = float(err) / float(bar) if bar > 0 else (0.0 if err == 0 else float("inf"))
    print(f"PAIR_RATIO {name} {r:.4f}")
    return r


def _lap_shapes(d, dtype):
    """(n, l) at which a workgroup of one of the kernels walks three tiles (none while every workgroup owns one tile)."""
    from sgformer_amd import _lib
    code = _lib.SGF_BF16 if dtype == torch.bfloat16 else _lib.SGF_F32
    rows = [int(_lib.load().sgf_pair_sigmoid_lap_rows(w, 3, d, code, 3)) for w in (0, 1, 2)]
    return [(r, 65) if w < 2 else (65, r) for w, r in enumerate(rows) if r > 0]


def _entries(q, k, v, g):
    """(out, rowsum, dq, dk, dv) of the three launches on tensors that are already on the GPU"""
    from sgformer_amd.pair_attn import _Hip
    out, rowsum = _Hip.pair_sigmoid_fwd(q, k, v)
    dq, delta = _Hip.pair_sigmoid_bwd_q(g, out, rowsum, q, k, v)
    dk, dv = _Hip.pair_sigmoid_bwd_kv(g, rowsum, delta, q, k, v)
    return out, rowsum, dq, dk, dv


# ------------------------------------------------------------------------------------------------
# 1. exact masks: layout, tails, saturation
# ------------------------------------------------------------------------------------------------
_exact = {}


def _exact_case(n, l, h, hv, d):
    """q_i = 4 e_c(i) with c(i) = (5 i + 1) mod D, k_j[m] = 8 if B[j][m] else -32 with the asymmetric table
    B[j][m] = (7 j + 3 m + (j >> 3)) mod 5 < 2: z is 32 or -128, S exactly 1 or 0.  Head t shifts c by 7 t and j by 3 t, so
    that heads cannot be mixed up unnoticed.  A query row the table leaves without any key (0 / 0; it happens at (1, 1)
    only) gets key i mod l switched on: every row's count is >= 1, which is asserted."""
    key = (n, l, h, hv, d)
    if key not in _exact:
        gen = torch.Generator().manual_seed(n * 131 + l * 7 + h * 3 + hv + d)
        i, j, m = torch.arange(n), torch.arange(l), torch.arange(d)
        q = torch.zeros(n, h, d, dtype=torch.float64)
        k = torch.empty(l, h, d, dtype=torch.float64)
        mask = torch.empty(h, n, l, dtype=torch.float64)
        for t in range(h):
            c = (5 * i + 1 + 7 * t) % d
            q[i, t, c] = 4.0
            b = ((7 * (j[:, None] + 3 * t) + 3 * m[None, :] + ((j[:, None] + 3 * t) >> 3)) % 5) < 2        # asymmetric table
            empty = (b[:, c].sum(0) == 0).nonzero().view(-1)             # (only (1, 1): the table drops its one key)
            b[empty % l, c[empty]] = True                                # such a row keeps key i mod l
            k[:, t, :] = torch.where(b, 8.0, -32.0)
            mask[t] = b[:, c].t().double()
        v = torch.randint(-3, 4, (l, hv, d), generator=gen).double()
        g = torch.randint(-2, 3, (n, h, d), generator=gen).double()
        count = mask.sum(2)                                            # [h, n]
        assert float(count.min()) >= 1, "a condition on the inputs: every row keeps at least one key"
        ve = v.expand(-1, h, -1)
        out = torch.stack([mask[t] @ ve[:, t] / count[t][:, None] for t in range(h)], 1)
        dv = torch.stack([(mask[t] / count[t][:, None]).t() @ g[:, t] for t in range(h)], 1)
        if hv == 1:
            dv = dv.sum(1, keepdim=True)
        _exact[key] = (q, k, v, g, count.t().contiguous(), out, dv)
    return _exact[key]


def _check_exact(cuda, dtype, n, l, h, hv, d, wide=False):
    q, k, v, g, count, out_ref, dv_ref = _exact_case(n, l, h, hv, d)

    def dev(t):
        t = t.to(cuda, dtype)
        if not wide:
            return t
        buf = torch.full((t.shape[0], t.shape[1] * t.shape[2] + 24), 77.0, device=cuda, dtype=dtype)       # ld > H * D
        view = buf[:, 8:8 + t.shape[1] * t.shape[2]].view(t.shape[0], t.shape[1], t.shape[2])
        view.copy_(t)
        return view
    out, rowsum, dq, dk, dv = _entries(dev(q), dev(k), dev(v), dev(g))
    tag = f"exact[{str(dtype)[6:]},{n}x{l},H{h},Hv{hv},D{d}{',wide' if wide else ''}]"
    assert torch.equal(rowsum.double().cpu(), count), tag
    err = (out.double().cpu() - out_ref).abs()
    ulp = ULP[dtype] * torch.exp2(torch.floor(torch.log2(out_ref.abs().clamp_min(1e-30))))
    assert bool((err <= ulp).all()), (tag, float((err / ulp).max()))
    assert not bool(dq.double().abs().max() > 0) and not bool(dk.double().abs().max() > 0), tag
    bar = GRAD_TOL[dtype] * (1.0 + 1e-2) * float(dv_ref.norm())
    assert _ratio(tag + ".dv", (dv.double().cpu() - dv_ref).norm(), bar) <= 1.0, tag


@pytest.mark.parametrize("h,hv", [(1, 1), (3, 1), (3, 3)])
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_masks(cuda, dtype, d, h, hv):
    for n, l in SHAPES + _lap_shapes(d, dtype):
        _check_exact(cuda, dtype, n, l, h, hv, d)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_masks_in_wider_buffers(cuda, dtype):
    _check_exact(cuda, dtype, 70, 193, 3, 3, 64, wide=True)
    _check_exact(cuda, dtype, 257, 255, 3, 1, 32, wide=True)


# ------------------------------------------------------------------------------------------------
# 2. random parity
# ------------------------------------------------------------------------------------------------
_random = {}


def _random_case(n, l, h, hv, d, zmax=None):
    """bf16-representable operands and the fp64 reference (out, rowsum, dq, dk, dv), made once per shape"""
    from sgformer_amd.difformer import _dense_attention
    key = (n, l, h, hv, d, zmax)
    if key not in _random:
        gen = torch.Generator().manual_seed(1 + n + 3 * l + 5 * h + 7 * hv + 11 * d)

        def rnd(*shape, scale=1.0):
            return (scale * torch.randn(*shape, generator=gen)).bfloat16().double()
        q, k = rnd(n, h, d, scale=2.0 / d ** 0.5), rnd(l, h, d, scale=2.0 / d ** 0.5)
        if zmax is not None:
            z = torch.einsum("nhd,lhd->nlh", q, k).abs().max()
            q = (q * (zmax / z)).bfloat16().double()
        v, g = rnd(l, hv, d), rnd(n, h, d)
        ops = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out, _ = _dense_attention(ops[0], ops[1], ops[2].expand(-1, h, -1) if hv == 1 else ops[2], 'sigmoid', False)
        out.backward(g)
        rowsum = torch.sigmoid(torch.einsum("nhd,lhd->nlh", q, k)).sum(1)
        _random[key] = (q, k, v, g, out.detach(), rowsum, ops[0].grad, ops[1].grad, ops[2].grad)
    return _random[key]


def _check_random(cuda, dtype, n, l, h, hv, d, zmax=None):
    q, k, v, g, out_ref, rs_ref, dq_ref, dk_ref, dv_ref = _random_case(n, l, h, hv, d, zmax)
    out, rowsum, dq, dk, dv = _entries(*(t.to(cuda, dtype) for t in (q, k, v, g)))
    tag = f"random[{str(dtype)[6:]},{n}x{l},H{h},Hv{hv},D{d}{',z' + str(zmax) if zmax else ''}]"
    worst = _ratio(tag + ".out", (out.double().cpu() - out_ref).abs().max(), FWD_BAR[dtype] * float(v.abs().max()))
    worst = max(worst, _ratio(tag + ".rowsum", ((rowsum.double().cpu() - rs_ref).abs() / rs_ref).max(), RS_BAR[dtype]))
    gmax = max(float(t.norm()) for t in (dq_ref, dk_ref, dv_ref))
    for name, got, ref in (("dq", dq, dq_ref), ("dk", dk, dk_ref), ("dv", dv, dv_ref)):
        bar = GRAD_TOL[dtype] * (float(ref.norm()) + 1e-2 * gmax)
        worst = max(worst, _ratio(f"{tag}.{name}", (got.double().cpu() - ref).norm(), bar))
    for t in (out, rowsum, dq, dk, dv):
        assert bool(torch.isfinite(t).all()), tag
    assert worst <= 1.0, tag


@pytest.mark.parametrize("h,hv,d", [(1, 1, 64), (2, 2, 32), (3, 1, 128), (3, 3, 64), (2, 1, 64)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_random_parity(cuda, dtype, h, hv, d):
    for n, l in SHAPES + _lap_shapes(d, dtype):
        _check_random(cuda, dtype, n, l, h, hv, d)


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_parity_large_scores(cuda, dtype):
    _check_random(cuda, dtype, 257, 255, 2, 2, 64, zmax=30.0)


# ------------------------------------------------------------------------------------------------
# 3. reproducibility
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_bit_reproducible(cuda, dtype):
    q, k, v, g = (t.to(cuda, dtype) for t in _random_case(1031, 1031, 3, 3, 64)[:4])
    a = _entries(q, k, v, g)
    b = _entries(q, k, v, g)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------
# 4. the module and the free function, kernels against the dense path
# ------------------------------------------------------------------------------------------------
class _Data:
    def __init__(self, x, ei):
        self.graph = {"node_feat": x, "edge_index": ei}


def _module_run(cuda, dtype, x, ei, y, state):
    from sgformer_amd import difformer as M
    m = M.DIFFormer(x.shape[1], 64, 7, num_layers=2, num_heads=2, kernel='sigmoid', dropout=0.0)
    m.load_state_dict(state)
    m = m.to(cuda).train()
    logits = m(_Data(x.to(cuda, dtype), ei.to(cuda)))
    torch.nn.functional.cross_entropy(logits.float(), y.to(cuda)).backward()
    return logits.detach().double().cpu(), {k: p.grad.double().cpu() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("dtype", DTYPES)
def test_module_matches_the_dense_path(cuda, dtype, monkeypatch):
    from sgformer_amd import difformer as M, pair_attn
    n, f = 3000, 40
    torch.manual_seed(5)
    state = M.DIFFormer(f, 64, 7, num_layers=2, num_heads=2, kernel='sigmoid').state_dict()
    x = torch.randn(n, f)
    src = torch.randint(0, n, (8 * n,))
    dst = (src + 1 + torch.randint(0, n - 1, (8 * n,))) % n
    ei = torch.stack([torch.cat([src, dst]), torch.cat([dst, src])])
    y = torch.randint(0, 7, (n,))
    monkeypatch.setenv("SGF_PAIR_ATTN", "0")
    ref, ref_g = _module_run(cuda, dtype, x, ei, y, state)
    monkeypatch.setenv("SGF_PAIR_ATTN", "1")
    calls = []
    fwd = pair_attn._Hip.pair_sigmoid_fwd
    monkeypatch.setattr(pair_attn._Hip, "pair_sigmoid_fwd", staticmethod(lambda *a: (calls.append(1), fwd(*a))[1]))
    got, got_g = _module_run(cuda, dtype, x, ei, y, state)
    assert len(calls) == 2                                        # both layers took the kernels
    if dtype == torch.float32:
        assert _ratio(f"module[{str(dtype)[6:]}].logits", (got - ref).abs().max(), 1e-4) <= 1.0
    else:
        assert _ratio(f"module[{str(dtype)[6:]}].logits", (got - ref).norm() / ref.norm(), 3e-2) <= 1.0
    gmax = max(float(g.norm()) for g in ref_g.values())
    assert set(got_g) == set(ref_g)
    for k, g in ref_g.items():
        bar = GRAD_TOL[dtype] * (float(g.norm()) + 1e-2 * gmax)
        assert _ratio(f"module[{str(dtype)[6:]}].{k}", (got_g[k] - g).norm(), bar) <= 1.0, k


@pytest.mark.parametrize("dtype", DTYPES)
def test_free_function_matches_the_dense_path(cuda, dtype, monkeypatch):
    from sgformer_amd import difformer as M
    q0, k0, v0, g0 = (t.to(cuda, dtype) for t in _random_case(257, 193, 2, 2, 64)[:4])
    res = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("SGF_PAIR_ATTN", switch)
        ops = [t.clone().requires_grad_(True) for t in (q0, k0, v0)]
        out = M.full_attention_conv(ops[0], ops[1], ops[2], 'sigmoid')
        out.backward(g0)
        res[switch] = [out.detach().double().cpu()] + [t.grad.double().cpu() for t in ops]
    assert type(out.grad_fn).__name__.startswith("_SigmoidAttention")
    ref, got = res["0"], res["1"]
    if dtype == torch.float32:
        assert float((got[0] - ref[0]).abs().max()) <= 1e-4
    else:
        assert float((got[0] - ref[0]).norm() / ref[0].norm()) <= 3e-2
    gmax = max(float(t.norm()) for t in ref[1:])
    for a, b in zip(got[1:], ref[1:]):
        assert float((a - b).norm()) <= GRAD_TOL[dtype] * (float(b.norm()) + 1e-2 * gmax)


# ------------------------------------------------------------------------------------------------
# 5. a size the dense path cannot reach
# ------------------------------------------------------------------------------------------------
def test_forty_thousand_nodes_without_a_score_tensor(cuda):
    """n = l = 40 009, H = 2, D = 64, bf16: one dense score tensor would be 12.8 GB; the kernels' peak stays within 256 MB of
    the operands.  out and dq on 64 fixed query rows against the fp64 formula over all keys."""
    from sgformer_amd import pair_attn
    n, h, d, dtype = 40009, 2, 64, torch.bfloat16
    gen = torch.Generator().manual_seed(40009)
    q, k = (((2.0 / d ** 0.5) * torch.randn(n, h, d, generator=gen)).bfloat16() for _ in range(2))
    v, g = (torch.randn(n, h, d, generator=gen).bfloat16() for _ in range(2))
    ops = [t.to(cuda).requires_grad_(True) for t in (q, k, v)]
    gd = g.to(cuda)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = pair_attn.sigmoid_attention(*ops)
    out.backward(gd)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"PAIR_MEMORY rise_mb {rise / 2 ** 20:.1f}")
    assert rise < 256 * 2 ** 20
    for t in (out, ops[0].grad, ops[1].grad, ops[2].grad):
        assert bool(torch.isfinite(t).all())
    rows = (torch.arange(64) * 631 + 17) % n
    qr, gr = q[rows].double(), g[rows].double()
    s = torch.sigmoid(torch.einsum("nhd,lhd->nlh", qr, k.double()))
    r = s.sum(1)
    out_ref = torch.einsum("nlh,lhd->nhd", s, v.double()) / r[:, :, None]
    p = torch.einsum("nhd,lhd->nlh", gr, v.double())
    delta = (gr * out_ref).sum(2)
    dz = s * (1 - s) * (p - delta[:, None, :]) / r[:, None, :]
    dq_ref = torch.einsum("nlh,lhd->nhd", dz, k.double())
    rows = rows.to(cuda)
    worst = _ratio("big[bfloat16].out", (out.detach()[rows].double().cpu() - out_ref).abs().max(), FWD_BAR[dtype] * float(v.abs().max()))
    bar = GRAD_TOL[dtype] * (1.0 + 1e-2) * float(dq_ref.norm())
    worst = max(worst, _ratio("big[bfloat16].dq", (ops[0].grad[rows].double().cpu() - dq_ref).norm(), bar))
    assert worst <= 1.0
