"""All-pair softmax attention on the GPU (csrc/pair_attn.hip block N8 through sgformer_amd/pair_attn.py and ours_soft.py).

The reference arithmetic is the dense formula softmax_j(scale q_i . k_j) v_j, run in fp64 on the CPU on the operands as rounded
to the storage dtype.  The operands are generated bf16-representable, so both storage dtypes see the same values and one
reference per shape serves both.

Bars (the project's, of tests/test_gpu_pair_attn.py: P <= 1 is rounded exactly as S was).  Forward, elementwise: fp32
|out - ref| <= 1e-4 max|v|; bf16 <= 2^-7 max|v|.  Backward, per gradient: ||err|| <= tol (||ref|| + 1e-2 gmax) with tol = 1e-3
(fp32) / 8e-2 (bf16).  lse: fp32 |err| <= 1e-5 max(1, |lse|); bf16 |err| <= 2^-9 (1 + |lse|) (the kernel sums P in fp32 before the
operand is rounded; the hardware exp2 and the bf16 scores' fp32 accumulation are what is left).  One case has a bar of its own,
MOVING_FWD_BAR below says why.  Each check prints
`PAIR_RATIO <name> <error / bar>` before it asserts (pytest -s shows them; profiles/pair_softmax_probe.md records the worst).

The module: after set_softmax_over('keys') it runs the kernels (SGF_PAIR_SOFTMAX=1) and meets the dense path and the fixtures'
`keys` recording; as constructed it computes the reference as shipped (a softmax over the heads, plain PyTorch) and meets the
fixtures' `logits` / `grad/*` recording, under SGF_PAIR_SOFTMAX=1 too."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_gpu_pair_attn import _exact_case  # noqa: E402  (the construction, and its cache, of the sigmoid tests)
from tests.test_ours_soft_host import FIXTURES, build_model, compare, load_fixture, run_step  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
SHAPES = [(1, 1), (31, 33), (33, 31), (70, 193), (257, 255), (1031, 1031)]
ULP = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7}        # spacing of the storage type relative to a power of two
FWD_BAR = {torch.float32: 1e-4, torch.bfloat16: 2.0 ** -7}
GRAD_TOL = {torch.float32: 1e-3, torch.bfloat16: 8e-2}


def _lse_bar(dtype, lse_ref):
    a = lse_ref.abs()
    return 1e-5 * a.clamp_min(1.0) if dtype == torch.float32 else 2.0 ** -9 * (1.0 + a)


def _ratio(name, err, bar):
    r = float(err) / float(bar) if bar > 0 else (0.0 if err == 0 else float("inf"))
    print(f"PAIR_RATIO {name} {r:.4f}")
    return r


def _lap_shapes(d, dtype):
    """(n, l) at which a workgroup of one of the kernels walks three tiles (none while every workgroup owns one tile)."""
    from sgformer_amd import _lib
    code = _lib.SGF_BF16 if dtype == torch.bfloat16 else _lib.SGF_F32
    rows = [int(_lib.load().sgf_pair_softmax_lap_rows(w, 3, d, code, 3)) for w in (0, 1, 2)]
    return [(r, 65) if w < 2 else (65, r) for w, r in enumerate(rows) if r > 0]


def _entries(q, k, v, g, scale=1.0):
    """(out, lse, dq, dk, dv) of the three launches on tensors that are already on the GPU"""
    from sgformer_amd.pair_attn import _Hip
    out, lse = _Hip.pair_softmax_fwd(q, k, v, scale)
    dq, delta = _Hip.pair_softmax_bwd_q(g, out, lse, q, k, v, scale)
    dk, dv = _Hip.pair_softmax_bwd_kv(g, lse, delta, q, k, v, scale)
    return out, lse, dq, dk, dv


def _dense64(q, k, v, g, scale):
    """(out, lse, dq, dk, dv) of the dense formula in fp64 on the CPU"""
    h = q.shape[1]
    ops = [t.clone().requires_grad_(True) for t in (q, k, v)]
    z = scale * torch.einsum("nhd,lhd->nlh", ops[0], ops[1])
    out = torch.einsum("nlh,lhd->nhd", torch.softmax(z, dim=1), ops[2].expand(-1, h, -1))
    out.backward(g)
    return out.detach(), torch.logsumexp(z.detach(), dim=1), ops[0].grad, ops[1].grad, ops[2].grad


def _check_grads(tag, dtype, got, ref):
    """the worst ratio of (dq, dk, dv) against the fp64 gradients under the gradient bar"""
    gmax = max(float(t.norm()) for t in ref)
    worst = 0.0
    for name, a, b in zip(("dq", "dk", "dv"), got, ref):
        bar = GRAD_TOL[dtype] * (float(b.norm()) + 1e-2 * gmax)
        worst = max(worst, _ratio(f"{tag}.{name}", (a.double().cpu() - b).norm(), bar))
    return worst


# ------------------------------------------------------------------------------------------------
# 1. exact masks: layout, tails, the masked keys
# ------------------------------------------------------------------------------------------------
_exact_grads = {}


def _check_exact(cuda, dtype, n, l, h, hv, d, wide=False):
    """z is 32 or -128: after the maximum P is exactly 1 or 0 (exp(-160) is 0 in fp32), so r is the count of keys a row keeps,
    lse = 32 + log(count) and out the masked mean.  dq and dk are not zero (dZ = P (g . v - delta)): against fp64."""
    q, k, v, g, count, out_ref, dv_ref = _exact_case(n, l, h, hv, d)
    key = (n, l, h, hv, d)
    if key not in _exact_grads:
        _exact_grads[key] = _dense64(q, k, v, g, 1.0)[2:]
    grads_ref = _exact_grads[key]

    def dev(t):
        t = t.to(cuda, dtype)
        if not wide:
            return t
        buf = torch.full((t.shape[0], t.shape[1] * t.shape[2] + 24), 77.0, device=cuda, dtype=dtype)       # ld > H * D
        view = buf[:, 8:8 + t.shape[1] * t.shape[2]].view(t.shape[0], t.shape[1], t.shape[2])
        view.copy_(t)
        return view
    out, lse, dq, dk, dv = _entries(dev(q), dev(k), dev(v), dev(g))
    tag = f"exact[{str(dtype)[6:]},{n}x{l},H{h},Hv{hv},D{d}{',wide' if wide else ''}]"
    lse_ref = 32.0 + torch.log(count)
    err = (lse.double().cpu() - lse_ref).abs()
    ulp = 2.0 ** -23 * torch.exp2(torch.floor(torch.log2(lse_ref)))
    assert bool((err <= ulp).all()), (tag, "lse", float((err / ulp).max()))
    err = (out.double().cpu() - out_ref).abs()
    ulp = ULP[dtype] * torch.exp2(torch.floor(torch.log2(out_ref.abs().clamp_min(1e-30))))
    assert bool((err <= ulp).all()), (tag, "out", float((err / ulp).max()))
    bar = GRAD_TOL[dtype] * (1.0 + 1e-2) * float(dv_ref.norm())
    assert _ratio(tag + ".dv_masked_mean", (dv.double().cpu() - dv_ref).norm(), bar) <= 1.0, tag
    assert n * l == 1 or (float(grads_ref[0].norm()) > 0 and float(grads_ref[1].norm()) > 0)      # unlike sigmoid: not zero
    assert _check_grads(tag, dtype, (dq, dk, dv), grads_ref) <= 1.0, tag


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
# 2. parity against fp64: the shared check, the moving maximum, random operands
# ------------------------------------------------------------------------------------------------
def _check_parity(cuda, dtype, tag, case, scale, finite_only=False, fwd_bar=None):
    q, k, v, g, ref = case
    out, lse, dq, dk, dv = _entries(*(t.to(cuda, dtype) for t in (q, k, v, g)), scale)
    tag = f"{tag}[{str(dtype)[6:]},{q.shape[0]}x{k.shape[0]},H{q.shape[1]},Hv{v.shape[1]},D{q.shape[2]},s{scale}]"
    worst = _ratio(tag + ".out", (out.double().cpu() - ref[0]).abs().max(), (fwd_bar or FWD_BAR[dtype]) * float(v.abs().max()))
    worst = max(worst, _ratio(tag + ".lse", ((lse.double().cpu() - ref[1]).abs() / _lse_bar(dtype, ref[1])).max(), 1.0))
    worst = max(worst, _check_grads(tag, dtype, (dq, dk, dv), ref[2:]))
    for t in (out, lse, dq, dk, dv):
        assert bool(torch.isfinite(t).all()), tag
    if not finite_only:
        assert worst <= 1.0, tag


_moving = {}


def _moving_case(kind, block):
    """n = 130 (one query tile and a tail), l = 1031, H = 2, Hv = 1, D = 64.  Feature 0 carries the maximum: q_i[0] = 64 and
    k_j[0] = 0.625 b(j), so z gains 40 b(j) over a random part of a few units (the large factor sits in q: dq = sum_j dZ k_j
    cancels over the keys, and a large common k[0] would only multiply the rounding of delta = g . out, out being stored in
    bf16, into a feature whose true gradient is 0).  'last': b = 1 on the keys from 1024 on (the last swept tile of both
    dtypes' kernels); 'first': b = 1 on keys 0 .. 31; 'rising': b = j // block, the row maximum rises by 40 from block to
    block (32: every tile of the fp32 kernels, 64: every tile of the bf16 kernels) and every rescale factor exp(m - m')
    underflows toward 0."""
    key = (kind, block)
    if key not in _moving:
        n, l, h, hv, d = 130, 1031, 2, 1, 64
        gen = torch.Generator().manual_seed(77 + block)

        def rnd(*shape, scale=1.0):
            return (scale * torch.randn(*shape, generator=gen)).bfloat16().double()
        q, k = rnd(n, h, d, scale=2.0 / d ** 0.5), rnd(l, h, d, scale=2.0 / d ** 0.5)
        j = torch.arange(l)
        b = (j >= 1024) if kind == "last" else (j < 32) if kind == "first" else j // block
        q[:, :, 0] = 64.0
        k[:, :, 0] = (0.625 * b.double())[:, None]                      # 5 b / 8 with 5 b <= 160: exact in bf16
        v, g = rnd(l, hv, d), rnd(n, h, d)
        _moving[key] = (q, k, v, g, _dense64(q, k, v, g, 1.0))
    return _moving[key]


# fp32, the maximum rising by 40 with every 32-row tile: the scores reach 1280, where one fp32 rounding is 2^-14 = 6e-5 and the
# score's 32 accumulation steps (v_mfma_f32_32x32x2_f32 over D = 64) leave about sqrt(32 / 3) 2^-14 = 2e-4 of absolute error in z,
# which is the RELATIVE error of P = exp(z - m) — in any fp32 evaluation, the dense one included.  Measured on the MI355X against
# fp64: max |out - ref| = 1.9791e-4 max|v| (0.8232e-4 with the rise every 64 rows, scores to 640, which stays under the 1e-4 bar).
# The bar of this one case is twice the measured value, the project's rule for a bound the formats set.
MOVING_FWD_BAR = {("rising", 32, torch.float32): 2 * 1.9791e-4}


@pytest.mark.parametrize("kind,block", [("last", 0), ("first", 0), ("rising", 32), ("rising", 64)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_running_maximum_moves(cuda, dtype, kind, block):
    _check_parity(cuda, dtype, f"moving.{kind}{block or ''}", _moving_case(kind, block), 1.0,
                  fwd_bar=MOVING_FWD_BAR.get((kind, block, dtype)))


_random = {}


def _random_case(n, l, h, hv, d, scale=1.0, zmax=None):
    """bf16-representable operands and the fp64 reference (out, lse, dq, dk, dv), made once per shape and scale"""
    key = (n, l, h, hv, d, scale, zmax)
    if key not in _random:
        gen = torch.Generator().manual_seed(1 + n + 3 * l + 5 * h + 7 * hv + 11 * d)

        def rnd(*shape, scale=1.0):
            return (scale * torch.randn(*shape, generator=gen)).bfloat16().double()
        q, k = rnd(n, h, d, scale=2.0 / d ** 0.5), rnd(l, h, d, scale=2.0 / d ** 0.5)
        if zmax is not None:
            z = scale * torch.einsum("nhd,lhd->nlh", q, k).abs().max()
            q = (q * (zmax / z)).bfloat16().double()
        v, g = rnd(l, hv, d), rnd(n, h, d)
        _random[key] = (q, k, v, g, _dense64(q, k, v, g, scale))
    return _random[key]


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("h,hv,d", [(1, 1, 64), (2, 2, 32), (3, 1, 128), (3, 3, 64), (2, 1, 64)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_random_parity(cuda, dtype, h, hv, d, scale):
    for n, l in [(257, 255), (1031, 1031)] + _lap_shapes(d, dtype):
        _check_parity(cuda, dtype, "random", _random_case(n, l, h, hv, d, scale), scale)


@pytest.mark.parametrize("dtype", DTYPES)
def test_scores_of_a_few_thousand_stay_finite(cuda, dtype):
    """|z| up to 3000: every output finite (the ratios are printed, the bars are not asserted here)."""
    case = _random_case(257, 255, 2, 2, 64, zmax=3000.0)
    assert 2500.0 <= float(torch.einsum("nhd,lhd->nlh", case[0], case[1]).abs().max()) <= 3500.0
    _check_parity(cuda, dtype, "large", case, 1.0, finite_only=True)


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
    q, k, v, g = (t.to(cuda, dtype) for t in _random_case(1031, 1031, 3, 1, 128)[:4])        # dv summed over the heads
    for x, y in zip(_entries(q, k, v, g), _entries(q, k, v, g)):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------
# 4. the module and the free function: kernels against the dense path, and against the fixtures
# ------------------------------------------------------------------------------------------------
class _Data:
    def __init__(self, x, ei):
        self.graph = {"node_feat": x, "edge_index": ei}


def _module_run(cuda, dtype, x, ei, y, state, heads, use_weight):
    from sgformer_amd import ours_medium, ours_soft
    f = x.shape[1]
    m = ours_soft.SGFormerSOFT(f, 64, 7, num_layers=2, num_heads=heads, dropout=0.0, use_weight=use_weight,
                               gnn=ours_medium.GCN(f, 64, 64, dropout=0.0)).set_softmax_over("keys")
    if state is None:
        return m.state_dict()
    m.load_state_dict(state)
    m = m.to(cuda).train()
    logits = m(_Data(x.to(cuda, dtype), ei.to(cuda)))
    torch.nn.functional.cross_entropy(logits.float(), y.to(cuda)).backward()
    return logits.detach().double().cpu(), {k: p.grad.double().cpu() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("heads,use_weight", [(2, True), (1, False)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_module_matches_the_dense_path(cuda, dtype, monkeypatch, heads, use_weight):
    from sgformer_amd import pair_attn
    n, f = 1500, 40
    torch.manual_seed(5)
    state = _module_run(None, None, torch.empty(0, f), None, None, None, heads, use_weight)
    x = torch.randn(n, f)
    src = torch.randint(0, n, (8 * n,))
    dst = (src + 1 + torch.randint(0, n - 1, (8 * n,))) % n
    ei = torch.stack([torch.cat([src, dst]), torch.cat([dst, src])])
    y = torch.randint(0, 7, (n,))
    monkeypatch.setenv("SGF_PAIR_SOFTMAX", "0")
    ref, ref_g = _module_run(cuda, dtype, x, ei, y, state, heads, use_weight)
    monkeypatch.setenv("SGF_PAIR_SOFTMAX", "1")
    calls = []
    fwd = pair_attn._Hip.pair_softmax_fwd
    monkeypatch.setattr(pair_attn._Hip, "pair_softmax_fwd", staticmethod(lambda *a: (calls.append(1), fwd(*a))[1]))
    got, got_g = _module_run(cuda, dtype, x, ei, y, state, heads, use_weight)
    assert len(calls) == 2                                        # both layers took the kernels
    tag = f"module[{str(dtype)[6:]},H{heads}]"
    if dtype == torch.float32:
        assert _ratio(tag + ".logits", (got - ref).abs().max(), 1e-4) <= 1.0
    else:
        assert _ratio(tag + ".logits", (got - ref).norm() / ref.norm(), 3e-2) <= 1.0
    gmax = max(float(g.norm()) for g in ref_g.values())
    assert set(got_g) == set(ref_g)
    for k, g in ref_g.items():
        bar = GRAD_TOL[dtype] * (float(g.norm()) + 1e-2 * gmax)
        assert _ratio(f"{tag}.{k}", (got_g[k] - g).norm(), bar) <= 1.0, k


@pytest.mark.parametrize("dtype", DTYPES)
def test_free_function_matches_the_dense_path(cuda, dtype, monkeypatch):
    from sgformer_amd import ours_soft
    q0, k0, v0, g0 = (t.to(cuda, dtype) for t in _random_case(257, 255, 2, 2, 32)[:4])
    res = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("SGF_PAIR_SOFTMAX", switch)
        ops = [t.clone().requires_grad_(True) for t in (q0, k0, v0)]
        out = ours_soft.softmax_attention(ops[0], ops[1], ops[2], over="keys")
        out.backward(g0)
        res[switch] = [out.detach().double().cpu()] + [t.grad.double().cpu() for t in ops]
    assert type(out.grad_fn).__name__.startswith("_SoftmaxAttention")
    ref, got = res["0"], res["1"]
    if dtype == torch.float32:
        assert float((got[0] - ref[0]).abs().max()) <= 1e-4
    else:
        assert float((got[0] - ref[0]).norm() / ref[0].norm()) <= 3e-2
    gmax = max(float(t.norm()) for t in ref[1:])
    for a, b in zip(got[1:], ref[1:]):
        assert float((a - b).norm()) <= GRAD_TOL[dtype] * (float(b.norm()) + 1e-2 * gmax)


def _fixture_run(cuda, dtype, path, monkeypatch, over):
    from sgformer_amd import pair_attn
    meta, state, x, ei, y, rec = load_fixture(path)
    monkeypatch.setenv("SGF_PAIR_SOFTMAX", "1")
    calls = []
    fwd = pair_attn._Hip.pair_softmax_fwd
    monkeypatch.setattr(pair_attn._Hip, "pair_softmax_fwd", staticmethod(lambda *a: (calls.append(1), fwd(*a))[1]))
    m = build_model(meta, over)
    m.load_state_dict(state)
    logits, grads = run_step(m.to(cuda), x.to(cuda, dtype), ei.to(cuda), y.to(cuda))
    assert len(calls) == (meta["num_layers"] if over == "keys" else 0)
    return logits, grads, rec


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
@pytest.mark.parametrize("dtype", DTYPES)
def test_module_matches_the_fixtures(cuda, dtype, monkeypatch, path):
    """the reference's code with the softmax over the keys (the fixtures' `keys` recording).  fp32: logits 1e-4 max(1, |ref|)
    elementwise; bf16: 3e-2 of the logits' norm (the whole model in bf16 storage, the bar of the other modules' bf16 parity);
    gradients under the gradient bars."""
    logits, grads, rec = _fixture_run(cuda, dtype, path, monkeypatch, "keys")
    tag = f"fixture[{str(dtype)[6:]},{os.path.basename(path)}]"
    if dtype == torch.float32:
        assert compare(tag, logits, grads, *rec["keys"], 1e-4, GRAD_TOL[dtype]) <= 1.0
    else:
        ref = rec["keys"][0].double()
        assert _ratio(tag + ".logits", (logits - ref).norm() / ref.norm(), 3e-2) <= 1.0
        assert compare(tag, ref, grads, *rec["keys"], 1e-4, GRAD_TOL[dtype]) <= 1.0          # (the gradients only)


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_module_matches_the_fixture_as_shipped(cuda, monkeypatch, path):
    """the module as constructed against the reference as shipped (softmax over the heads; no kernel call, SGF_PAIR_SOFTMAX=1)"""
    logits, grads, rec = _fixture_run(cuda, torch.float32, path, monkeypatch, "heads")
    assert compare(f"fixture_shipped[{os.path.basename(path)}]", logits, grads, *rec["shipped"], 1e-4, GRAD_TOL[torch.float32]) <= 1.0


# ------------------------------------------------------------------------------------------------
# 5. a size the dense path cannot reach
# ------------------------------------------------------------------------------------------------
def test_forty_thousand_nodes_without_a_score_tensor(cuda):
    """n = l = 40 009, H = 2, D = 64, bf16: one dense score tensor would be 12.8 GB; the kernels' peak stays within 256 MB of
    the operands.  out, lse and dq on 64 fixed query rows against the fp64 formula over all keys."""
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
    out = pair_attn.softmax_attention(*ops)
    out.backward(gd)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"PAIR_MEMORY rise_mb {rise / 2 ** 20:.1f}")
    assert rise < 256 * 2 ** 20
    for t in (out, ops[0].grad, ops[1].grad, ops[2].grad):
        assert bool(torch.isfinite(t).all())
    rows = (torch.arange(64) * 631 + 17) % n
    qr, gr = q[rows].double(), g[rows].double()
    z = torch.einsum("nhd,lhd->nlh", qr, k.double())
    p = torch.softmax(z, dim=1)
    out_ref = torch.einsum("nlh,lhd->nhd", p, v.double())
    delta = (gr * out_ref).sum(2)
    dz = p * (torch.einsum("nhd,lhd->nlh", gr, v.double()) - delta[:, None, :])
    dq_ref = torch.einsum("nlh,lhd->nhd", dz, k.double())
    rows = rows.to(cuda)
    worst = _ratio("big[bfloat16].out", (out.detach()[rows].double().cpu() - out_ref).abs().max(), FWD_BAR[dtype] * float(v.abs().max()))
    bar = GRAD_TOL[dtype] * (1.0 + 1e-2) * float(dq_ref.norm())
    worst = max(worst, _ratio("big[bfloat16].dq", (ops[0].grad[rows].double().cpu() - dq_ref).norm(), bar))
    assert worst <= 1.0
    assert math.isfinite(worst)
