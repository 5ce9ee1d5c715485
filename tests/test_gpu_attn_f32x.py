"""The one-head attention from the un-projected input over fp32 storage under torch.set_float32_matmul_precision('high'):
sgf_attn_h_fwd / _bwd_apply / _bwd_reduce with SGF_F32_BF16X3 (csrc/attn_f32x.hip), called through kernels.HipKernels, against
fp64 within the split-bf16 bound of DESIGN.md §4.  With P the same product over absolute values and ACC = 5e-6 the fp32
accumulation allowance of the exact-path tests:

    forward          |out - out64| <= 2^-14 (|h| |M|) / |den| + ACC max|out64|;  den (not split) relative 2e-5
    backward apply   |dh - dh64|   <= 2^-14 (|dnum| |M|^T + |h| |D|) + ACC max|dh64|
    backward reduce  d x d block within 2^-14 |h|^T |dnum| + ACC max; the vector blocks (fp32 VALU sums in both paths) at the
                     tolerance tests/test_gpu_kernels.py holds them to (relative 1e-5)

For n >= 4097 and d in {64, 128, 256} the 'high' result differs bitwise from the 'highest' one (the split kernels ran: this
fails without them), two 'high' launches are bit-identical, and 'highest' is bit-identical before and after a 'high' call.
den = h.w + beta stays near beta = 3 (|h.w| < 1), so the bounds measure the products and not a cancelling denominator."""
import contextlib

import pytest
import torch

from oracle import sgformer_oracle as O

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


def _strided(t, pad=4):
    """t as a column slice of a wider tensor (leading dimension = width + pad)."""
    big = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=t.dtype, device=t.device)
    big[:, : t.shape[1]] = t
    return big[:, : t.shape[1]]


def _check(out, ref, p, what):
    err = (out.double() - ref).abs()
    tol = BOUND * p + ACC * float(ref.abs().max()) + 1e-30
    bad = err > tol
    print(f"{what}: max err {float(err.max()):.3e}, max err / tol {float((err / tol).max()):.3f}")
    assert not bool(bad.any()), (what, float(err.max()), int(bad.sum()))


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _operands(cuda, n, d, seed):
    g_ = torch.Generator(device=cuda).manual_seed(seed)
    h = _strided(torch.randn(n, d, generator=g_, device=cuda))
    g = _strided(torch.randn(n, d, generator=g_, device=cuda))
    M = torch.randn(d, d, generator=g_, device=cuda) / d ** 0.5
    D = torch.randn(d, d, generator=g_, device=cuda) / d ** 0.5
    m = torch.randn(d, generator=g_, device=cuda)
    w = 0.5 * torch.rand(d, generator=g_, device=cuda) / d           # |h.w| < 1 (asserted by the caller)
    ds = torch.randn(d, generator=g_, device=cuda)
    beta = torch.full((1,), 3.0, device=cuda)
    return h, g, M, D, m, w, ds, beta


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("n", NS)
def test_three_entries_against_fp64(cuda, n, d):
    from sgformer_amd import ops
    K = ops.K
    h, g, M, D, m, w, ds, beta = _operands(cuda, n, d, 7 * n + d)
    h64, g64, M64, D64 = h.double(), g.double(), M.double(), D.double()
    den64 = h64 @ w.double() + 3.0
    assert float((den64 - 3.0).abs().max()) < 1.0
    den64 = den64.reshape(-1, 1)

    # ---- forward ----
    with precision("highest"):
        o0, den0 = K.attn_h_fwd(h, M, m, w, beta)
    with precision("high"):
        o1, den1 = K.attn_h_fwd(h, M, m, w, beta)
        o1b, den1b = K.attn_h_fwd(h, M, m, w, beta)
    with precision("highest"):
        o2, den2 = K.attn_h_fwd(h, M, m, w, beta)
    assert o1.dtype == torch.float32 and den1.shape == (n, 1)
    out64 = (h64 @ M64 + m.double()) / den64
    _check(o1, out64, (h64.abs() @ M64.abs()) / den64.abs(), f"fwd n={n} d={d}")
    for den in (den0, den1):
        assert float(((den.double() - den64).abs() / den64.abs()).max()) <= 2e-5
    assert torch.equal(o1, o1b) and torch.equal(den1, den1b)           # deterministic
    assert torch.equal(o0, o2) and torch.equal(den0, den2)             # no state leaks into 'highest'

    # ---- backward, from the SAME saved (out, den) under both settings ----
    o = _strided(o0)
    den = den0
    inv64 = 1.0 / den.double()
    o64 = o.double()
    dnum64 = g64 * inv64
    dden64 = -(g64 * o64).sum(1, keepdim=True) * inv64

    with precision("highest"):
        dh0 = K.attn_h_bwd_apply(h, g, o, den, M, w, D, ds)
        hs0 = K.attn_h_bwd_reduce(h, g, o, den)
    with precision("high"):
        dh1 = K.attn_h_bwd_apply(h, g, o, den, M, w, D, ds)
        hs1 = K.attn_h_bwd_reduce(h, g, o, den)
        dh1b = K.attn_h_bwd_apply(h, g, o, den, M, w, D, ds)
        hs1b = K.attn_h_bwd_reduce(h, g, o, den)
    with precision("highest"):
        dh2 = K.attn_h_bwd_apply(h, g, o, den, M, w, D, ds)
        hs2 = K.attn_h_bwd_reduce(h, g, o, den)
    dh64 = dnum64 @ M64.t() + dden64 * w.double() + h64 @ D64 + ds.double()
    _check(dh1, dh64, dnum64.abs() @ M64.abs().t() + h64.abs() @ D64.abs(), f"bwd apply n={n} d={d}")
    assert hs1.shape == (d * d + 2 * d + 1,)
    _check(hs1[: d * d].reshape(d, d), h64.t() @ dnum64, h64.abs().t() @ dnum64.abs(), f"bwd reduce n={n} d={d}")
    for hs in (hs0, hs1):
        assert _rel(hs[d * d: d * d + d], (h64 * dden64).sum(0)) <= 1e-5
        assert _rel(hs[d * d + d: d * d + 2 * d], dnum64.sum(0)) <= 1e-5
        assert abs(float(hs[-1]) - float(dden64.sum())) <= 1e-5 * max(1.0, float(dden64.abs().sum()))
    assert torch.equal(dh1, dh1b) and torch.equal(hs1, hs1b)
    assert torch.equal(dh0, dh2) and torch.equal(hs0, hs2)
    if n >= 4097 and d in (64, 128, 256):
        assert not torch.equal(o1, o0)
        assert not torch.equal(dh1, dh0)
        assert not torch.equal(hs1[: d * d], hs0[: d * d])


def test_empty_input(cuda):
    from sgformer_amd import ops
    K = ops.K
    d = 64
    h, g, M, D, m, w, ds, beta = _operands(cuda, 0, d, 3)
    with precision("high"):
        o, den = K.attn_h_fwd(h, M, m, w, beta)
        hs = K.attn_h_bwd_reduce(h, g, o, den)
        dh = K.attn_h_bwd_apply(h, g, o, den, M, w, D, ds)
    assert o.shape == (0, d) and dh.shape == (0, d) and int(torch.count_nonzero(hs)) == 0


@pytest.mark.parametrize("d", [64, 256])
def test_non_finite_inputs_propagate(cuda, d):
    """inf / -inf / NaN planted in h and in g: whatever is non-finite under 'highest' is non-finite under 'high', and NaNs
    stay NaNs."""
    from sgformer_amd import ops
    K = ops.K
    n = 5000
    h, g, M, D, m, w, ds, beta = _operands(cuda, n, d, 11 + d)
    with precision("highest"):
        o, den = K.attn_h_fwd(h, M, m, w, beta)          # finite saved tensors for the backward
    o, den = o.clone(), den.clone()
    hp, gp = h.clone(), g.clone()
    hp[10, 3], hp[20, 5], hp[30, 7] = float("inf"), float("-inf"), float("nan")
    gp[40, 3], gp[50, 5], gp[60, 7] = float("inf"), float("-inf"), float("nan")

    def both(fn):
        with precision("highest"):
            a = fn()
        with precision("high"):
            b = fn()
        return a, b

    pairs = []
    (oe, dene), (oh, denh) = both(lambda: K.attn_h_fwd(hp, M, m, w, beta))
    pairs += [(oe, oh), (dene, denh)]
    for hh, gg in ((hp, g), (h, gp), (hp, gp)):
        pairs.append(both(lambda: K.attn_h_bwd_apply(hh, gg, o, den, M, w, D, ds)))
        pairs.append(both(lambda: K.attn_h_bwd_reduce(hh, gg, o, den)))
    for ex, hi_ in pairs:
        nf = ~torch.isfinite(ex)
        assert bool(nf.any()) and bool((~torch.isfinite(hi_[nf])).all())
        assert torch.equal(torch.isnan(ex), torch.isnan(ex) & torch.isnan(hi_))


def test_attention_from_input_under_high(cuda):
    """ops.attention_from_input forward + backward on fp32 inputs under 'high' against the fp64 oracle applied to explicitly
    projected Q / K / V (as tests/test_gpu_kernels.py::test_attention_from_input; n_total = 4 so that the all-pair term is
    O(1)), RELATIVE (Frobenius) errors of the output, of dh and of the six parameter gradients.

    Tolerance.  A parameter gradient is not one product but the end of a chain (G = h^T h, out = (h M + m) / den,
    dM = h^T dnum, dh = dnum M^T + h D, with the d x d algebra in between), so it is not derived in closed form.  As the
    exact path runs the same chain on the same inputs, its own error against fp64 is measured here first; it carries the
    chain's conditioning.  The split path may add, per split product on the way to a quantity, the relative (Frobenius)
    size of the per-product bound, 2^-14 kappa with kappa = || |A| |B| || / || A B ||; kappa is taken as the largest of
    the four row-pass products (computed below in fp64 from the oracle's own tensors), and at most four split products lie
    on any path from the inputs to a checked quantity (G, h M, h^T dnum, one apply product):

        tol(q) = err_highest(q) + 4 * 2^-14 * kappa."""
    from sgformer_amd import ops
    from tests import attn_algebra as A
    n, d, n_total = 3000, 256, 4.0
    g_ = torch.Generator().manual_seed(n + d)
    h = torch.relu(torch.randn(n, d, generator=g_)) * 0.8 + 0.05
    ws = [torch.randn(d, d, generator=g_) / d ** 0.5 for _ in range(3)]
    bs = [torch.randn(d, generator=g_) * 0.1 for _ in range(3)]
    wgt = torch.randn(n, d, generator=g_)

    hd = h.double().requires_grad_(True)
    wd = [w.double().requires_grad_(True) for w in ws]
    bd = [b.double().requires_grad_(True) for b in bs]
    q = (hd @ wd[0].t() + bd[0]).unsqueeze(1)
    k = (hd @ wd[1].t() + bd[1]).unsqueeze(1)
    v = (hd @ wd[2].t() + bd[2]).unsqueeze(1)
    ref = O.attention(q, k, v, n_total=n_total)
    (ref * wgt.double()).sum().backward()
    refs = {"out": ref.detach().reshape(n, d), "dh": hd.grad}
    for i, nm in enumerate("qkv"):
        refs["dW" + nm], refs["db" + nm] = wd[i].grad, bd[i].grad

    # kappa of the row-pass products, in fp64
    with torch.no_grad():
        h64 = h.double()
        M, m, w, beta = A.attn_h_small(h64.t() @ h64, h64.sum(0), float(n), n_total, wd[0], bd[0], wd[1], bd[1], wd[2], bd[2])
        den = (h64 @ w + beta).reshape(-1, 1)
        out = (h64 @ M + m) / den
        assert _rel(out, refs["out"]) <= 1e-9
        dnum = wgt.double() / den
        kappa = max(float((h64.abs() @ M.abs()).norm() / (h64 @ M).norm()),
                    float((dnum.abs() @ M.abs().t()).norm() / (dnum @ M.t()).norm()),
                    float((h64.abs().t() @ dnum.abs()).norm() / (h64.t() @ dnum).norm()),
                    1.0)                                            # G = h^T h with h >= 0: no cancellation

    def run():
        hg = h.to(cuda).requires_grad_(True)
        wg = [w_.to(cuda).requires_grad_(True) for w_ in ws]
        bg = [b_.to(cuda).requires_grad_(True) for b_ in bs]
        o = ops.attention_from_input(hg, wg[0], bg[0], wg[1], bg[1], wg[2], bg[2], None, n_total)
        (o * wgt.to(cuda)).sum().backward()
        got = {"out": o.detach(), "dh": hg.grad}
        for i, nm in enumerate("qkv"):
            got["dW" + nm], got["db" + nm] = wg[i].grad, bg[i].grad
        return {k_: _rel(v_.cpu(), refs[k_]) for k_, v_ in got.items()}

    with precision("highest"):
        exact = run()
    with precision("high"):
        high = run()
    print(f"\nkappa = {kappa:.2f}, allowance 4 * 2^-14 * kappa = {4 * BOUND * kappa:.3e}")
    for k_ in refs:
        print(f"{k_}: 'highest' rel err {exact[k_]:.3e}, 'high' rel err {high[k_]:.3e}")
    for k_ in refs:
        assert high[k_] <= exact[k_] + 4 * BOUND * kappa, (k_, high[k_], exact[k_], kappa)
