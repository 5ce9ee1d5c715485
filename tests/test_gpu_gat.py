"""The edge-softmax kernels of csrc/gat.hip (include/sgf.h block N10) and sgformer_amd/gat.py on the GPU.

The reference is tests/gat_reference.py: GATConv's aggregation as dense fp64 algebra on the device, on the operands as rounded
to the storage dtype (the operands are generated bf16-representable, so both storage dtypes see the same values).

The ladder graph: 520 nodes, every node a target, in-degrees cycling through LADDER (or POW2 in the exact arm), sources
pseudo-random with parallel entries (every degree above 520 forces them) and self-loops; a variant empties a few rows.

Arms
  exact    att = 0 (every score is exactly 0), integer xw and g in [-8, 8], negative_slope = 1/4, in-degrees powers of two: out,
           delta, dar, dal, dxw equal the fp64 result rounded once (torch.equal), lse is logf(degree) to 1 ulp.  Every value is a
           dyadic rational that fp32 holds, and the case asserts so ("broken test" otherwise), as it asserts that the sums the
           kernels form on the way are short enough to be exact in any order.  On the full ladder the same inputs hold out to
           1 ulp of fp32 (a quotient by a degree that is no power of two is rounded; the head mean then adds H such values:
           (8 x 1/2 + 1/2 (2 + 4 + 8)) / 8 < 1 ulp at the magnitude of the largest per-head value).
  random   normal xw, att scaled so that the scores span about +-20, the largest score of the rows node 519 feeds coming last in
           the row: against the reference, forward and every gradient, under the bars below.
  dropout  p in {0.5, 0.9}: the host Philox mask (tests/cpu_kernels_gat.gat_keep) is fed to the reference; the random arm's
           bars (one wrong keep bit moves an output by |xw| / (L (1 - p)), far above them); bit-identical under the same seed,
           another `out` under another.
  laps     n = max(ceil(2.25 lap) + 5, 4099) targets for sgf_gat_lap_rows, degrees 1 - 4, the exact arm's inputs: every output of
           the four kernels against the module's fp64 edge-list path (held to the reference at small n in
           tests/test_gat_host.py) and the closed formulas over the edge list.
  module   GAT (2 and 3 layers, BatchNorm both ways) against its own edge-list path in fp64, and ours_medium.SGFormer with a GAT
           branch against itself with the branch on the edge-list path (the attention branch has no fp64 kernels), 2 000 nodes.

Bars of the random and dropout arms (derived, measured on the MI355X, set at twice the measured maximum, required
to sit under the derived bound).  With u = 2^-24, L the longest row walked (in- or out-degree), S = max_n,h sum_c |xw att| and
Z = max |z|, every weight p_e carries
    * its score's error: al and ar are C-term fp32 dot products, (C + 1) u S each, their sum and the leaky slope 2 u Z more, and
      that error enters p_e once through exp(s - m) and once through the normaliser: 2 (2 (C + 1) S + 2 Z) u, relative;
    * the normaliser's L-term sum, the exp and the product with 1 / l: (L + 8) u, relative;
and a result that sums L such terms of magnitude M adds L u M: in units of u M
    bound = 2 L + 4 (C + 1) S + 4 Z + 2 C + 16         (2 C: the C-term dot products dp of the backward)
M is per tensor: out: max|xw| / (1 - p); delta: D / (1 - p) with D = C max|g_h| max|xw|; dar: 2 D / (1 - p); dal: 2 D T / (1 - p)
with T the largest out-degree; dxw: (max|g_h| T + 2 D T max|att_l| + 2 D max|att_r|) / (1 - p); datt_l, datt_r: N max|xw| times
dal's / dar's M (ATen column sums over the nodes, N u more: the bound's L is then max(L, N)).  bf16 storage adds the one
rounding of out and dxw: half a bf16 spacing at the element's own magnitude is taken off every element's error.  BARS holds, per storage dtype and tensor, twice the largest measured error in units of
u M over all cases of both arms (the measured maxima are beside them and in profiles/gat_probe.md); each check prints
`GAT_UNITS <case> <tensor> <measured> <bound>` before it asserts."""
import math
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import gat_reference as R  # noqa: E402
from tests.cpu_kernels_gat import gat_keep  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
U = 2.0 ** -24
N = 520
LADDER = [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 3001]
POW2 = [1, 2, 4, 8, 16, 32, 64, 128, 256, 1024, 4096]
SHAPES = [(1, 4), (1, 64), (2, 32), (8, 8), (8, 32), (8, 64), (8, 128)]
DTYPES = [F32, BF16]
CASES = [(h, c, dt, concat) for (h, c) in SHAPES for dt in DTYPES for concat in (True, False)]
IDS = [f"h{h}c{c}-{'bf16' if dt == BF16 else 'f32'}-{'cat' if concat else 'mean'}" for h, c, dt, concat in CASES]
SLOPE_EXACT = 0.25

# twice the largest measured error in units of u M over the 28 cases of the random arm and the 56 of the dropout arm (the measured
# maximum on the MI355X is in the comment; profiles/gat_probe.md has the table), per storage dtype and tensor.  The smallest
# derived bound of any case is 6681 units.  bf16 out / dxw: beyond half a bf16 spacing of each element (_half_ulp_bf16).
BARS = {
    F32: dict(out=112.2,        # 56.091   random.h8c128-f32-cat
              lse=5.064,        # 2.5316   dropout0.9.h8c32-f32-mean
              delta=6.408,      # 3.2035   random.h8c8-f32-mean
              dar=3.128,        # 1.5632   random.h8c8-f32-cat
              dal=8.792e-3,     # 4.3951e-3 random.h8c8-f32-cat
              dxw=8.280e-3,     # 4.1396e-3 random.h8c8-f32-cat
              datt_l=2.172e-5,  # 1.0856e-5 random.h8c8-f32-mean
              datt_r=5.060e-3),  # 2.5296e-3 random.h8c8-f32-cat
    BF16: dict(out=42.71,       # 21.353   random.h1c64-bf16-mean
               lse=5.064,       # 2.5316   dropout0.9.h8c32-bf16-mean
               delta=6.408,     # 3.2035   random.h8c8-bf16-mean
               dar=3.128,       # 1.5632   random.h8c8-bf16-cat
               dal=8.792e-3,    # 4.3951e-3 random.h8c8-bf16-cat
               dxw=5.506e-3,    # 2.7528e-3 random.h8c8-bf16-cat
               datt_l=2.172e-5,  # 1.0856e-5 random.h8c8-bf16-mean
               datt_r=5.060e-3),  # 2.5296e-3 random.h8c8-bf16-cat
}


# ---- graphs ---------------------------------------------------------------------------------------------------------------
_graphs = {}


def ladder_graph(degrees, device, n=N, empty=()):
    """(edge_index [2, E] source / target, CSRGraph) with in-degree degrees[i % len] for target i (0 for i in `empty`); source k
    of target i is a fixed pseudo-random node, the first entry of every third row the row itself (a self-loop), node n - 1 a
    source of every row whose index is a multiple of 7 (it is the last entry there: the CSR is sorted by source)."""
    from sgformer_amd import ops
    key = (tuple(degrees), str(device), n, tuple(empty))
    if key not in _graphs:
        deg = torch.tensor([0 if i in empty else degrees[i % len(degrees)] for i in range(n)], dtype=torch.int64)
        tgt = torch.repeat_interleave(torch.arange(n), deg)
        k = torch.arange(tgt.numel()) - torch.repeat_interleave(torch.cumsum(deg, 0) - deg, deg)      # position in the row
        src = (tgt * 7919 + k * 104729 + (k * k % 1009) * 31 + 17) % n
        src = torch.where((k == 0) & (tgt % 3 == 0), tgt, src)
        src = torch.where((k == deg[tgt] - 1) & (tgt % 7 == 0) & (deg[tgt] > 1), torch.full_like(src, n - 1), src)
        ei = torch.stack([src, tgt]).to(device)
        _graphs[key] = (ei, ops.CSRGraph(ei, n))
    return _graphs[key]


def _degrees(graph):
    t_rowptr = graph.transposed()[0]
    return int((graph.rowptr[1:] - graph.rowptr[:-1]).max()), int((t_rowptr[1:] - t_rowptr[:-1]).max())


# ---- the four launches and the reference -------------------------------------------------------------------------------------
def run_entries(graph, xw, att_l, att_r, bias, g, heads, concat, slope, p=0.0, seed=0):
    """dict(out, lse, delta, dar, dal, dxw) of the four launches (the table gat._table() names: the HIP entries on the GPU)"""
    from sgformer_amd import gat
    t = gat._table()
    mean = not concat
    wl, wr = att_l.reshape(-1).float().contiguous(), att_r.reshape(-1).float().contiguous()
    al, ar = t.gat_scores(xw, wl, wr, heads)
    out, lse, norm = t.gat_fwd(graph.rowptr, graph.colind, xw, al, ar, bias, heads, mean, slope, p, seed)
    delta, dar = t.gat_bwd_dst(graph.rowptr, graph.colind, g, xw, al, ar, norm, heads, mean, slope, p, seed)
    t_rowptr, t_colind = graph.transposed()[:2]
    dal, dxw = t.gat_bwd_src(t_rowptr, t_colind, g, xw, al, ar, norm, delta, dar, wl, wr, heads, mean, slope, p, seed)
    return dict(out=out, lse=lse, delta=delta, dar=dar, dal=dal, dxw=dxw, al=al, ar=ar)


def reference(ei, n, xw, att_l, att_r, bias, g, heads, concat, slope, keep=None, p=0.0):
    mult = R.multiplicity(ei, n, add_self_loops=False)
    x3 = xw.double().view(n, heads, -1)
    out, lse = R.dense(x3, att_l.double(), att_r.double(), mult, slope, keep, p, concat, None if bias is None else bias.double())
    ref = R.backward(x3, att_l.double(), att_r.double(), mult, g.double(), slope, keep, p, concat)
    ref.update(out=out, lse=lse, dxw=ref["dxw"].reshape(n, -1), mult=mult)
    return ref


def _fp32_holds(t):
    return bool((t.float().double() == t).all())


def _ulp32(t):
    """spacing of fp32 at the magnitude of every element of the fp64 tensor t (the spacing above |t|)"""
    a = t.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def _half_ulp_bf16(ref, got=None):
    """per element: half the spacing of bfloat16 at the magnitude of the fp64 reference (or of the result where that is the
    larger): what the one rounding of an exact value to bf16 storage may move it by; 0 at 0"""
    a = ref.abs() if got is None else torch.maximum(ref.abs(), got.double().abs())
    _, e = torch.frexp(a)                                  # a = m 2^e, 1/2 <= m < 1: spacing 2^(e - 8)
    return torch.where(a > 0, torch.ldexp(torch.ones_like(a), e - 9), torch.zeros_like(a))


# ---- exact arm ------------------------------------------------------------------------------------------------------------
def _exact_inputs(n, heads, c, dtype, concat, device, seed=0):
    """integer xw, g in [-8, 8] (three quarters of them 0, so that the row sums stay short), att = 0, integer bias"""
    gen = torch.Generator().manual_seed(1000 * heads + c + seed)
    def ints(*shape):
        v = torch.randint(-8, 9, shape, generator=gen).float()
        return (v * (torch.rand(shape, generator=gen) < 0.25)).to(device)
    xw = ints(n, heads * c).to(dtype)
    g = ints(n, heads * c if concat else c).to(dtype)
    att = torch.zeros(heads, c, device=device)
    bias = torch.randint(-8, 9, (heads * c if concat else c,), generator=gen).float().to(device)
    return xw, g, att, bias


def _assert_sums_are_exact(ref, heads, concat, kmax):
    """broken-test guards: what the kernels add up on the way is exact in fp32 whatever the order — every term is a multiple
    of the quantum q and the sum of the magnitudes stays below 2^24 q"""
    gq = 1.0 if concat else 1.0 / heads                     # quantum of g_h (heads is a power of two here)
    q = 2.0 ** -kmax * gq
    mult = ref["mult"]
    p, sl, _ = R._weights(ref["x3"], ref["att"], ref["att"], mult, SLOPE_EXACT)
    p = p / mult.clamp_min(1.0)[:, :, None]                 # per stored entry (the kernels never see a pair's multiplicity)
    dp = torch.einsum("ihc,jhc->ijh", ref["gh"], ref["x3"])
    assert float((p * mult[:, :, None] * dp.abs()).sum(1).max()) < 2.0 ** 24 * q * SLOPE_EXACT, "broken test: delta / dar row sums too long"
    dz = p * (dp - ref["delta"][:, None, :]) * sl
    # dal sums thousands of dz whose quanta differ by the square of the degrees: the kernel adds them in fp64 and rounds once,
    # as the reference does; what must be exact is every term
    assert _fp32_holds(dp - ref["delta"][:, None, :]) and _fp32_holds(dz), "broken test: dz is not an fp32 value"
    assert float(torch.einsum("ijh,ihc->jhc", p * mult[:, :, None], ref["gh"].abs()).max()) < 2.0 ** 24 * q, "broken test: dxw sums too long"


@pytest.mark.parametrize("h,c,dtype,concat", CASES, ids=IDS)
def test_exact_on_power_of_two_degrees(cuda, h, c, dtype, concat):
    ei, graph = ladder_graph(POW2, cuda)
    xw, g, att, bias = _exact_inputs(N, h, c, dtype, concat, cuda)
    got = run_entries(graph, xw, att, att, bias, g, h, concat, SLOPE_EXACT)
    ref = reference(ei, N, xw, att, att, bias, g, h, concat, SLOPE_EXACT)
    ref.update(x3=xw.double().view(N, h, c), att=att.double(),
               gh=g.double().view(N, h, c) if concat else (g.double() / h)[:, None, :].expand(N, h, c))
    for name in ("out", "delta", "dar", "dxw"):
        assert _fp32_holds(ref[name]), f"broken test: the reference {name} is not an fp32 value"
    _assert_sums_are_exact(ref, h, concat, 12)
    for name in ("delta", "dar", "dal"):
        assert torch.equal(got[name], ref[name].float()), name
    for name in ("out", "dxw"):
        assert got[name].dtype == dtype and torch.equal(got[name], ref[name].to(dtype)), name
    deg = (graph.rowptr[1:] - graph.rowptr[:-1]).float()
    want = torch.log(deg)[:, None].expand(N, h)              # fp32 logf of the degree
    assert float(((got["lse"] - want).abs() / _ulp32(want.double()).float().clamp_min(2.0 ** -149)).max()) <= 1.0
    assert float(got["dal"].abs().max()) > 0 and float(got["delta"].abs().max()) > 0


@pytest.mark.parametrize("h,c,dtype,concat", CASES, ids=IDS)
def test_full_ladder_and_empty_rows(cuda, h, c, dtype, concat):
    empty = (5, 100, 519)
    for variant in ((), empty):
        ei, graph = ladder_graph(LADDER, cuda, empty=variant)
        xw, g, att, bias = _exact_inputs(N, h, c, dtype, concat, cuda, seed=1)
        got = run_entries(graph, xw, att, att, bias, g, h, concat, SLOPE_EXACT)
        ref = reference(ei, N, xw, att, att, bias, g, h, concat, SLOPE_EXACT)
        # 1 ulp of fp32 at the magnitude of the result (concat) or of the largest per-head value (mean); bf16: and its rounding
        per_head, _ = R.dense(xw.double().view(N, h, c), att.double(), att.double(), ref["mult"], SLOPE_EXACT, concat=True)
        mag = ref["out"] - bias.double() if concat else per_head.view(N, h, c).abs().max(1).values
        # (and the rounding of the sum with the bias; and the fp64 reference's own sum of up to 3001 products p x, |x| <= 8)
        tol = _ulp32(mag) + 0.5 * _ulp32(ref["out"]) + 3001 * 8 * 2.0 ** -53
        if dtype == BF16:
            tol = tol + _half_ulp_bf16(ref["out"], got["out"])
        err = (got["out"].double() - ref["out"]).abs()
        assert bool((err <= tol).all()), float((err / tol.clamp_min(1e-300)).max())
        for i in variant:                                   # an empty row: bias alone, lse 0, nothing backward
            assert torch.equal(got["out"][i], bias.to(dtype))
            assert float(got["lse"][i].abs().max()) == 0 and float(got["delta"][i].abs().max()) == 0
            assert float(got["dar"][i].abs().max()) == 0
        assert bool(torch.isfinite(got["dxw"].float()).all()) and bool(torch.isfinite(got["lse"]).all())


# ---- random arm -----------------------------------------------------------------------------------------------------------
def _random_inputs(n, heads, c, dtype, concat, device):
    """bf16-representable normal xw and g, att ~ N(0, 25 / C) (scores of standard deviation 7: about +-20), node n - 1 turned
    towards att_l so that its score is the largest of every row it feeds, where it comes last"""
    gen = torch.Generator().manual_seed(77 * heads + c)
    xw = torch.randn(n, heads, c, generator=gen)
    att_l = torch.randn(heads, c, generator=gen) * (5.0 / math.sqrt(c))
    att_r = torch.randn(heads, c, generator=gen) * (5.0 / math.sqrt(c))
    xw[n - 1] = att_l * (24.0 / (att_l * att_l).sum(1, keepdim=True))            # al[n - 1] = 24 for every head
    g = torch.randn(n, heads * c if concat else c, generator=gen)
    bias = torch.randn(heads * c if concat else c, generator=gen)
    rb = lambda t: t.bfloat16().float()
    return (rb(xw).reshape(n, heads * c).to(device).to(dtype), rb(g).to(device).to(dtype), rb(att_l).to(device),
            rb(att_r).to(device), bias.to(device))


def _scales(ref, xw, g, att_l, att_r, heads, c, concat, graph, p):
    """(bound in units of u M, M per tensor) of the module docstring"""
    n = xw.shape[0]
    x3 = xw.double().view(n, heads, c)
    lin, tout = _degrees(graph)
    s = float(torch.maximum((x3.abs() * att_l.double().abs()).sum(-1).max(), (x3.abs() * att_r.double().abs()).sum(-1).max()))
    al, ar = (x3 * att_l.double()).sum(-1), (x3 * att_r.double()).sum(-1)
    z = float(al.abs().max() + ar.abs().max())
    xmax, gmax = float(x3.abs().max()), float(g.double().abs().max()) / (1 if concat else heads)
    d = c * gmax * xmax
    ks = 1.0 / (1.0 - p)
    m = dict(out=xmax * ks, lse=max(1.0, float(ref["lse"].abs().max())), delta=d * ks, dar=2 * d * ks, dal=2 * d * tout * ks,
             dxw=(gmax * tout + 2 * d * tout * float(att_l.abs().max()) + 2 * d * float(att_r.abs().max())) * ks)
    m["datt_l"], m["datt_r"] = n * xmax * m["dal"], n * xmax * m["dar"]
    bound = 2 * max(lin, tout) + 4 * (c + 1) * s + 4 * z + 2 * c + 16
    return bound, 2 * max(lin, tout, n) + 4 * (c + 1) * s + 4 * z + 2 * c + 16, m


def _check_units(tag, dtype, got, ref, bound, bound_att, m):
    """every tensor against the reference: error in units of u M, printed, under the bar, the bar under the derived bound"""
    worst = {}
    for name in ("out", "lse", "delta", "dar", "dal", "dxw", "datt_l", "datt_r"):
        err = (got[name].double() - ref[name]).abs()
        if dtype == BF16 and name in ("out", "dxw"):         # the one rounding to bf16 storage, element by element
            err = (err - _half_ulp_bf16(ref[name], got[name])).clamp_min(0.0)
        err = float(err.max())
        worst[name] = err / (U * m[name])
        print(f"GAT_UNITS {tag} {name} {worst[name]:.4e} {bound_att if name.startswith('datt') else bound:.1f}")
    for name, units in worst.items():
        bar, lim = BARS[dtype][name], (bound_att if name.startswith("datt") else bound)
        assert bar is not None and bar <= lim, f"{name}: no bar under the derived bound {lim} (measured {units})"
        assert units <= bar, (name, units, bar)
    return worst


def _with_att_grads(got, xw, heads):
    x3 = xw.float().view(xw.shape[0], heads, -1)
    got["datt_l"] = torch.einsum("nh,nhc->hc", got["dal"], x3)
    got["datt_r"] = torch.einsum("nh,nhc->hc", got["dar"], x3)
    return got


@pytest.mark.parametrize("h,c,dtype,concat", CASES, ids=IDS)
def test_random_scores_against_the_reference(cuda, h, c, dtype, concat):
    ei, graph = ladder_graph(LADDER, cuda)
    xw, g, att_l, att_r, bias = _random_inputs(N, h, c, dtype, concat, cuda)
    got = _with_att_grads(run_entries(graph, xw, att_l, att_r, bias, g, h, concat, 0.2), xw, h)
    ref = reference(ei, N, xw, att_l, att_r, bias, g, h, concat, 0.2)
    # the construction: the scores span +-20 and the largest of row 7 is its last entry
    z = got["al"][graph.colind[graph.rowptr[7]:graph.rowptr[8]].long()] + got["ar"][7]
    assert int(graph.colind[graph.rowptr[8] - 1]) == N - 1 and bool((z.argmax(0) == z.shape[0] - 1).all())
    assert float((got["al"][:, None, :] + got["ar"][None, :, :]).abs().max()) >= 20.0
    bound, bound_att, m = _scales(ref, xw, g, att_l, att_r, h, c, concat, graph, 0.0)
    _check_units("random." + IDS[CASES.index((h, c, dtype, concat))], dtype, got, ref, bound, bound_att, m)


# ---- dropout arm ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.5, 0.9])
@pytest.mark.parametrize("h,c,dtype,concat", CASES, ids=IDS)
def test_dropout_follows_the_host_philox_mask(cuda, h, c, dtype, concat, p):
    seed = 0x1234567 * 1000003 + 17 * h + c
    ei, graph = ladder_graph(LADDER, cuda)
    xw, g, att_l, att_r, bias = _random_inputs(N, h, c, dtype, concat, cuda)
    got = _with_att_grads(run_entries(graph, xw, att_l, att_r, bias, g, h, concat, 0.2, p, seed), xw, h)
    ii, jj = torch.meshgrid(torch.arange(N, device=cuda), torch.arange(N, device=cuda), indexing="ij")
    keep = gat_keep(seed, ii.reshape(-1), jj.reshape(-1), h, p).view(N, N, h)
    ref = reference(ei, N, xw, att_l, att_r, bias, g, h, concat, 0.2, keep, p)
    bound, bound_att, m = _scales(ref, xw, g, att_l, att_r, h, c, concat, graph, p)
    _check_units(f"dropout{p}." + IDS[CASES.index((h, c, dtype, concat))], dtype, got, ref, bound, bound_att, m)
    again = run_entries(graph, xw, att_l, att_r, bias, g, h, concat, 0.2, p, seed)
    for name in ("out", "lse", "delta", "dar", "dal", "dxw"):
        assert torch.equal(again[name], got[name]), name     # the same seed: bit-identical
    other = run_entries(graph, xw, att_l, att_r, bias, g, h, concat, 0.2, p, seed + 1)
    assert not torch.equal(other["out"], got["out"]) and torch.equal(other["lse"], got["lse"])


# ---- lap arm --------------------------------------------------------------------------------------------------------------
def _lap_n(h, c, dtype):
    from sgformer_amd import _lib
    code = _lib.SGF_BF16 if dtype == BF16 else _lib.SGF_F32
    laps = [int(_lib.load().sgf_gat_lap_rows(h, c, code, which)) for which in range(4)]
    assert min(laps) > 0
    return max(math.ceil(2.25 * max(laps)) + 5, 4099)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("h,c", [(8, 64), (1, 64)])
def test_past_the_first_lap(cuda, h, c, dtype):
    """Every output of the forward and of both backward kernels at 2 1/4 laps + 5 rows, degrees 1 - 4, the exact arm's inputs
    (att = 0: every weight is 1 / degree).  dxw, datt, dbias against fp64 autograd of the module's edge-list path; delta, dar,
    dal, which that path has no tensor for, against the closed formulas over the edge list in fp64.  Bit-equal where every
    degree involved is 1, 2 or 4.  A target of degree 3 has p = fl(1/3) (u relative): a sum of k products p x carries
    (k + 2) u sum |terms|; dar = B - A S is then A sl (1 - 3 fl(1/3)) instead of 0: 4 u |A| sl."""
    from sgformer_amd import gat
    n = _lap_n(h, c, dtype)
    ei, graph = ladder_graph([1, 2, 3, 4], cuda, n=n)
    tout = _degrees(graph)[1]
    xw, g, att, bias = _exact_inputs(n, h, c, dtype, True, cuda, seed=2)
    got = run_entries(graph, xw, att, att, bias, g, h, True, SLOPE_EXACT)
    # the module's edge-list path in fp64
    b = [t.double().clone().requires_grad_(True) for t in (xw, att.view(1, h, c), att.view(1, h, c), bias)]
    ref = gat.edge_list_aggregate(ei, n, b[0], b[1], b[2], negative_slope=SLOPE_EXACT, bias=b[3])
    ref.backward(g.double())
    ref = ref.detach()
    # the closed formulas over the edge list
    src, tgt = ei[0], ei[1]
    deg = (graph.rowptr[1:] - graph.rowptr[:-1])
    x3, g3 = xw.double().view(n, h, c), g.double().view(n, h, c)
    p = (1.0 / deg.double())[tgt][:, None]                                        # [E, 1]
    dp = (g3[tgt] * x3[src]).sum(-1)                                              # [E, H]
    zero = torch.zeros((n, h), dtype=F64, device=cuda)
    delta = zero.index_add(0, tgt, p * dp)
    adelta = zero.index_add(0, tgt, p * dp.abs())
    dz = p * (dp - delta[tgt]) * SLOPE_EXACT
    dal = zero.index_add(0, src, dz)
    adal = zero.index_add(0, src, p * (dp.abs() + adelta[tgt]) * SLOPE_EXACT)
    adxw = torch.zeros((n, h, c), dtype=F64, device=cuda).index_add(0, src, p[:, :, None] * g3[tgt].abs()).view(n, h * c)
    odd_t = deg == 3                                                              # targets whose weights are rounded
    odd_s = torch.zeros(n, dtype=F64, device=cuda).index_add(0, src, odd_t[tgt].double()) > 0        # sources that feed one
    assert int(odd_t.sum()) > n // 8 and int((~odd_s).sum()) > n // 8 and int(odd_s.sum()) > n // 8

    def held(name, a, want, exact_rows, tol):
        a, exact = a.double(), want if a.dtype != BF16 else want.to(BF16).double()
        assert torch.equal(a[exact_rows], exact[exact_rows]), f"{name}: not bit-equal on the power-of-two rows"
        allow = tol + (_half_ulp_bf16(want, a) if name in ("out", "dxw") and dtype == BF16 else 0)
        bad = (a - want).abs() > allow
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements off, first row {int(bad.nonzero()[0, 0])}"

    agg = ref - bias.double()
    held("out", got["out"], ref, ~odd_t, _ulp32(agg) + 0.5 * _ulp32(ref) + 4 * 8 * 2.0 ** -53)
    held("delta", got["delta"], delta, ~odd_t, 5 * U * adelta)
    held("dar", got["dar"], torch.zeros_like(delta), ~odd_t, 4 * U * adelta * SLOPE_EXACT)
    held("dal", got["dal"], dal, ~odd_s, (tout + 8) * U * adal)
    held("dxw", got["dxw"], b[0].grad, ~odd_s, (tout + 2) * U * adxw)
    want_lse = torch.log(deg.float())[:, None].expand(n, h)
    assert float(((got["lse"] - want_lse).abs() / _ulp32(want_lse.double()).float()).max()) <= 1.0
    assert float(got["dal"].abs().max()) > 0 and float(got["delta"].abs().max()) > 0 and float(got["dxw"].float().abs().max()) > 0
    # the autograd function on the same launches, and its ATen column sums: datt_l = sum_n dal xw, n terms in fp32:
    # (n + 8) u sum |terms| per element, with dal's own error ahead of it
    a = [t.clone().requires_grad_(True) for t in (xw, att.view(1, h, c), att.view(1, h, c), bias)]
    out = gat.gat_aggregate(graph, a[0], a[1], a[2], negative_slope=SLOPE_EXACT, bias=a[3])
    out.backward(g)
    assert torch.equal(out.detach(), got["out"]) and torch.equal(a[0].grad, got["dxw"])
    assert torch.equal(a[3].grad.double(), b[3].grad)                              # integer column sums
    adatt = torch.einsum("nh,nhc->hc", adal, x3.abs())
    assert float(((a[1].grad.double()[0] - b[1].grad[0]).abs() / ((n + tout + 16) * U * adatt).clamp_min(1e-300)).max()) <= 1.0
    assert float(a[2].grad.abs().max()) <= float((4 * U * adelta * SLOPE_EXACT).sum(0).max() * float(x3.abs().max()))   # dar ~ 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("h,c", [(8, 64), (1, 64)])
def test_scores_past_the_first_lap(cuda, h, c, dtype):
    """sgf_gat_scores at the same row count with integer xw and integer att in [-2, 2]: al and ar are integer sums, bit-equal"""
    from sgformer_amd import gat
    n = _lap_n(h, c, dtype)
    gen = torch.Generator().manual_seed(5)
    xw = torch.randint(-8, 9, (n, h * c), generator=gen).float().to(cuda).to(dtype)
    att_l = torch.randint(-2, 3, (h * c,), generator=gen).float().to(cuda)
    att_r = torch.randint(-2, 3, (h * c,), generator=gen).float().to(cuda)
    al, ar = gat._table().gat_scores(xw, att_l, att_r, h)
    x3 = xw.double().view(n, h, c)
    assert torch.equal(al.double(), (x3 * att_l.double().view(1, h, c)).sum(-1))
    assert torch.equal(ar.double(), (x3 * att_r.double().view(1, h, c)).sum(-1))
    assert float(al.abs().max()) > 0


# ---- module arm -----------------------------------------------------------------------------------------------------------
def _relnorm(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _community_graph(n, device, seed=0):
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (8 * n,), generator=gen)
    dst = (src + torch.randint(-20, 21, (8 * n,), generator=gen)) % n
    return torch.stack([src, dst]).to(device)


# fp32 against fp64 through two or three layers, BatchNorm's division by a batch deviation and ELU: the unit roundoff 6e-8 times
# a few hundred accumulated terms per value; 1e-4 of the norm for the logits and 1e-3 for a gradient are the project's bars for
# a whole fp32 model against fp64 (tests/test_gpu_pair_softmax.py)
MODEL_BAR, MODEL_GRAD_BAR = 1e-4, 1e-3


@pytest.mark.parametrize("layers,use_bn", [(2, False), (2, True), (3, False), (3, True)])
def test_gat_model_against_the_edge_list_path(cuda, layers, use_bn, monkeypatch):
    import copy
    from sgformer_amd import gat
    torch.manual_seed(9)
    n = 2000
    ei = _community_graph(n, cuda)
    model = gat.GAT(48, 16, 7, num_layers=layers, dropout=0.0, use_bn=use_bn, heads=8, out_heads=1).to(cuda)
    model64 = copy.deepcopy(model).double()
    x = torch.randn(n, 48, device=cuda)
    w = torch.randn(n, 7, device=cuda)
    monkeypatch.setenv("SGF_GAT", "1")
    out = model(types.SimpleNamespace(graph={"node_feat": x, "edge_index": ei}))
    (out * w).sum().backward()
    monkeypatch.setenv("SGF_GAT", "0")
    ref = model64(types.SimpleNamespace(graph={"node_feat": x.double(), "edge_index": ei}))
    (ref * w.double()).sum().backward()
    assert out.shape == (n, 7) and _relnorm(out.detach(), ref.detach()) <= MODEL_BAR
    gmax = max(float(p.grad.norm()) for p in model64.parameters() if p.grad is not None)
    for (name, p), q in zip(model.named_parameters(), model64.parameters()):
        if q.grad is None:
            assert p.grad is None, name
            continue
        assert float((p.grad.double() - q.grad).norm()) <= MODEL_GRAD_BAR * (float(q.grad.norm()) + 1e-2 * gmax), name


def test_sgformer_with_a_gat_branch(cuda, monkeypatch):
    """ours_medium.SGFormer(gnn=GAT) with the branch on the kernels against the same model with the branch on the edge-list path
    (fp32 both: the attention branch has no fp64 kernels; the branch alone is held to fp64 above)"""
    from sgformer_amd import gat, ours_medium
    torch.manual_seed(10)
    n, hidden = 2000, 64
    ei = _community_graph(n, cuda, seed=1)
    gnn = gat.GAT(48, hidden // 8, hidden, num_layers=2, dropout=0.0, heads=8, out_heads=1)
    model = ours_medium.SGFormer(48, hidden, 7, num_layers=1, dropout=0.0, use_bn=True, use_graph=True, gnn=gnn).to(cuda)
    data = types.SimpleNamespace(graph={"node_feat": torch.randn(n, 48, device=cuda), "edge_index": ei})
    w = torch.randn(n, 7, device=cuda)
    res = []
    for switch in ("1", "0"):
        monkeypatch.setenv("SGF_GAT", switch)
        model.zero_grad()
        out = model(data)
        (out * w).sum().backward()
        res.append((out.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}))
    (out1, g1), (out0, g0) = res
    assert _relnorm(out1, out0) <= MODEL_BAR and sorted(g1) == sorted(g0) and any(k.startswith("gnn.") for k in g1)
    gmax = max(float(v.norm()) for v in g0.values())
    for k in g0:
        assert float((g1[k].double() - g0[k].double()).norm()) <= MODEL_GRAD_BAR * (float(g0[k].norm()) + 1e-2 * gmax), k
