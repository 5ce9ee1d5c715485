"""GPU-free guards of tests/test_gpu_attn_laps.py: the row count still gives every workgroup three tiles and a ragged last one
under the library's CURRENT tile heights and grid cap (sgf_attn_tile_rows / sgf_attn_max_blocks), the input builders meet the
exactness preconditions the bit-exact checks rest on, and the restated fp64 formulas agree with oracle/sgformer_oracle.py."""
import pytest
import torch

from oracle import sgformer_oracle as O
from tests import test_gpu_attn_laps as G

F64 = torch.float64


def _lib():
    from sgformer_amd import _lib
    if not _lib.available():
        pytest.skip("libsgf.so not built (run `make`)")
    return _lib


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("dtype", ["SGF_F32", "SGF_BF16"])
def test_every_workgroup_laps_three_times(kind, dtype):
    """For every (kernel family, width, storage type) the GPU file runs: 3 * blocks * rows per tile < N (the buffer index of every
    workgroup goes 0 -> 1 -> 0), the tiles do not divide evenly over the workgroups, and the last tile is ragged (five rows)."""
    L = _lib()
    lib, code = L.load(), getattr(L, dtype)
    nb = lib.sgf_attn_max_blocks()
    assert 1 <= nb <= 256
    assert lib.sgf_attn_tile_rows(2, 64, code) == -1 and lib.sgf_attn_tile_rows(kind, 260, code) == -1
    for d in sorted({c[1] for c in G.CASES}):
        r = lib.sgf_attn_tile_rows(kind, d, code)
        assert 1 <= r <= 256, (d, r)
        assert r == lib.sgf_attn_tile_rows(kind, G.padded(d), code), "the kernels pad d as the GPU file assumes"
        if G.padded(d) > 64:
            assert r != lib.sgf_attn_tile_rows(kind, G.padded(d) // 2, code), "a width of its own, not the next smaller one's"
        assert 3 * nb * r < G.N, (d, r, nb)
        assert G.N % r == 5, (d, r)
        tiles = -(-G.N // r)
        assert tiles // nb >= 3 and tiles % nb != 0, (d, r, tiles)


def test_widths_cover_every_padded_dim():
    assert {G.padded(c[1]) for c in G.CASES} == {64, 128, 256}
    assert any(c[1] != G.padded(c[1]) for c in G.CASES), "one case with padded columns"
    assert {(c[0], c[2]) for c in G.CASES} >= {(1, 1), (2, 2), (2, 1)}
    # the shared module-scoped instances: the H = 1 cases are a prefix
    assert [p.values for p in G.H1] == [p.values for p in G.ALL[:len(G.H1)]]


@pytest.mark.parametrize("H,d", sorted({c[:2] for c in G.CASES}))
def test_builders_meet_their_exactness_preconditions(H, d):
    """At the full N: value sets, powers of two where the checks rely on them, bf16-exact matrices, and every worst-case abs-sum
    (in units of the operands' quantum) below 2^24 - so that any summation order gives the fp64 result in fp32."""
    c = G.get_case(H, d)
    hd = H * d
    assert c.n == G.N and c.qkv.shape == (G.N, 3 * hd) and c.go.shape == (G.N, 2 * hd)
    assert int(c.qkv[:, :hd].abs().max()) == 1 and int(c.qkv[:, hd:].abs().max()) == 2 and int(c.go.abs().max()) == 1
    assert abs(float((c.qkv[:, :hd] != 0).float().mean()) - 0.5) < 0.01
    assert abs(float((c.go != 0).float().mean()) - 0.25) < 0.01
    assert set(c.den.unique().tolist()) == {1.0, 2.0, 4.0}
    for name, v in c.pre.items():
        assert 0 < v < G.EXACT, (name, v)
    # c = 1 / (sqrt(ssq_q) sqrt(ssq_k)) is a power of two, the ssq powers of four; |c q.z0| <= 2 < NTOT
    for s in (c.ssq_q, c.ssq_k):
        e = torch.log2(torch.tensor(s, dtype=F64)).item()
        assert e == round(e) and round(e) % 2 == 0, s
    assert c.c == 2.0 / c.DP and c.c * d <= 2.0 < G.NTOT
    assert float(c.stats_in[-2]) == c.ssq_q and float(c.stats_in[-1]) == c.ssq_k and float(c.bstats_in[-1]) == 0.0
    for t in (c.stats_in[:-2], c.bstats_in, c.hM, c.hm, c.hw, c.hD, c.hds, c.hbeta):
        assert torch.equal(t.bfloat16().float(), t) and torch.equal(t.round(), t)
    assert float(c.hbeta) >= d + 4 + 2                        # den = h.w + beta >= 2 for |h.w| <= d + 4
    # the matrix term shows in every row pass's output (the GPU file asserts it again on all rows)
    n = 16384
    q, k, v = (c.qkv[:n, i * hd:(i + 1) * hd].double() for i in range(3))
    g, o, den = c.go[:n, :hd].double(), c.go[:n, hd:].double(), c.den[:n].double()
    st, bst = c.stats_in.double(), c.bstats_in.double()
    for vh in {1, H}:
        vv = v[:, :vh * d]
        _, r_den, r_o, _, pair = G.ref_fwd_apply(q, vv, st, G.NTOT, H, vh, d)
        assert float(r_den.min()) >= 2.0 and float(r_den.max()) <= 6.0
        G.check_visible("o_heads", pair, r_o)
        for per_head in (False, True):
            _, res = G.ref_bwd_apply(q, k, vv, g if per_head else g[:, :d], o, den, st, bst, G.NTOT, H, vh, d, per_head)
            for name, (r, _, pair, _) in res.items():
                G.check_visible(name, pair, r)
    if H == 1:
        r, r_den, _, pair = G.ref_h_fwd(q, c.hM.double(), c.hm.double(), c.hw.double(), c.hbeta.double())
        G.check_visible("h out", pair, r)
        assert float(r_den.min()) >= 2.0
        r, _, pair, _ = G.ref_h_bwd_apply(q, g, o, den, c.hM.double(), c.hw.double(), c.hD.double(), c.hds.double())
        G.check_visible("dh", pair, r)


def _close(a, b, tol=1e-11):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * float(b.abs().max()), float((a - b).abs().max())


@pytest.mark.parametrize("H,d,vh", [(1, 8, 1), (2, 8, 2), (3, 4, 1)])
def test_references_agree_with_the_oracle(H, d, vh):
    """ref_fwd_reduce -> ref_fwd_apply composed = oracle attention; ref_bwd_reduce -> ref_bwd_apply = autograd through it, for
    the head-mean cotangent and for per-head cotangents."""
    n = 37
    gen = torch.Generator().manual_seed(H * 10 + d)
    q, k = torch.randn(n, H * d, generator=gen, dtype=F64), torch.randn(n, H * d, generator=gen, dtype=F64)
    v = torch.randn(n, vh * d, generator=gen, dtype=F64)
    q3, k3, v3 = (t.reshape(n, -1, d).clone().requires_grad_(True) for t in (q, k, v))
    want, parts = O.attention(q3, k3, v3, return_parts=True)
    stats = G.ref_fwd_reduce(q, k, v, H, vh, d)
    _close(stats, O.attention_raw_stats(q3, k3, v3).detach())
    out, den, o, tabs, pair = G.ref_fwd_apply(q, v, stats, float(n), H, vh, d)
    _close(out, want.detach())
    _close(o, parts["o"].detach().reshape(n, H * d))
    _close(den, parts["den"].detach().reshape(n, H))
    assert bool((tabs >= o.abs() - 1e-12).all())
    for per_head in (False, True):
        g = torch.randn(n, H * d if per_head else d, generator=gen, dtype=F64)
        target = parts["o"].reshape(n, H * d) if per_head else want
        gq, gk, gv = torch.autograd.grad((target * g).sum(), (q3, k3, v3), retain_graph=True)
        bstats, _, _ = G.ref_bwd_reduce(q, g, o, den, H, d, per_head)
        sdot, res = G.ref_bwd_apply(q, k, v, g, o, den, stats, bstats, float(n), H, vh, d, per_head)
        _close(res["dq"][0], gq.reshape(n, -1), 1e-9)
        _close(res["dk"][0], gk.reshape(n, -1), 1e-9)
        _close(res["dv"][0], gv.reshape(n, -1), 1e-9)
        for name in res:
            assert bool((res[name][1] >= res[name][0].abs() - 1e-12).all())


def test_h_references_agree_with_the_oracle():
    """The h form with identity projections is the oracle's attention of (h, h, h); its backward references are autograd through
    out = (h M + m) / (h.w + beta) plus the affine h D + ds."""
    n, d = 41, 8
    gen = torch.Generator().manual_seed(5)
    h = torch.randn(n, d, generator=gen, dtype=F64)
    h3 = h.reshape(n, 1, d)
    stats = O.attention_raw_stats(h3, h3, h3)
    S0, z0 = stats[:d * d].reshape(d, d), stats[d * d:d * d + d]
    c = 1.0 / (stats[-2].sqrt() * stats[-1].sqrt())
    M, m, w, beta = c * S0 + n * torch.eye(d, dtype=F64), torch.zeros(d, dtype=F64), c * z0, torch.tensor([float(n)], dtype=F64)
    out, den, tabs, _ = G.ref_h_fwd(h, M, m, w, beta)
    _close(out, O.attention(h3, h3, h3))
    # backward: arbitrary constants, autograd through the row formula
    M, m, w = (torch.randn(s, generator=gen, dtype=F64).requires_grad_(True) for s in ((d, d), (d,), (d,)))
    beta = torch.tensor([9.0], dtype=F64, requires_grad=True)
    hh = h.clone().requires_grad_(True)
    out = (hh @ M + m) / (hh @ w + beta)[:, None]
    g = torch.randn(n, d, generator=gen, dtype=F64)
    gh, gM, gm, gw, gb = torch.autograd.grad((out * g).sum(), (hh, M, m, w, beta))
    o, den = out.detach(), (h @ w + beta).detach().reshape(n, 1)
    _close(G.ref_h_fwd(h, M.detach(), m.detach(), w.detach(), beta.detach())[0], o)
    _close(G.ref_h_bwd_reduce(h, g, o, den), torch.cat([gM.reshape(-1), gw, gm, gb]), 1e-9)
    D, ds = torch.randn(d, d, generator=gen, dtype=F64), torch.randn(d, generator=gen, dtype=F64)
    dh, tabs, _, first = G.ref_h_bwd_apply(h, g, o, den, M.detach(), w.detach(), D, ds)
    _close(dh, gh + h @ D + ds, 1e-9)
    _close(first, gh, 1e-9)
    assert bool((tabs >= dh.abs() - 1e-12).all())
