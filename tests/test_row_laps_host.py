"""GPU-free guards of tests/test_gpu_row_laps.py: under the library's CURRENT launch geometry (sgf_row_lap_rows) its row counts
still give every wave three tiles, an uneven share and a ragged last tile; the input builders meet, at the full N, the
exactness preconditions the bit-exact checks rest on; the restated formulas agree with tests/cpu_kernels.py and
oracle/sgformer_oracle.py; and the checkers reject what a missed `cur = nxt` or one dropped row in the statistics produces."""
import pytest
import torch

from oracle import sgformer_oracle as O
from tests import test_gpu_row_laps as G
from tests.cpu_kernels import CpuKernels as C

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16

# (kind of sgf_row_lap_rows, the widths the GPU file runs it at, its row count)
GEOMETRY = [(0, G.WIDTHS, G.N), (1, G.WIDTHS, G.N), (2, G.WIDTHS, G.N), (3, G.WIDTHS, G.N), (4, G.WIDTHS, G.N),
            (5, sorted({d for _, d in G.STEM}), G.N), (6, sorted({d for d, _ in G.HEAD}), G.N_FWD),
            (7, sorted({d for d, _ in G.HEAD}), G.N)]
BF16_ONLY = (2, 3, 4, 5)     # entries without an fp32 form; the others run other kernels in fp32, which the query does not describe


def _lib():
    from sgformer_amd import _lib
    if not _lib.available():
        pytest.skip("libsgf.so not built (run `make`)")
    return _lib


@pytest.mark.parametrize("kind,widths,n", GEOMETRY, ids=lambda v: None if isinstance(v, list) else str(v))
def test_every_wave_laps_three_times(kind, widths, n):
    """3 * (rows per lap) < N, N mod 32 = 5, and the tiles do not divide evenly over the waves; -1 for what is not supported"""
    L = _lib()
    lib = L.load()
    assert n % 32 == 5
    tiles = -(-n // 32)
    for d in widths:
        lap = lib.sgf_row_lap_rows(kind, d, L.SGF_BF16)
        assert lap > 0 and lap % 32 == 0, (kind, d, lap)
        assert 3 * lap < n, (kind, d, lap)
        waves = lap // 32
        assert tiles // waves >= 3 and tiles % waves != 0, (kind, d, tiles, waves)
    assert lib.sgf_row_lap_rows(kind, 100, L.SGF_BF16) == -1
    assert lib.sgf_row_lap_rows(kind, 0, L.SGF_BF16) == -1 and lib.sgf_row_lap_rows(kind, 512, L.SGF_BF16) == -1
    if kind in BF16_ONLY:
        assert lib.sgf_row_lap_rows(kind, widths[0], L.SGF_F32) == -1
    assert lib.sgf_row_lap_rows(8, 64, L.SGF_BF16) == -1 and lib.sgf_row_lap_rows(-1, 64, L.SGF_BF16) == -1


def test_lap_table_of_the_gpu_file():
    """the table in the GPU file's docstring (and the issue it closes): laps per entry at N"""
    L = _lib()
    lib = L.load()
    q = lambda kind, d: lib.sgf_row_lap_rows(kind, d, L.SGF_BF16)        # noqa: E731
    assert [q(0, d) for d in G.WIDTHS] == [65536] * 3 == [q(5, d) for d in G.WIDTHS] == [q(7, d) for d in G.WIDTHS]
    assert [q(1, d) for d in G.WIDTHS] == [32768] * 3
    assert [q(2, d) for d in G.WIDTHS] == [65536, 65536, 32768] == [q(4, d) for d in G.WIDTHS]
    assert [q(3, d) for d in G.WIDTHS] == [65536, 32768, 16384]
    assert [q(6, d) for d in G.WIDTHS] == [131072] * 3
    assert G.N // q(3, 256) == 12 and G.N // q(1, 256) == 6


def test_cases_cover_what_the_issue_names():
    assert G.WIDTHS == [64, 128, 256]
    assert {f for f, _ in G.STEM} == {100, 128} and {d for _, d in G.STEM} == {64, 256}
    assert {c for _, c in G.HEAD} == {47, 64, 7} and {d for d, _ in G.HEAD} == {64, 128, 256}
    assert G.HEAD_AB == [(0.5, 0.5), (0.75, 0.25)]
    assert sum(G.ADD_GY) == 2
    assert G.N == 3 * 65536 + 5 and G.N_FWD == 3 * 131072 + 5


def _bf16_exact(t):
    return torch.equal(t.bfloat16().float(), t.float())


@pytest.mark.parametrize("d", G.WIDTHS)
def test_rowgemm_builders_meet_their_preconditions(d):
    """At the full N.  The matrix products run in fp32 here: their operands are integers with abs-sums of at most 2 d * 3 * 2,
    so every fp32 result is the exact one (the GPU file forms the same values in fp64)."""
    c = G.get_case(d)
    n = G.N
    assert c.n == n and c.a.shape == (n, 2 * d) and c.g.shape == (n, 2 * d) and c.ai.shape == (n, d)
    assert set(c.a.unique().tolist()) == {-1, 0, 1} and set(c.ai.unique().tolist()) == {-1, 0, 1}
    assert set(c.g.unique().tolist()) == {-2, -1, 0, 1, 2}
    assert abs(float((c.a != 0).float().mean()) - 0.25) < 0.01 and abs(float((c.ai != 0).float().mean()) - 0.5) < 0.01
    assert set(c.ws.unique().tolist()) == {-1.0, 0.0, 1.0} and abs(float((c.ws != 0).float().mean()) - 0.25) < 0.03
    assert float(c.wd.abs().max()) == 3.0 and float(c.wg.abs().max()) == 31.0
    assert float(c.bias.abs().max()) <= 2.0 and float(c.shift.abs().max()) <= 1.0
    for t in (c.ws, c.wd, c.wg, c.bias, c.shift):
        assert _bf16_exact(t) and torch.equal(t.round(), t)
    # ---- the statistics: y an integer and a bf16 value, sum |y - shift| and sum (y - shift)^2 below 2^24 in every column ----
    a1, a2 = c.a[:, :d].float(), c.a[:, d:].float()
    p1, p2 = a1 @ c.ws[:, :d].T, a2 @ c.ws[:, d:].T
    for name, y in (("stats", p1 + c.bias), ("stats, no bias", p1), ("two-pass", p2 + G.rnd(p1 + c.bias)), ("cat", p1 + p2 + c.bias)):
        assert torch.equal(G.rnd(y), y), name
        worst = G.stats_abs_sum(y, c.shift)
        assert 0 < worst < G.EXACT, (name, worst)
    assert torch.equal(G.ref_two_pass(a1, a2, c.ws, c.bias), p2 + G.rnd(p1 + c.bias))
    assert torch.equal(G.ref_cat(a1, a2, c.ws, c.bias), p1 + p2 + c.bias)
    # ---- the gradient forms: |dy W| <= 2 * 31 * d, far below 2^24; many values need rounding (more than 8 significant bits) ----
    assert 2 * 31 * d + 2 + 1 < G.EXACT
    dx = c.g[:4096, :d].float() @ c.wg[:, :d]
    assert int((G.rnd(dx) != dx).sum()) > 4096, "the rounding of dx should be a real one"
    # ---- sgf_gcn_bn_bwd_dx: constants as the docstring of bn_coefs says, dz a multiple of 1/512 below 16 ----
    # (gy, z) take 25 value pairs (asserted above), the constants are per column: the 25 x d grid is every element there is
    v = torch.arange(-2, 3, dtype=F64)
    gy, z = v.repeat_interleave(5)[:, None].expand(25, d), v.repeat(5)[:, None].expand(25, d)
    worst, rounded = 0.0, 0
    for k in c.bn:
        assert set(k["rstd"].tolist()) <= {0.5, 1.0} and set(k["gamma"].tolist()) <= {0.5, 1.0, 2.0}
        for name, q in (("mean", 4), ("beta", 2)):
            assert torch.equal((q * k[name]).round(), q * k[name]) and float(k[name].abs().max()) <= 1.0
        k0, k1 = k["stats"][:d].double() * G.INV_N, k["stats"][d:].double() * G.INV_N
        assert torch.equal((4 * k0).round(), 4 * k0) and float(k0.abs().max()) <= 1.0
        assert torch.equal((16 * k1).round(), 16 * k1) and float(k1.abs().max()) <= 0.5
        for t in k.values():
            assert _bf16_exact(t)
        # the prologue's coefficients in fp32, in its order of operations, against fp64: no rounding anywhere
        rs, ga = k["rstd"], k["gamma"]
        m = -k["mean"] * rs
        k0f, k1f = k["stats"][:d] * F32_INV_N, k["stats"][d:] * F32_INV_N
        cs = ga * rs
        coefs32 = (rs * ga, m * ga + k["beta"], -cs * k1f * rs, -cs * (k0f + k1f * m))
        m64 = -k["mean"].double() * rs.double()
        coefs64 = (rs.double() * ga.double(), m64 * ga.double() + k["beta"].double(), -cs.double() * k1 * rs.double(),
                   -cs.double() * (k0 + k1 * m64))
        for c32, c64 in zip(coefs32, coefs64):
            assert torch.equal(c32.double(), c64)
        for relu in (True, False):
            for training in (True, False):
                dz = G.ref_bn_bwd(gy, z, k, relu, training)
                assert torch.equal((G.DZ_UNITS * dz).round(), G.DZ_UNITS * dz)
                assert torch.equal(dz.float().double(), dz)
                worst = max(worst, float(dz.abs().max()))
                rounded += int((G.rnd(dz) != dz).sum())
    assert rounded > 25, "the rounding of dz should be a real one"
    # the dz W sums and the running sum over three calls, in units of 1/512: max |dz| * 3 * d per product, + |gy|, three times
    # (a bound from the largest |dz| of the data; the GPU file asserts the abs-sums themselves)
    assert worst < 16.0 and G.DZ_UNITS * 3 * (worst * 3 * d + 2) < G.EXACT, worst


F32_INV_N = torch.tensor(G.INV_N, dtype=F32)


@pytest.mark.parametrize("f,d", G.STEM)
def test_stem_builders_meet_their_preconditions(f, d):
    c = G.build_stem(f, d)
    assert c.x.shape == (G.N, f) and set(c.x.unique().tolist()) == {-1, 0, 1}
    assert abs(float((c.x != 0).float().mean()) - 0.25) < 0.01
    for t in (c.w0, c.w1, c.b0, c.b1, c.shift):
        assert _bf16_exact(t) and torch.equal(t.round(), t)
    y0 = c.x.float() @ c.w0.T + c.b0
    assert torch.equal(G.rnd(y0), y0)
    assert 0 < G.stats_abs_sum(y0, c.shift) < G.EXACT


@pytest.mark.parametrize("d,classes", G.HEAD)
def test_head_builders_meet_their_preconditions(d, classes):
    c = G.build_head(d, classes)
    assert c.x.shape == (G.N_FWD, 2 * d) and c.dl.shape == (G.N, classes)
    assert set(c.x.unique().tolist()) == {-2, -1, 0, 1, 2} == set(c.dl.unique().tolist())
    for t in (c.w, c.bias):
        assert _bf16_exact(t) and torch.equal(t.round(), t)
    assert float(c.w.abs().max()) == 3.0
    for n, m in ((G.N_FWD, c.map_fwd), (G.N, c.map_bwd)):
        assert m.dtype == torch.int32 and torch.equal(m.long().sort().values, torch.arange(n))
        assert not torch.equal(m.long(), torch.arange(n))
    x1, x2 = c.x[:65536, :d].double(), c.x[:65536, d:].double()
    for a, b in G.HEAD_AB:
        assert a + b == 1.0
        xc = a * x1 + b * x2
        assert torch.equal(G.rnd(xc), xc), "a x1 + b x2 must be a bf16 value"
        # logits: multiples of 1/4, |sum| <= 2 * 3 * d + 4;  g W: integers up to 2 * 3 * classes, a (g W) multiples of 1/4
        assert 4 * (2 * 3 * d + 4) < G.EXACT and 4 * 2 * 3 * classes < G.EXACT
        r1, _ = G.ref_head_bwd(c.dl[:65536].double(), c.w.double(), a, b)
        assert torch.equal(r1.float().double(), r1)
        if a == 0.75 and classes >= 47:
            assert int((G.rnd(r1) != r1).sum()) > 0, "no dx1 value needs rounding"


# ------------------------------------------------------------------------------------------------------------------------------
# the restated formulas against tests/cpu_kernels.py (integer operands: its fp32 arithmetic is exact too) and the oracle
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_references_agree_with_the_cpu_kernels(d):
    n = 4099
    c = G.build_case(d, n)
    a1, a2, g1, g2, ai = (t.to(BF16) for t in (c.a[:, :d], c.a[:, d:], c.g[:, :d], c.g[:, d:], c.ai))
    ws, wd, wg = c.ws.to(BF16), c.wd.to(BF16), c.wg.to(BF16)
    D = lambda t: t.double()                                          # noqa: E731
    y, st = C.gcn_epilogue_stats(a1, ws[:, :d], c.bias, c.shift, True)
    ref = G.ref_linear(D(a1), D(ws[:, :d]), D(c.bias))
    assert torch.equal(G.rnd(ref).to(BF16), y) and torch.equal(G.ref_stats(ref, D(c.shift)).float(), st)
    y, st = C.gcn_epilogue_cat(a1, a2, ws, c.bias, c.shift, True)     # (the CPU stand-in rounds the first product: two-pass)
    ref = G.ref_two_pass(D(a1), D(a2), D(ws), D(c.bias))
    assert torch.equal(G.rnd(ref).to(BF16), y) and torch.equal(G.ref_stats(ref, D(c.shift)).float(), st)
    assert torch.equal(G.rnd(G.ref_cat(D(a1), D(a2), D(ws), D(c.bias))).to(BF16), y)     # integers: one rounding or two
    assert torch.equal(G.rnd(G.ref_dx(D(g1), D(wg[:, :d]))).to(BF16), C.gcn_epilogue_dx(g1, wg[:, :d]))
    for gadd, acc_in in ((None, None), (g2, None), (None, ai), (g2, ai)):
        dy, acc = C.gcn_epilogue_dx2_acc(g1, wg, gadd, acc_in)
        r_dy, r_acc = G.ref_dx2_acc(D(g1), D(wg), None if gadd is None else D(gadd), None if acc_in is None else D(acc_in))
        assert torch.equal(G.rnd(r_dy).to(BF16), dy) and torch.equal(G.rnd(r_acc).to(BF16), acc)
    for relu in (True, False):
        for training in (True, False):
            refs = G.ref_bn_chain(D(g1), D(g2), D(wd), c.bn, relu, training, G.ADD_GY)
            acc = None
            for i, (k, add) in enumerate(zip(c.bn, G.ADD_GY)):
                dz, dy, acc = C.gcn_bn_bwd_dx(g1, g2, k["mean"], k["rstd"], k["gamma"], k["beta"], relu, k["stats"], G.INV_N,
                                              training, wd, acc, i == 2, add)
                for got, want in zip((dz, dy, acc), refs[i]):
                    assert torch.equal(G.rnd(want).to(BF16), got), (relu, training, i)


def test_stem_and_head_references_agree_with_the_cpu_kernels():
    s = G.build_stem(100, 64, 4099)
    x, w0, w1 = s.x.to(BF16), s.w0.to(BF16), s.w1.to(BF16)
    y0, y1, st = C.stem_pair(x, w0, s.b0, w1, s.b1, s.shift, True)
    r0 = G.ref_linear(x.double(), w0.double(), s.b0.double())
    assert torch.equal(G.rnd(r0).to(BF16), y0) and torch.equal(G.ref_stats(r0, s.shift.double()).float(), st)
    assert torch.equal(G.rnd(G.ref_linear(x.double(), w1.double(), s.b1.double())).to(BF16), y1)
    h = G.build_head(64, 47, 4099, 4099)
    x1, x2, dl = h.x[:, :64].to(BF16), h.x[:, 64:].to(BF16), h.dl.float()
    for a, b in G.HEAD_AB:
        for rmap in (None, h.map_fwd):
            ref, _ = G.ref_head_fwd(x1.double(), a, x2.double(), b, h.w.double(), h.bias.double())
            if rmap is not None:
                out = torch.empty_like(ref)
                out[rmap.long()] = ref
                ref = out
            assert torch.equal(ref.float(), C.combine_fc_fwd(x1, a, x2, b, h.w, h.bias, rmap))
        for rmap in (None, h.map_bwd):
            g = dl if rmap is None else dl[rmap.long()]
            r1, r2 = G.ref_head_bwd(g.double(), h.w.double(), a, b)
            d1, d2 = C.combine_fc_bwd(dl, h.w, a, b, BF16, rmap)
            assert torch.equal(G.rnd(r1).to(BF16), d1) and torch.equal(G.rnd(r2).to(BF16), d2)


def _close(a, b, tol=1e-11):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * float(b.abs().max()), float((a - b).abs().max())


def test_references_agree_with_the_oracle():
    """ref_linear / ref_cat = the oracle's Linear (of the concatenation); ref_bn_bwd = autograd through the oracle's training
    BatchNorm + ReLU; the chain's products = autograd through the Linear; the head = the oracle's combine + fc."""
    n, d = 2053, 16
    gen = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F64)          # noqa: E731
    a1, a2, w, b = r(n, d), r(n, d), r(d, 2 * d), r(d)
    p = {"W.weight": w, "W.bias": b, "W1.weight": w[:, :d], "W1.bias": b}
    _close(G.ref_cat(a1, a2, w, b), O._linear(p, "W", torch.cat([a1, a2], 1)))
    _close(G.ref_linear(a1, w[:, :d], b), O._linear(p, "W1", a1))
    shift = r(d)
    y = G.rnd(G.ref_linear(a1, w[:, :d], b))
    _close(G.ref_stats(y, shift), torch.cat([(y - shift).sum(0), ((y - shift) ** 2).sum(0)]))
    # BatchNorm + ReLU backward
    z, gy = r(n, d).requires_grad_(True), r(n, d)
    bn = {"bn.weight": r(d), "bn.bias": r(d)}
    out = torch.relu(O._batch_norm(bn, "bn", z, True, None))
    gz, = torch.autograd.grad((out * gy).sum(), z)
    zd = z.detach()
    mean, var = zd.mean(0), ((zd - zd.mean(0)) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    xh = (zd - mean) * rstd
    gp = gy * ((xh * bn["bn.weight"] + bn["bn.bias"]) > 0)
    k = {"mean": mean, "rstd": rstd, "gamma": bn["bn.weight"], "beta": bn["bn.bias"],
         "stats": torch.cat([gp.sum(0), (gp * xh).sum(0)])}
    _close(G.ref_bn_bwd(gy, zd, k, True, True, 1.0 / n), gz, 1e-9)
    # both input gradients of the two-operand Linear
    x1, x2 = r(n, d).requires_grad_(True), r(n, d).requires_grad_(True)
    dzz = r(n, d)
    g1, g2 = torch.autograd.grad((O._linear(p, "W", torch.cat([x1, x2], 1)) * dzz).sum(), (x1, x2))
    _close(G.ref_dx(dzz, w[:, :d]), g1)
    _close(G.ref_dx(dzz, w[:, d:]), g2)
    # head: x = gw x2 + (1 - gw) x1;  logits = fc(x)
    c, gw = 7, 0.75
    fc = {"fc.weight": r(c, d), "fc.bias": r(c)}
    x1, x2 = G.rnd(r(n, d)).requires_grad_(True), G.rnd(r(n, d)).requires_grad_(True)
    logits = O._linear(fc, "fc", gw * x2 + (1 - gw) * x1)
    ref, _ = G.ref_head_fwd(x1.detach(), 1 - gw, x2.detach(), gw, fc["fc.weight"], fc["fc.bias"])
    _close(ref, logits.detach(), 2.0 ** -7)                           # (the combined row is rounded to bf16 once)
    dl = r(n, c)
    h1, h2 = torch.autograd.grad((logits * dl).sum(), (x1, x2))
    r1, r2 = G.ref_head_bwd(dl, fc["fc.weight"], 1 - gw, gw)
    _close(r1, h1)
    _close(r2, h2)


# ------------------------------------------------------------------------------------------------------------------------------
# sensitivity: the checkers see what a broken hand-over produces
# ------------------------------------------------------------------------------------------------------------------------------
def test_checkers_reject_a_stale_tile_and_a_dropped_row():
    """A missed `cur = nxt` makes a wave multiply its FIRST tile again on its second lap: 32 rows among 196 613 take the
    values of 32 others.  One row left out of the column statistics changes a sum by a small integer."""
    d, lap = 64, 65536
    c = G.get_case(d)
    y = c.a[:, :d].float() @ c.ws[:, :d].T + c.bias                    # exact (integers), as the builders test shows
    good = y.bfloat16()
    G.check_bf16("y", good, y.double())
    wave = 1234
    first, second = G.wave_tile_rows(lap, wave, 0, G.N), G.wave_tile_rows(lap, wave, 1, G.N)
    assert second.start == 32 * (wave + lap // 32) and second.stop - second.start == 32
    stale = good.clone()
    stale[second] = good[first]
    with pytest.raises(AssertionError, match="differ from the exact result"):
        G.check_bf16("y", stale, y.double())
    # the last wave's fourth tile is the ragged one
    last = G.wave_tile_rows(lap, 0, 3, G.N)
    assert last.stop - last.start == 5 and last.stop == G.N
    stats = G.ref_stats(y.double(), c.shift.double())
    G.check_exact("stats", stats.float(), stats)
    row = second.start + 7
    assert bool((y[row] - c.shift != 0).any())
    kept = torch.cat([y[:row], y[row + 1:]]).double()
    with pytest.raises(AssertionError, match="differ from the exact result"):
        G.check_exact("stats", G.ref_stats(kept, c.shift.double()).float(), stats)
    doubled = torch.cat([y, y[row:row + 1]]).double()
    with pytest.raises(AssertionError, match="differ from the exact result"):
        G.check_exact("stats", G.ref_stats(doubled, c.shift.double()).float(), stats)
