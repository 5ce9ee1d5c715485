"""GPU-free guards of tests/test_gpu_ew_laps.py: under the library's CURRENT launch geometry (sgf_ew_lap_rows) its row counts
still give every workgroup two full iterations, a quarter of them a third and a ragged end; the lap table of the GPU file
holds; the input builders meet, at the full N, the exactness preconditions the bit-exact checks rest on; the restated
formulas (and the integer Philox) agree with tests/cpu_kernels.py, with known-answer vectors and with
oracle/sgformer_oracle.py; and the checkers reject a stale lap, a dropped row in a statistic, a row normalised twice and one
flipped keep bit.  (tests/cpu_kernels_dropout.py draws its keep pattern from torch.rand, not from Philox: the dropout VALUES are
compared with it under a given pattern, the pattern itself with the published Philox4x32-10 vectors.)"""
import pytest
import torch

from oracle import sgformer_oracle as O
from tests import test_gpu_ew_laps as G
from tests.cpu_kernels import CpuKernels as C
from tests.cpu_kernels_dropout import CpuKernelsDropout

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
GRID = 2048          # the grid cap every lap below is a multiple of (flat kernels: 2048 * 256 chunks)


def _lib():
    from sgformer_amd import _lib
    if not _lib.available():
        pytest.skip("libsgf.so not built (run `make`)")
    return _lib


def _q(kind, d, dtype, wide):
    L = _lib()
    return L.load().sgf_ew_lap_rows(kind, d, L.SGF_BF16 if dtype == BF16 else L.SGF_F32, int(wide))


def _geometry():
    """every (kind, d, dtype, wide) the GPU file runs a grid-stride kernel at"""
    out = set()

    def add(kind, cases, has_wide, reads_env=True):
        for case in cases:
            d, path = case[0], case[1]
            out.add((kind, d, G.PATHS[path][0], G.runs_wide(path, d, has_wide, reads_env)))

    add(G.K_AXPBY, G.AXPBY_CASES, G.no_wide)
    add(G.K_SUM_N, G.SUM_CASES, G.ew8_width, reads_env=False)
    add(G.K_DROPOUT, G.DROP_CASES, G.no_wide)
    for cases in (G.LN_PLAIN_CASES, G.LN_CASES, [(d, p) for d in G.LN_WIDE_WIDTHS for p in ("bf16", "bf16_ld4")]):
        add(G.K_LN_FWD, cases, G.ln8_width, reads_env=False)
        add(G.K_LN_BWD, cases, G.ln8_width)
    add(G.K_BN_APPLY, G.BN_APPLY_CASES, G.ew8_width)
    add(G.K_BN_BWD_APPLY, G.BN_BWD_CASES, G.ew8_width)
    out |= {(G.K_GATHER, d, G.PATHS[s][0], False) for d, s, _t, _i in G.GATHER_CASES}
    out |= {(G.K_PAD, dp, G.PATHS[s][0], False) for _d, dp, s, _t, _i in G.PAD_CASES}
    out |= {(G.K_NLL_BWD, c, dt, False) for c in G.NLL_CLASSES for dt in (F32, BF16)}
    return sorted(out, key=lambda t: (t[0], t[1], str(t[2]), t[3]))


FLAT = (G.K_AXPBY, G.K_SUM_N, G.K_DROPOUT, G.K_GATHER, G.K_PAD)


@pytest.mark.parametrize("kind,d,dtype,wide", _geometry(), ids=G._ids)
def test_every_workgroup_iterates_twice_and_some_a_third_time(kind, d, dtype, wide):
    lap = _q(kind, d, dtype, wide)
    assert lap > 0, (kind, d, dtype, wide)
    n = G.rows_at(lap)
    assert n == 2 * lap + lap // 4 + 5 and 2 * lap < n < 3 * lap
    if kind in FLAT:
        per_row = (d // 8 if wide else d // 4) if (d % 4 == 0 and kind != G.K_PAD) else d
        chunks = GRID * 256
        assert lap == chunks // per_row, (lap, per_row)
        total = n * per_row
        assert total // chunks == 2 and total % 256 != 0            # two full iterations, a third, and a partly filled workgroup
        first_idle = -(-(total - 2 * chunks) // 256)
        assert GRID // 8 < first_idle < GRID // 2                   # about a quarter of the workgroups run the third iteration
    else:
        assert lap % GRID == 0
        block = lap // GRID                                         # rows of one workgroup in one iteration
        assert (n - 2 * lap) % block != 0, "the last group of rows must be ragged"
        busy = -(-(n - 2 * lap) // block)
        assert GRID // 8 < busy < GRID // 2
        if kind in (G.K_BN_APPLY, G.K_BN_BWD_APPLY) and not wide:
            # the four unrolled rows of k_bn_apply / k_bn_bwd_apply are lap / 4 apart: in the third iteration u = 0 is in range
            # for every workgroup, u = 1 for five rows, u = 2 and 3 for none
            assert n - 2 * lap - lap // 4 == 5


def test_lap_table_of_the_gpu_file():
    """the table in the GPU file's docstring (and the issue it closes), from the query"""
    for kind in (G.K_LN_FWD, G.K_LN_BWD):
        for dt in (F32, BF16):
            assert [_q(kind, d, dt, 0) for d in (64, 100, 128, 256, 512, 768, 1024)] == [32768, 16384, 16384, 8192, 8192, 8192, 8192]
        assert [_q(kind, d, BF16, 1) for d in (64, 128, 256, 512)] == [262144, 131072, 65536, 32768]
    for kind in (G.K_BN_APPLY, G.K_BN_BWD_APPLY):
        for dt in (F32, BF16):
            assert [_q(kind, d, dt, 0) for d in (64, 100, 128, 256, 512)] == [131072, 81920, 65536, 32768, 16384]
        assert [_q(kind, d, BF16, 1) for d in (64, 104, 128, 256, 512)] == [262144, 155648, 131072, 65536, 32768]
    for kind in (G.K_AXPBY, G.K_SUM_N, G.K_DROPOUT, G.K_GATHER):
        for dt in (F32, BF16):
            assert [_q(kind, d, dt, 0) for d in (64, 100, 128, 256, 512)] == [32768, 20971, 16384, 8192, 4096]
    assert 524288 * 4 // 100 == 20971 and (524288 * 4) % 100 != 0               # d = 100: the lap ends inside a row
    assert [_q(G.K_SUM_N, d, BF16, 1) for d in (64, 128, 256, 512)] == [65536, 32768, 16384, 8192]
    assert _q(G.K_GATHER, 65, F32, 0) == 524288 // 65
    assert [_q(G.K_PAD, d, F32, 0) for d in (68, 104)] == [7710, 5041]
    assert [_q(G.K_NLL_BWD, c, dt, 0) for c in (47, 64, 65, 172) for dt in (F32, BF16)] == [32768] * 4 + [8192] * 4
    # the blocked reductions: the row count at which the grid stops growing
    assert [_q(G.K_COLSTATS, d, dt, 0) for d in (64, 100, 512) for dt in (F32, BF16)] == [G.STAT_CAP] * 6
    assert _q(G.K_COLSTATS, 256, BF16, 1) == G.STAT_CAP == _q(G.K_COLSUM, 47, F32, 0) == _q(G.K_COLSUM, 256, BF16, 0)
    assert _q(G.K_NLL_FWD, 47, F32, 0) == G.NLL_CAP == _q(G.K_NLL_FWD, 172, BF16, 0)
    for cap, rows in ((G.STAT_CAP, G.STAT_ROWS), (G.NLL_CAP, G.NLL_FWD_ROWS)):
        assert rows == [cap + 1, 2 * cap + 5]
        blocks, per = cap // 64, -(-rows[0] // (cap // 64))
        assert per == 65 and -(-rows[0] // per) < blocks, "n = cap + 1 must leave trailing workgroups without rows"


def test_unsupported_combinations_return_minus_one():
    L = _lib()
    q = L.load().sgf_ew_lap_rows
    f32, bf16 = L.SGF_F32, L.SGF_BF16
    assert q(-1, 64, f32, 0) == -1 and q(13, 64, f32, 0) == -1                 # unknown kind
    for kind in range(13):
        assert q(kind, 64, 2, 0) == -1 and q(kind, 64, -1, 0) == -1            # SGF_F32_BF16X3 and an unknown dtype
        assert q(kind, 0, f32, 0) == -1 and q(kind, -4, bf16, 0) == -1
        assert q(kind, 64, f32, 1) == -1 and q(kind, 64, bf16, 2) == -1        # no 16-byte kernel in fp32; wide is 0 or 1
    for kind in (0, 1, 2, 3, 4, 5, 6, 10):
        assert q(kind, 66, f32, 0) == -1 and q(kind, 1028, bf16, 0) == -1       # d % 4 == 0, d <= 1024
    for kind in (4, 6, 7, 8, 9, 11, 12):
        assert q(kind, 64, bf16, 1) == -1                                      # no 16-byte form
    assert q(0, 100, bf16, 1) == -1 and q(1, 768, bf16, 1) == -1 and q(0, 104, bf16, 1) == -1   # LayerNorm: 64, 128, 256, 512 only
    assert q(2, 100, bf16, 1) == -1 and q(3, 100, bf16, 1) == -1 and q(5, 100, bf16, 1) == -1 and q(10, 100, bf16, 1) == -1
    assert q(11, 257, f32, 0) == -1 and q(11, 256, f32, 0) > 0


def test_cases_cover_what_the_issue_names():
    widths = lambda cases: {c[0] for c in cases}                                # noqa: E731
    paths = lambda cases, d: {c[1] for c in cases if c[0] == d}                 # noqa: E731
    for cases in (G.LN_PLAIN_CASES, G.LN_CASES):
        assert widths(cases) == {64, 100, 128, 256, 512, 768, 1024}
        assert paths(cases, 768) == paths(cases, 1024) == {"f32", "bf16"}
        assert paths(cases, 256) == set(G.PATHS)
    for cases in (G.BN_APPLY_CASES, G.BN_BWD_CASES):
        assert widths(cases) == {64, 100, 104, 128, 256, 512}
        assert paths(cases, 104) == {"bf16", "bf16_ld8"} and paths(cases, 100) == {"f32", "bf16"}
        assert paths(cases, 64) == set(G.PATHS) == paths(cases, 256)
        assert len({c[2:] for c in cases if c[0] == 512}) == 4                   # the whole flag matrix at the shortest lap
    assert widths(G.AXPBY_CASES) == widths(G.DROP_CASES) == widths(G.COLSTATS_CASES) == {64, 100, 128, 256, 512}
    assert {k for d, p, k in G.SUM_CASES if d == 512 and p == "bf16"} == set(G.SUM_K) == {k for d, p, k in G.SUM_CASES if p == "bf16_ld4" and d == 512}
    assert {c[3] for c in G.GATHER_CASES} == {32, 64} and {c[4] for c in G.PAD_CASES} == {0, 32, 64}
    assert G.NLL_CLASSES == [47, 64, 172]
    # the widest operand: 16-byte bf16 at d = 64, about 100 MB with its guard columns
    n = G.rows_at(_q(G.K_BN_APPLY, 64, BF16, 1))
    assert n == 589829 and 70e6 < n * 80 * 2 < 110e6


# ------------------------------------------------------------------------------------------------------------------------------
# exactness preconditions of the builders, at the full N
# ------------------------------------------------------------------------------------------------------------------------------
def _fp32_value(t):
    return torch.equal(t.float().double(), t)


def _bf16_value(t):
    return torch.equal(t.bfloat16().double(), t.double())


def _rounds(t):
    """number of elements of the exact result whose rounding to bf16 changes them"""
    return int((t.bfloat16().double() != t).sum())


def test_streamed_builders():
    n = G.rows_at(_q(G.K_LN_FWD, 64, BF16, 1))                                  # the longest case of the file
    x = G.ints(40, n, 64, -31, 31)
    assert x.shape == (n, 64) and x.dtype == torch.int8 and int(x.min()) == -31 and int(x.max()) == 31
    assert torch.equal(x, G.ints(40, n, 64, -31, 31)) and not torch.equal(x, G.ints(41, n, 64, -31, 31))
    assert _bf16_value(x) and _bf16_value(G.ints(10, 4099, 64, -127, 127))
    z = G.nonzero_ints(30, 4099, 64, 31)
    assert int((z == 0).sum()) == 0 and int(z.min()) == -31 and int(z.max()) == 31 and abs(float(z.float().mean())) < 0.5
    idx = G.gather_index(64, 73733, G.GATHER_SRC, torch.int32)
    assert idx.dtype == torch.int32 and int(idx.min()) == -8 and int(idx.max()) == G.GATHER_SRC + 7
    assert int(((idx < 0) | (idx >= G.GATHER_SRC)).sum()) > 16


@pytest.mark.parametrize("d", [64, 512])
def test_elementwise_references_are_fp32_values_before_their_rounding(d):
    """axpby, the LayerNorm without gamma, bn_apply, bn_bwd_apply, sum_n at the longest N each runs at that width"""
    n = G.rows_at(_q(G.K_BN_APPLY, d, BF16, 1))
    x1, x2, x3 = (G.ints(s, n, d, -31, 31).double() for s in (50, 51, 53))
    y = G.ref_axpby(x1, 3.0, x2, 0.25)
    assert _fp32_value(y) and _rounds(y) > n                                    # the rounding to bf16 is a real one
    for relu in (True, False):
        y = G.ref_ln_plain(x1, x2, 1.5, 0.125, relu)
        assert _fp32_value(y) and _rounds(y) > n
        dx, dres = G.ref_ln_plain_bwd(x3, y, 1.5, 0.125, relu)
        assert _fp32_value(dx) and _fp32_value(dres) and _bf16_value(dx) and _bf16_value(dres)
    for call in (0, 1):
        k = G.bn_coefs(d, call)
        assert set(k["rstd"].tolist()) <= {0.5, 1.0} and set(k["gamma"].tolist()) <= {0.5, 1.0, 2.0}
        assert torch.equal((4 * k["mean"]).round(), 4 * k["mean"]) and torch.equal((2 * k["beta"]).round(), 2 * k["beta"])
        k0, k1 = k["stats"][:d].double() * G.INV_N, k["stats"][d:].double() * G.INV_N
        assert torch.equal((4 * k0).round(), 4 * k0) and torch.equal((16 * k1).round(), 16 * k1)
        assert float(k0.abs().max()) <= 1.0 and float(k1.abs().max()) <= 0.5
    k = G.bn_coefs(d, 0)
    for relu in (True, False):
        for res in (x2, None):
            y = G.ref_bn_apply(x1, k, res, relu)
            assert _fp32_value(y) and torch.equal((16 * y).round(), 16 * y) and float(y.abs().max()) < 128
        assert _rounds(G.ref_bn_apply(x1, k, x2, relu)) > 0
    k = G.bn_coefs(d, 1)
    for relu in (True, False):
        for training in (True, False):
            dx = G.ref_bn_bwd_apply(x3, x1, k, relu, training)
            assert _fp32_value(dx) and torch.equal((512 * dx).round(), 512 * dx) and float(dx.abs().max()) < 256
    assert _rounds(G.ref_bn_bwd_apply(x3, x1, k, True, True)) > 0
    # the pieces of bn_bwd_apply's bracket in fp32, in the kernels' order of operations, against fp64: no rounding anywhere
    xs, gs = x1[:4099].float(), x3[:4099].float()
    xh = (xs - k["mean"]) * k["rstd"]
    inv = torch.tensor(G.INV_N, dtype=F32)
    br = gs - (k["stats"][:d] * inv + xh * k["stats"][d:] * inv)
    xh64 = (xs.double() - k["mean"].double()) * k["rstd"].double()
    br64 = gs.double() - (k["stats"][:d].double() * G.INV_N + xh64 * k["stats"][d:].double() * G.INV_N)
    assert torch.equal(xh.double(), xh64) and torch.equal(br.double(), br64)
    m = G.rows_at(_q(G.K_SUM_N, d, BF16, 1))
    s = sum(G.ints(10 + j, m, d, -127, 127).double() for j in range(8))
    assert _fp32_value(s) and float(s.abs().max()) <= 8 * 127 and _rounds(s) > m


@pytest.mark.parametrize("d", G.WIDTHS + [100])
def test_statistics_are_integer_sums_below_2_24(d):
    """at the larger of the two row counts: colstats with and without shift, bn_bwd_stats / _stats2 with and without relu"""
    n = G.STAT_ROWS[1]
    x = G.ints(60, n, d, -3, 3).float()                                        # fp32 here: integers with abs-sums below 2^24 are exact
    shift = torch.randint(-1, 2, (d,), generator=torch.Generator().manual_seed(d)).float()
    for v in (x, x - shift):
        assert torch.equal(v.round(), v)
        worst = max(float(v.abs().sum(0).max()), float((v * v).sum(0).max()))
        assert 0 < worst < G.EXACT, worst
    k = G.bn_coefs(d, 2)
    xs, gy, gy2 = (G.ints(s, n, d, -2, 2).float() for s in (61, 62, 63))
    for relu in (True, False):
        for g2 in (None, gy2):
            ref, worst = G.ref_bn_bwd_stats(gy, g2, xs, k, relu)
            assert 0 < worst < G.EXACT, worst
            assert torch.equal(ref[:d].round(), ref[:d]) and torch.equal((8 * ref[d:]).round(), 8 * ref[d:])
    c = G.ints(64, n, 47, -3, 3).float()
    assert 0 < float(c.abs().sum(0).max()) < G.EXACT


@pytest.mark.parametrize("c", G.NLL_CLASSES)
def test_nll_builder(c):
    m = G.rows_at(_q(G.K_NLL_BWD, c, F32, 0))
    n = m + 4099
    arg, labels, idx = G.nll_case(c, n, m)
    assert bool((labels != arg).all()) and int(arg.min()) == 0 and int(arg.max()) == c - 1
    bad = (labels < 0) | (labels >= c)
    assert n // 32 < int(bad.sum()) < n // 8
    assert idx.shape == (m,) and idx.unique().numel() == m and not torch.equal(idx, idx.sort().values)
    loss, g = G.ref_nll_onehot(arg, labels, idx, c, G.NLL_INV_DENOM, n)
    assert loss == 128.0 * int((~bad)[idx].sum()) and 0 < loss < 128.0 * m and float(torch.tensor(loss, dtype=F32)) == loss
    assert _bf16_value(g) and set(g.unique().tolist()) == {-G.NLL_INV_DENOM, 0.0, G.NLL_INV_DENOM}
    on = torch.zeros(n, dtype=torch.bool)
    on[idx[(~bad)[idx]]] = True
    assert int((g != 0).sum()) == 2 * int(on.sum()) and int((g[~on] != 0).sum()) == 0 and float(g.sum(1).abs().max()) == 0.0
    assert float(torch.exp(torch.tensor(G.NLL_OFF, dtype=F32))) == 0.0            # exp(-128) is zero in fp32: lse = 0 exactly


# ------------------------------------------------------------------------------------------------------------------------------
# the restated formulas against tests/cpu_kernels.py, known Philox answers and the oracle
# ------------------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """Philox4x32-10 of Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (SC11): the three known-answer vectors of
    the Random123 distribution (counter, key -> output)"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        got = G.philox4x32_10(tuple(torch.tensor([v], dtype=torch.int64) for v in ctr), key)
        assert tuple(int(g) for g in got) == want, [hex(int(g)) for g in got]
    # a * c in 16-bit pieces against Python's integers
    c = torch.tensor([0, 1, 0xFFFF, 0x10000, 0x89ABCDEF, 0xFFFFFFFF], dtype=torch.int64)
    for a in (0xD2511F53, 0xCD9E8D57):
        hi, lo = G._mulhilo(a, c)
        assert [(int(h) << 32) | int(v) for h, v in zip(hi, lo)] == [a * int(v) for v in c]


def test_philox_keep_layout():
    """chunk i covers elements 4 i .. 4 i + 3 of the logical row-major tensor whatever d is; the pattern depends on both seed halves"""
    k64 = G.philox_keep(G.SEED, 50, 64, 0.5, "cpu")
    k100 = G.philox_keep(G.SEED, 32, 100, 0.5, "cpu")
    assert k64.shape == (50, 64) and torch.equal(k64.reshape(-1), k100.reshape(-1))
    assert abs(float(G.philox_keep(G.SEED, 4099, 64, 0.5, "cpu").float().mean()) - 0.5) < 0.01
    assert abs(float(G.philox_keep(G.SEED, 4099, 64, 0.25, "cpu").float().mean()) - 0.75) < 0.01
    for other in (G.SEED ^ 1, G.SEED ^ (1 << 63)):
        assert not torch.equal(G.philox_keep(other, 50, 64, 0.5, "cpu"), k64)
    # the values under a given pattern: tests/cpu_kernels_dropout.py's formula with the pattern put in place of its own draw
    x, res = G.nonzero_ints(30, 50, 64, 31).float(), G.ints(32, 50, 64, -31, 31).float()
    cpu = CpuKernelsDropout()
    assert torch.equal(cpu.dropout(x, res, 0.0, 5), x + res)                    # (p = 0: everything kept)
    assert torch.equal(G.ref_dropout(x.double(), res.double(), torch.ones_like(k64), 0.5).float(), 2 * x + res)
    assert torch.equal(G.ref_dropout(x.double(), None, k64, 0.5).float(), 2 * x * k64)


def test_references_agree_with_the_cpu_kernels():
    n, d = 4099, 64
    D = lambda t: t.double()                                                    # noqa: E731
    x1, x2, x3 = (G.ints(s, n, d, -31, 31).to(BF16) for s in (50, 51, 53))
    same = lambda ref, got: torch.equal(ref.to(got.dtype), got)                 # noqa: E731  (exact references: one rounding)
    assert same(G.ref_axpby(D(x1), 3.0, D(x2), 0.25), C.axpby(x1, 3.0, x2, 0.25))
    xs = [G.ints(10 + j, n, d, -127, 127).to(BF16) for j in range(7)]
    assert same(sum(D(t) for t in xs), C.sum_n(xs))
    for relu in (True, False):
        for res in (x2, None):
            y, _, _ = C.ln_fwd(x1, res, 1.5, 0.125, None, None, relu, G.LN_EPS)
            assert same(G.ref_ln_plain(D(x1), None if res is None else D(res), 1.5, 0.125, relu), y)
            dx, dres, _, _ = C.ln_bwd(x3, y, x1, x2, 1.5, 0.125, None, relu, None, None)
            rdx, rdres = G.ref_ln_plain_bwd(D(x3), D(y), 1.5, 0.125, relu)
            assert same(rdx, dx) and same(rdres, dres)
            k = G.bn_coefs(d, 0)
            assert same(G.ref_bn_apply(D(x1), k, None if res is None else D(res), relu),
                        C.bn_apply(x1, k["mean"], k["rstd"], k["gamma"], k["beta"], res, relu))
        for training in (True, False):
            k = G.bn_coefs(d, 1)
            assert same(G.ref_bn_bwd_apply(D(x3), D(x1), k, relu, training),
                        C.bn_bwd_apply(x3, x1, k["mean"], k["rstd"], k["gamma"], k["beta"], relu, k["stats"], G.INV_N, training))
        k = G.bn_coefs(d, 2)
        g1, g2, xx = (G.ints(s, n, d, -2, 2).to(BF16) for s in (62, 63, 61))
        args = (k["mean"], k["rstd"], k["gamma"], k["beta"], relu)
        assert torch.equal(G.ref_bn_bwd_stats(D(g1), None, D(xx), k, relu)[0].float(), C.bn_bwd_stats(g1, xx, *args))
        assert torch.equal(G.ref_bn_bwd_stats(D(g1), D(g2), D(xx), k, relu)[0].float(), C.bn_bwd_stats2(g1, g2, xx, *args))
    shift = torch.randint(-1, 2, (d,), generator=torch.Generator().manual_seed(d)).float()
    xc = G.ints(60, n, d, -3, 3).to(BF16)
    assert torch.equal(G.ref_colstats(D(xc), D(shift)).float(), C.colstats(xc, shift))
    assert torch.equal(G.ref_colstats(D(xc), None).float(), C.colstats(xc, None))
    assert torch.equal(D(xc).sum(0).float(), C.colsum(xc))
    # gather / pad with in-range indices (the CPU stand-in has no zero rows), then the out-of-range rule on its own
    src = G.ints(20, 300, 65, -127, 127).float()
    idx = torch.randint(0, 300, (999,), generator=torch.Generator().manual_seed(3))
    assert same(G.ref_gather(D(src), idx), C.gather_rows(src, idx, BF16))
    assert same(G.ref_gather(D(src), idx, 68), C.pad_rows(src, idx, 68, BF16))
    assert same(G.ref_gather(D(src), torch.arange(300), 68), C.pad_rows(src, None, 68))
    out = G.ref_gather(D(src), torch.tensor([-1, 0, 299, 300, 2 ** 31 - 1]))
    assert float(out[[0, 3, 4]].abs().max()) == 0.0 and torch.equal(out[1], D(src)[0]) and torch.equal(out[2], D(src)[299])
    # the loss on one-hot logits
    c, m = 47, 1500
    arg, labels, idx = G.nll_case(c, 2000, m)
    logits = torch.full((2000, c), G.NLL_OFF)
    logits[torch.arange(2000), arg] = 0.0
    loss, g = G.ref_nll_onehot(arg, labels, idx, c, G.NLL_INV_DENOM, 2000)
    assert float(C.nll_fwd(logits, labels, idx)) == loss
    assert torch.equal(C.nll_bwd(logits, labels, idx, torch.ones(1), G.NLL_INV_DENOM).double(), g)


def _close(a, b, tol=1e-11):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * float(b.abs().max().clamp_min(1e-300)), float((a - b).abs().max())


def test_references_agree_with_the_oracle_and_the_cpu_kernels_in_floating_point():
    n, d = 1031, 24
    gen = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F64)                    # noqa: E731
    x, res, gy, gamma, beta = r(n, d), r(n, d), r(n, d), r(d) + 2, r(d)
    a, b = 0.3, 0.7
    p = {"ln.weight": gamma, "ln.bias": beta}
    xg, rg = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
    gg, bg = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    out = torch.relu(O._layer_norm({"ln.weight": gg, "ln.bias": bg}, "ln", a * xg + b * rg))
    (out * gy).sum().backward()
    y, mean, rstd, pre = G.ref_ln(x, res, a, b, gamma, beta, True)
    _close(y, torch.relu(O._layer_norm(p, "ln", a * x + b * res)))
    dx, dres, dgamma, dbeta, _, _ = G.ref_ln_bwd(gy, y, pre, a, b, gamma, True, mean, rstd)
    for got, want in ((dx, xg.grad), (dres, rg.grad), (dgamma, gg.grad), (dbeta, bg.grad)):
        _close(got, want, 1e-9)
    cy, cm, cr = C.ln_fwd(x.float(), res.float(), a, b, gamma.float(), beta.float(), True, G.LN_EPS)
    _close(cy.double(), y, 1e-5), _close(cm.double(), mean, 1e-5), _close(cr.double(), rstd, 1e-5)
    cdx, cdres, cdg, cdb = C.ln_bwd(gy.float(), cy, x.float(), res.float(), a, b, gamma.float(), True, cm, cr)
    for got, want in ((cdx, dx), (cdres, dres), (cdg, dgamma), (cdb, dbeta)):
        _close(got.double(), want, 1e-4)
    # BatchNorm in evaluation mode: rstd from the running variance
    rv = torch.rand(d, generator=gen, dtype=F64) + 0.5
    k = {"mean": r(d), "rstd": 1.0 / torch.sqrt(rv + 1e-5), "gamma": gamma, "beta": beta}
    bn = {"bn.weight": gamma, "bn.bias": beta, "bn.running_mean": k["mean"], "bn.running_var": rv}
    _close(G.ref_bn_apply(x, k, res, True), torch.relu(O._batch_norm(bn, "bn", x, False, None)) + res)
    # ... and in training mode, differentiated: ref_bn_bwd_stats feeds ref_bn_bwd_apply
    z = x.clone().requires_grad_(True)
    out = torch.relu(O._batch_norm(bn, "bn", z, True, None))
    gz, = torch.autograd.grad((out * gy).sum(), z)
    mu, var = x.mean(0), ((x - x.mean(0)) ** 2).mean(0)
    k = {"mean": mu, "rstd": 1.0 / torch.sqrt(var + 1e-5), "gamma": gamma, "beta": beta}
    k["stats"], _ = G.ref_bn_bwd_stats(gy, None, x, k, True)
    _close(G.ref_bn_bwd_apply(gy, x, k, True, True, 1.0 / n), gz, 1e-9)
    # the loss
    c, m = 7, 400
    logits, labels = r(n, c), torch.randint(0, c, (n,), generator=gen)
    idx = torch.randperm(n, generator=gen)[:m]
    ref = -torch.log_softmax(logits, 1)[idx, labels[idx]].mean()
    _close(ref.reshape(1), O.nll_loss(logits, labels, idx).reshape(1))
    _close(C.nll_fwd(logits.float(), labels, idx).double() / m, ref.reshape(1), 1e-5)


def test_derived_bounds_hold_for_fp32_arithmetic_on_the_host():
    """ln_stat_bounds against an fp32 evaluation (torch's own summation order: chains no longer than the kernels')"""
    n, d = 2053, 256
    gen = torch.Generator().manual_seed(9)
    x = (torch.randn(n, d, generator=gen) * 1.5 + 0.3).bfloat16()
    res = (torch.randn(n, d, generator=gen) * 1.5 + 0.3).bfloat16()
    gamma, beta = torch.rand(d, generator=gen) + 0.5, torch.randn(d, generator=gen) * 0.1
    _, mean, rstd, pre = G.ref_ln(x.double(), res.double(), 0.5, 0.5, gamma.double(), beta.double(), True)
    _, cm, cr = C.ln_fwd(x, res, 0.5, 0.5, gamma, beta, True, G.LN_EPS)
    e_mean, e_rstd = G.ln_stat_bounds(x.double(), res.double(), 0.5, 0.5, pre, mean, rstd)
    G.check_close("mean", cm, mean, e_mean)
    G.check_close("rstd", cr, rstd, e_rstd)
    assert float((e_mean / mean.abs().clamp_min(0.1)).max()) < 1e-4 and float((e_rstd / rstd).max()) < 1e-4   # and they are tight
    with pytest.raises(AssertionError, match="over the bound"):
        G.check_close("mean", cm * (1 + 1e-4), mean, e_mean)
    with pytest.raises(AssertionError, match="over the bound"):
        G.check_close("rstd", cr * (1 + 1e-4), rstd, e_rstd)
    assert G.ln_row_chain(1024) == 25
    if _lib():
        assert G.ln_chain(18437, 256, False) == 3 + 4 + 50 and G.ln_chain(589829, 64, True) == 12 + 32 + 50
        assert G.ln_chain(589829, 64, False) == 19 + 16 + 50                    # SGF_EW8=0 at the 16-byte forward's N


# ------------------------------------------------------------------------------------------------------------------------------
# sensitivity: the checkers see what a broken loop produces
# ------------------------------------------------------------------------------------------------------------------------------
def test_checkers_reject_a_stale_lap():
    """rows of the second lap left at their initial value (a loop that ran once), in both storage types"""
    d = 64
    lap = _q(G.K_AXPBY, d, F32, 0)
    n = G.rows_at(lap)
    x1, x2 = G.ints(1, n, d, -31, 31).double(), G.ints(2, n, d, -31, 31).double()
    ref = G.ref_axpby(x1, 3.0, x2, 0.25)
    for dtype in (F32, BF16):
        good = ref.to(dtype)
        G.check_stored("y", good, ref)
        stale = good.clone()
        stale[lap:2 * lap] = G.SENTINEL
        with pytest.raises(AssertionError, match="differ from the exact result"):
            G.check_stored("y", stale, ref)
        one = good.clone()
        one[n - 1] = good[n - 2]                                                # the ragged tail's last row took its neighbour's values
        with pytest.raises(AssertionError, match="differ from the exact result"):
            G.check_stored("y", one, ref)


def test_checkers_reject_a_dropped_or_doubled_row_and_a_nonzero_empty_partial():
    d, n = 64, G.STAT_ROWS[0]
    x = G.ints(60, n, d, -3, 3).double()
    shift = torch.randint(-1, 2, (d,), generator=torch.Generator().manual_seed(d)).double()
    ref = G.ref_colstats(x, shift)
    worst = float(max((x - shift).abs().sum(0).max(), ((x - shift) ** 2).sum(0).max()))
    G.check_sums("stats", ref.float(), ref, worst)
    row = 65 * 1000 + 7
    assert bool(((x[row] - shift) != 0).any())
    for bad in (torch.cat([x[:row], x[row + 1:]]), torch.cat([x, x[row:row + 1]])):
        with pytest.raises(AssertionError, match="differ from the exact result"):
            G.check_sums("stats", G.ref_colstats(bad, shift).float(), ref, worst)
    leaked = ref.float()
    leaked[3] += 1.0                                                            # an empty workgroup's partial that was not zero
    with pytest.raises(AssertionError, match="differ from the exact result"):
        G.check_sums("stats", leaked, ref, worst)
    with pytest.raises(AssertionError, match="outside"):
        G.check_sums("stats", ref.float(), ref, float(G.EXACT))
    k = G.bn_coefs(d, 2)
    gy, xs = G.ints(62, n, d, -2, 2).double(), G.ints(61, n, d, -2, 2).double()
    ref, worst = G.ref_bn_bwd_stats(gy, None, xs, k, True)
    G.check_sums("stats", ref.float(), ref, worst)
    keep = torch.ones(n, dtype=torch.bool)
    keep[row] = False
    short, _ = G.ref_bn_bwd_stats(gy[keep], None, xs[keep], k, True)
    with pytest.raises(AssertionError, match="differ from the exact result"):
        G.check_sums("stats", short.float(), ref, worst)


def test_checkers_reject_a_row_normalised_twice():
    """exact form: bn_apply applied to its own output on one row; fp64 form: the LayerNorm of one row's output"""
    d, n = 64, 4099
    k = G.bn_coefs(d, 0)
    x = G.ints(50, n, d, -31, 31).double()
    ref = G.ref_bn_apply(x, k, None, False)
    for dtype in (F32, BF16):
        good = ref.to(dtype)
        G.check_stored("y", good, ref)
        twice = good.clone()
        twice[n - 3] = G.ref_bn_apply(ref[n - 3:n - 2], k, None, False)[0].to(dtype)
        with pytest.raises(AssertionError, match="differ from the exact result"):
            G.check_stored("y", twice, ref)
    gen = torch.Generator().manual_seed(2)
    xr = (torch.randn(n, d, generator=gen) * 1.5 + 0.3).bfloat16()
    gamma, beta = (torch.rand(d, generator=gen) + 0.5).double(), (torch.randn(d, generator=gen) * 0.1).double()
    y, mean, rstd, pre = G.ref_ln(xr.double(), None, 1.0, 0.0, gamma, beta, False)
    for dtype, bars in ((BF16, {}), (F32, {"f32_abs": 2e-5})):
        good = y.to(dtype)
        G.check_per_element("y", good, y, **bars)
        twice = good.clone()
        twice[7] = G.ref_ln(y[7:8], None, 1.0, 0.0, gamma, beta, False)[0][0].to(dtype)
        with pytest.raises(AssertionError, match="over the bound"):
            G.check_per_element("y", twice, y, **bars)
    # dgamma with one row's term missing against the derived bound
    gy = torch.randn(n, d, generator=gen).bfloat16().double()
    _, _, dgamma, dbeta, dz, xh = G.ref_ln_bwd(gy, y, pre, 1.0, 0.0, gamma, False, mean, rstd)
    bound = (3 + 16 + 50 + 5) * G.EPS32 * (dz * xh).abs().sum(0)
    G.check_close("dgamma", dgamma.float(), dgamma, bound)
    with pytest.raises(AssertionError, match="over the bound"):
        G.check_close("dgamma", (dgamma - (dz * xh)[11]).float(), dgamma, bound)
    with pytest.raises(AssertionError, match="over the bound"):
        G.check_close("dbeta", (dbeta - dz[11]).float(), dbeta, (3 + 16 + 50) * G.EPS32 * dz.abs().sum(0))


def test_checkers_reject_a_flipped_keep_bit():
    n, d = 4099, 64
    keep = G.philox_keep(G.SEED, n, d, 0.5, "cpu")
    x = G.nonzero_ints(30, n, d, 31).double()
    res = G.ints(32, n, d, -31, 31).double()
    ref = G.ref_dropout(x, res, keep, 0.5)
    G.check_keep("forward", (ref - res) != 0, keep)
    G.check_stored("y", ref.bfloat16(), ref)
    flipped = keep.clone()
    flipped[n - 1, d - 1] = ~flipped[n - 1, d - 1]
    got = G.ref_dropout(x, res, flipped, 0.5)
    with pytest.raises(AssertionError, match="keep decisions in 1 rows"):
        G.check_keep("forward", (got - res) != 0, keep)
    with pytest.raises(AssertionError, match="differ from the exact result"):
        G.check_stored("y", got.bfloat16(), ref)
    # a counter that restarts with the lap (chunk index taken modulo the grid) repeats the first lap's pattern
    lap = 4096
    wrapped = torch.cat([keep[:lap // d * 4], keep[:n - lap // d * 4]])
    with pytest.raises(AssertionError, match="keep decisions"):
        G.check_keep("forward", wrapped, keep)
