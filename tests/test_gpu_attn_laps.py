"""The attention row kernels where ONE workgroup walks SEVERAL tiles (csrc/attn.hip: k_attn_reduce, k_reduce_bf16, k_attn_apply,
k_apply_bf16; csrc/rowgemm.hip: k_hrow_bf16 where it serves the attention from the input in bf16).

Every case runs N = 3 * 256 * 256 + 5 rows.  With at most 256 workgroups and at most 256 rows per tile every workgroup then
runs at least three tiles (the LDS buffer index goes 0 -> 1 -> 0), some run one more than others, and the last tile has five
rows whatever the tile height (N mod R = 5 for R = 16 ... 256).  tests/test_attn_laps_host.py asserts exactly that from the
library's own geometry queries, so a retuned tile height or grid cap fails there instead of thinning this file out.

Tiles per workgroup at N (ceil(N / R) tiles over 256 workgroups):
    storage   kernel          DP = 64        DP = 128       DP = 256
    fp32      k_attn_reduce   R  64: 12-13   R  32: 24-25   R 16: 48-49
    fp32      k_attn_apply    R 128:  6-7    R  64: 12-13   R 32: 24-25
    bf16      k_reduce_bf16   R 256:  3-4    R 128:  6-7    R 64: 12-13
    bf16      k_apply_bf16    R 256:  3-4    R 128:  6-7    R 64: 12-13
    bf16      k_hrow_bf16     32-row tiles per WAVE, 256 workgroups x 8 waves: 6145 tiles over 2048 waves = 3 (one wave: 4)
k_hrow_bf16 serves sgf_attn_h_fwd / sgf_attn_h_bwd_apply in bf16 at d in {64, 128, 256} when the rows are 16-byte aligned; the
same entries on a view that starts 8 bytes into a row, and d = 100, run k_apply_bf16 (kApplyHFwd / HBwd1 / HBwd2).

How the stages are pinned:
  * reductions (S0, z0, dS0, dz0, the sums of the h form, sgf_gram) BIT-EXACTLY.  The operands are small integers (times powers
    of two), so every product and every partial sum in any order is exactly representable in fp32: torch.equal against fp64.
    One dropped or doubled row among 196 613 changes the result; no tolerance could see that.  Each test first asserts this
    precondition from the inputs (worst abs-sum in units of the quantum < 2^24).
  * the row passes PER ELEMENT, every row:  |got - ref| <= [2^-8 |ref|, bf16 storage only] + R 2^-24 sum|terms|, where the
    terms are the addends ar (A B) + br cvec + gr E of the row expression and R is the number of fp32 operations between the
    (exact) matrix product and the stored value, counted from the kernel source next to each call.  Where bf16 storage rounds a
    stored intermediate a second time (the per-head outputs before their mean, a shared V's gradient accumulated over the
    heads, the first pass of sgf_attn_h_bwd_apply which the second pass reads back) one more 2^-8 |intermediate| is allowed.

The inputs are built once per (H, d) on the host; the fp64 references are the formulas of include/sgf.h as plain torch code
(run on the device's fp64 units here; tests/test_attn_laps_host.py holds the same functions against oracle/sgformer_oracle.py
on the CPU).  Operands carry 64 poisoned rows behind row N and the gradients are written between sentinel columns.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 3 * 256 * 256 + 5
# (heads, head width, heads of V); the H = 1 cases first: the parametrised fixture below shares their instances
CASES = [(1, 64, 1), (1, 128, 1), (1, 100, 1), (1, 256, 1), (2, 64, 2), (2, 64, 1)]
DTYPES = ["float32", "bfloat16"]
NTOT = 4.0
PAD_ROWS = 64          # poisoned rows behind row N of every streamed operand
POISON = 64.0
GAP = 4                # sentinel columns around dq / dk / dv
SENTINEL = 7.0
EPS32 = 2.0 ** -24
EPS16 = 2.0 ** -8
EXACT = 2 ** 24

# fp32 operations between the exact matrix product and the stored value, counted from k_attn_apply / k_apply_bf16 (commit +
# epilogue; k_hrow_bf16 does fewer: one fma per element).  Scalars that are exact by construction (c, a power of two) still count.
R_FWD = 8    # ar = c / den, gr = ntot / den (2); c0 + c1, ar *, gr * e, + (4); head mean: +, / H (2)
R_DQ = 12    # inv, w = g inv, br = c (-gdo inv) (2), gconst (2); c0 + c1, ar *, gr * e, +, br * z0, + (6)
R_DK = 8     # gconst (2); the same six epilogue operations
R_DV = 7     # gr = ntot gscale / den (2); c0 + c1, ar *, gr * e, + (4); + the stored value when accumulating (1), per head
R_HFWD = 8   # den = h.w + beta, ar = 1 / den (2); c0 + c1, ar *, br * m, + (4); gr * e = 0 and its + (2)
R_HBWD = 12  # pass 1: inv, w = g inv, br = -gdo inv (3), c0 + c1, ar *, br * w, + (4); pass 2: c0 + c1, ar *, br * ds, +, += (5)
# longest sequential fp32 chain behind ssq_q / ssq_k: a thread adds <= 49 tiles x (4 products + 1) (fp32: R = 16 at DP = 256;
# bf16: <= 13 tiles x 2 passes x 4 rows x 4) = 416, the wave tree 6, the block's waves 16, k_attn_finalize heads x 256 = 512
L_SSQ = 1024


def padded(d):
    return 64 if d <= 64 else (128 if d <= 128 else 256)


def _tri(gen, shape, m):
    """{-1, 0, 1}: +1 and -1 with probability 1/m each"""
    r = torch.randint(0, m, shape, generator=gen, dtype=torch.int8)
    return (r == 0).to(torch.int8) - (r == 1).to(torch.int8)


class Case:
    pass


def build_case(H, d, n=N):
    """Host inputs of one (H, d): integer-valued (int8) streamed operands and fp32 constants, from a seeded generator."""
    c = Case()
    gen = torch.Generator().manual_seed(7919 * H + d)
    hd, DP = H * d, padded(d)
    c.H, c.d, c.n, c.DP = H, d, n, DP
    q = _tri(gen, (n, hd), 4)                                           # Q in {-1, 0, 1}, nonzero with probability 1/2
    kv = torch.randint(-2, 3, (n, 2 * hd), generator=gen, dtype=torch.int8)  # K, V uniform in {-2 .. 2}
    c.qkv = torch.cat([q, kv], 1)                                       # packed [q | k | v], ld = 3 H d
    c.go = _tri(gen, (n, 2 * hd), 8)                                    # packed [g | o], nonzero with probability 1/4
    c.den = torch.pow(2.0, torch.randint(0, 3, (n, H), generator=gen).float())   # {1, 2, 4} per (row, head)
    # ---- constants of the apply stages ----
    # c = 1 / (sqrt(ssq_q) sqrt(ssq_k)) = 2 / DP, a power of two: |c q.z0| <= 2 d / DP <= 2, so den = c q.z0 + 4 in [2, 6]
    c.ssq_q = 16.0
    c.ssq_k = DP * DP / 4.0 / c.ssq_q
    c.c = 1.0 / (c.ssq_q ** 0.5 * c.ssq_k ** 0.5)
    S0 = 16 * torch.randint(-3, 4, (H, d, d), generator=gen)            # bf16-exact; scaled so the all-pair term shows
    z0 = _tri(gen, (H, d), 3)
    c.stats_in = torch.cat([S0.reshape(-1).float(), z0.reshape(-1).float(), torch.tensor([c.ssq_q, c.ssq_k])])
    # dS0, dz0: redrawn until sdot = <S0, dS0> + <z0, dz0> puts the radial term's factor c |sdot| / ssq_q of dQ in [1/4, 1]:
    # a random sdot is often large enough for -s Q / ||Q||^2 to bury the matrix term (and a tiny one would hide the s term)
    for _ in range(256):
        dS0 = torch.randint(-1, 2, (H, d, d), generator=gen)
        dz0 = _tri(gen, (H, d), 3)
        c.bstats_in = torch.cat([dS0.reshape(-1).float(), dz0.reshape(-1).float(), torch.zeros(1)])
        sdot = abs(float((c.stats_in[:-2].double() * c.bstats_in[:-1].double()).sum()))
        if 0.25 <= c.c * sdot / c.ssq_q <= 1.0:
            break
    else:
        raise AssertionError("no (dS0, dz0) draw with sdot in the window (broken test)")
    # ---- the h form (H = 1): out = (h M + m) / (h.w + beta); |h.w| <= d + 4 (h in {-1, 0, 1}, four columns up to 2) ----
    c.hM = torch.randint(-3, 4, (d, d), generator=gen).float()
    c.hm = torch.randint(-2, 3, (d,), generator=gen).float()
    c.hw = _tri(gen, (d,), 3).float()
    c.hbeta = torch.tensor([DP + 8.0])
    c.hD = torch.randint(-3, 4, (d, d), generator=gen).float()
    c.hds = torch.randint(-2, 3, (d,), generator=gen).float()
    # ---- exactness preconditions: worst abs-sum of any accumulator, in units of the operands' quantum ----
    k, v, g, o = c.qkv[:, hd:2 * hd], c.qkv[:, 2 * hd:], c.go[:, :hd], c.go[:, hd:]
    colabs = lambda t: int(t.abs().sum(0, dtype=torch.int64).max())      # noqa: E731
    gdo = (g.reshape(n, H, d).to(torch.int32) * o.reshape(n, H, d).to(torch.int32)).sum(2).abs()
    c.pre = {
        # sum_n |k||v| <= max|k| max_j sum_n |v_nj|;  sum_n |k|
        "fwd": max(2 * colabs(v), colabs(k)),
        # quantum gscale / 4: |dnum| <= 4 |g| units and |q| <= 1;  |dden| <= 4 |g.o| units
        "bwd": max(4 * colabs(g), 4 * int(gdo.sum(0).max())),
        # <S0, dS0> + <z0, dz0> in units of one
        "sdot": int((c.stats_in[:-2].double() * c.bstats_in[:-1].double()).abs().sum()),
    }
    return c


@functools.lru_cache(maxsize=2)
def get_case(H, d):
    return build_case(H, d)


# ------------------------------------------------------------------------------------------------------------------------------
# fp64 references: the formulas of include/sgf.h.  q, k: [n, H d]; v: [n, Hv d]; g: [n, d] (head mean) or [n, H d] (per head)
# ------------------------------------------------------------------------------------------------------------------------------
def _head(t, h, d):
    return t[:, h * d:(h + 1) * d]


def ref_fwd_reduce(q, k, v, H, vh, d):
    S0 = torch.stack([_head(k, h, d).T @ _head(v, h if vh > 1 else 0, d) for h in range(H)])
    return torch.cat([S0.reshape(-1), k.sum(0), (q * q).sum().reshape(1), (k * k).sum().reshape(1)])


def _unpack(stats, H, d):
    mat = H * d * d
    return stats[:mat].reshape(H, d, d), stats[mat:mat + H * d].reshape(H, d)


def ref_fwd_apply(q, v, stats, ntot, H, vh, d):
    """out, den [n, H], o_heads [n, H d], and per element of o_heads: sum |terms| and the all-pair term"""
    S0, z0 = _unpack(stats, H, d)
    c = 1.0 / (stats[-2].sqrt() * stats[-1].sqrt())
    dens, os_, tabs, pair = [], [], [], []
    for h in range(H):
        qh, vv = _head(q, h, d), _head(v, h if vh > 1 else 0, d)
        den = c * (qh @ z0[h]) + ntot
        ap, sv = c * (qh @ S0[h]) / den[:, None], ntot * vv / den[:, None]
        dens.append(den), os_.append(ap + sv), tabs.append(ap.abs() + sv.abs()), pair.append(ap)
    o = torch.cat(os_, 1)
    out = sum(os_) / H
    return out, torch.stack(dens, 1), o, torch.cat(tabs, 1), torch.cat(pair, 1)


def _row_scalars(g, o, den, h, H, d, per_head):
    gs = 1.0 if per_head else 1.0 / H
    gh = _head(g, h, d) if per_head else g
    inv = gs / den[:, h]
    return gh * inv[:, None], -(gh * _head(o, h, d)).sum(1) * inv          # dnum, dden


def ref_bwd_reduce(q, g, o, den, H, d, per_head):
    """[dS0 | dz0 | 0] and, for the h form, (sum dnum, sum dden) of head 0"""
    dS, dz = [], []
    for h in range(H):
        dnum, dden = _row_scalars(g, o, den, h, H, d, per_head)
        dS.append(_head(q, h, d).T @ dnum), dz.append((_head(q, h, d) * dden[:, None]).sum(0))
    dnum, dden = _row_scalars(g, o, den, 0, H, d, per_head)
    return torch.cat([torch.stack(dS).reshape(-1), torch.cat(dz), dS[0].new_zeros(1)]), dnum.sum(0), dden.sum()


def ref_bwd_apply(q, k, v, g, o, den, stats, bstats, ntot, H, vh, d, per_head):
    """sdot and, for dq / dk / dv, (ref, sum |terms|, all-pair term, twice-rounded intermediate or None)"""
    S0, z0 = _unpack(stats, H, d)
    dS0, dz0 = _unpack(bstats, H, d)
    ssq_q, ssq_k = stats[-2], stats[-1]
    c = 1.0 / (ssq_q.sqrt() * ssq_k.sqrt())
    sdot = (stats[:-2] * bstats[:-1]).sum()
    gs = 1.0 if per_head else 1.0 / H
    res = {"dq": [[], [], []], "dk": [[], [], []], "dv": [[], [], []]}
    for h in range(H):
        qh, kh, vv = _head(q, h, d), _head(k, h, d), _head(v, h if vh > 1 else 0, d)
        dnum, dden = _row_scalars(g, o, den, h, H, d, per_head)
        t = {"dq": (c * (dnum @ S0[h].T), c * dden[:, None] * z0[h], -(c * sdot / ssq_q) * qh),
             "dk": (c * (vv @ dS0[h].T), (c * dz0[h]).expand_as(kh), -(c * sdot / ssq_k) * kh),
             "dv": (c * (kh @ dS0[h]), ntot * dnum)}
        for name, terms in t.items():
            res[name][0].append(sum(terms)), res[name][1].append(sum(x.abs() for x in terms)), res[name][2].append(terms[0])
    out = {}
    for name in ("dq", "dk"):
        out[name] = tuple(torch.cat(x, 1) for x in res[name]) + (None,)
    if vh > 1 or H == 1:
        out["dv"] = tuple(torch.cat(x, 1) for x in res["dv"]) + (None,)
    else:                                                   # shared V: summed over the heads, head 0 stored first
        out["dv"] = (sum(res["dv"][0]), sum(res["dv"][1]), sum(res["dv"][2]), res["dv"][0][0])
    return sdot, out


def ref_h_fwd(h, M, m, w, beta):
    den = h @ w + beta
    t1, t2 = (h @ M) / den[:, None], m / den[:, None]
    return t1 + t2, den, t1.abs() + t2.abs(), t1


def ref_h_bwd_reduce(h, g, o, den):
    """[dM | dw | dm | dbeta]"""
    dnum, dden = g / den, -(g * o).sum(1) / den[:, 0]
    return torch.cat([(h.T @ dnum).reshape(-1), (h * dden[:, None]).sum(0), dnum.sum(0), dden.sum().reshape(1)])


def ref_h_bwd_apply(h, g, o, den, M, w, D, ds):
    """dh, sum |terms|, the two matrix terms, and the first pass's value (stored, then read back by the second pass)"""
    dnum, dden = g / den, -(g * o).sum(1) / den[:, 0]
    t1, t2, t3 = dnum @ M.T, dden[:, None] * w, h @ D
    return t1 + t2 + t3 + ds, t1.abs() + t2.abs() + t3.abs() + ds.abs().expand_as(t1), t1 + t3, t1 + t2


# ------------------------------------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------------------------------------
class Dev:
    """One (case, Hv, storage type) on the device: the packed operands with PAD_ROWS poisoned rows behind row N."""

    def __init__(self, case, vh, dtype, device):
        self.c, self.vh, self.dtype, self.device = case, vh, dtype, device
        H, d, n = case.H, case.d, case.n
        hd = H * d
        self.bufs = {}

        def up(name, t, fill=POISON, dt=dtype):
            buf = torch.full((n + PAD_ROWS, t.shape[1]), fill, dtype=dt, device=device)
            buf[:n] = t.to(device).to(dt)
            self.bufs[name] = (buf, buf.clone())
            return buf[:n]

        if vh == H:                                          # [q | k | v], ld = 3 H d, as ops._Attention passes them
            qkv = up("qkv", case.qkv)
            self.q, self.k, self.v = qkv[:, :hd], qkv[:, hd:2 * hd], qkv[:, 2 * hd:]
        else:                                                # [q | k], ld = 2 H d, and a separate shared V
            qk = up("qk", case.qkv[:, :2 * hd])
            self.q, self.k = qk[:, :hd], qk[:, hd:]
            self.v = up("v", case.qkv[:, 2 * hd:2 * hd + d])
        go = up("go", case.go)
        self.g_heads, self.g, self.o = go[:, :hd], go[:, :d], go[:, hd:]
        self.den = up("den", case.den, fill=1.0, dt=torch.float32)
        for name in ("stats_in", "bstats_in", "hM", "hm", "hw", "hbeta", "hD", "hds"):
            setattr(self, name, getattr(case, name).to(device))

    def f64(self, *ts):
        return tuple(t.double() for t in ts)

    def operands_untouched(self):
        return all(torch.equal(a, b) for a, b in self.bufs.values())

    @property
    def bf16(self):
        return self.dtype == torch.bfloat16


def _ids(cases):
    return [pytest.param((c, t), id="H%d-d%d-v%d-%s" % (c + (t,))) for c in cases for t in DTYPES]


ALL = _ids(CASES)
H1 = _ids([c for c in CASES if c[0] == 1])                   # a prefix of ALL: the module-scoped instances are shared


@pytest.fixture(scope="module")
def dev(request, cuda):
    (H, d, vh), t = request.param
    return Dev(get_case(H, d), vh, getattr(torch, t), cuda)


def _K():
    from sgformer_amd.kernels import HipKernels
    return HipKernels


def check_exact(name, got, ref):
    ref32 = ref.float()
    assert torch.equal(ref32.double(), ref), f"{name}: the reference itself is not an fp32 value (broken test)"
    bad = got != ref32
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} of {bad.numel()} values differ from the exact result, first at "
                                 f"{int(bad.reshape(-1).nonzero()[0])}, worst |diff| {float((got.double() - ref).abs().max())}")


def check_rows(name, got, ref, tabs, R, bf16, twice=None):
    """|got - ref| <= [2^-8 |ref| (+ 2^-8 |twice|) in bf16 storage] + R 2^-24 sum|terms|, every element of every row"""
    tol = R * EPS32 * tabs
    if bf16:
        tol = tol + EPS16 * ref.abs()
        if twice is not None:
            tol = tol + EPS16 * twice.abs()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)                                       # (a NaN fails)
    if bool(bad.any()):
        rows = bad.any(1).nonzero().reshape(-1)
        raise AssertionError(f"{name}: {int(bad.sum())} elements in {rows.numel()} rows over the bound; first row {int(rows[0])}, "
                             f"last row {int(rows[-1])}, worst excess {float((err - tol)[bad].max())}")


def check_visible(name, pair, ref):
    """the term that goes through the matrix cores must show in the output: a kernel that returned the rest would fail"""
    a, b = float(pair.abs().median()), float(ref.abs().median())
    assert a >= 0.25 * b, f"{name}: median |matrix term| {a} < 1/4 median |output| {b} (broken test)"


# ------------------------------------------------------------------------------------------------------------------------------
# reductions: bit-exact
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", ALL, indirect=True)
def test_fwd_reduce_exact(dev):
    """sgf_attn_fwd_reduce: S0 = K^T V and z0 = sum K equal the fp64 values bit for bit (grid (256, H); partials indexed
    head * gridDim.x + block).  ssq_q / ssq_k exceed 2^24 here, so they are bounded by L_SSQ 2^-24 relative: sums of
    non-negative terms, a sanity bound only (where the value is below 2^24 it must be exact)."""
    c = dev.c
    assert c.pre["fwd"] < EXACT, f"abs-sum {c.pre['fwd']} >= 2^24 (broken test)"
    K = _K()
    stats = K.attn_fwd_reduce(dev.q, dev.k, dev.v, c.H, dev.vh, c.d)
    again = K.attn_fwd_reduce(dev.q, dev.k, dev.v, c.H, dev.vh, c.d)
    ref = ref_fwd_reduce(*dev.f64(dev.q, dev.k, dev.v), c.H, dev.vh, c.d)
    check_exact("S0 | z0", stats[:-2], ref[:-2])
    for name, got, want in (("ssq_q", stats[-2], ref[-2]), ("ssq_k", stats[-1], ref[-1])):
        print(f"{name}: got {float(got)!r} ref {float(want)!r}")
        if float(want) < EXACT:
            assert float(got) == float(want), name
        else:
            assert abs(float(got) - float(want)) <= L_SSQ * EPS32 * float(want), name
    assert torch.equal(stats, again)
    assert dev.operands_untouched()


@pytest.mark.parametrize("dev", H1, indirect=True)
def test_gram_exact(dev):
    """sgf_gram (m = k = d) on the same integer operands: C = K^T V and the column sums of K, exact.  fp32 storage runs
    k_attn_reduce<kModeGram> (R and laps as the forward reduce); bf16 runs whichever Gram kernel the entry picks."""
    c = dev.c
    assert c.pre["fwd"] < EXACT, f"abs-sum {c.pre['fwd']} >= 2^24 (broken test)"
    out, cs = _K().gram(dev.k, dev.v)
    out2, cs2 = _K().gram(dev.k, dev.v)
    k64, v64 = dev.f64(dev.k, dev.v)
    check_exact("K^T V", out, k64.T @ v64)
    check_exact("colsum K", cs, k64.sum(0))
    assert torch.equal(out, out2) and torch.equal(cs, cs2)


@pytest.mark.parametrize("per_head", [False, True])
@pytest.mark.parametrize("dev", ALL, indirect=True)
def test_bwd_reduce_exact(dev, per_head):
    """sgf_attn_bwd_reduce / _heads: dS0 = sum Q^T dnum and dz0 = sum Q dden, exact (den in {1, 2, 4} and H in {1, 2}: gscale / den
    is a power of two, dnum a multiple of 1/8 that survives the bf16 kernel's re-rounding); the last slot is zeroed."""
    c = dev.c
    assert c.pre["bwd"] < EXACT, f"abs-sum {c.pre['bwd']} >= 2^24 (broken test)"
    g = dev.g_heads if per_head else dev.g
    K = _K()
    bstats = K.attn_bwd_reduce(dev.q, g, dev.o, dev.den, c.H, c.d, per_head=per_head)
    again = K.attn_bwd_reduce(dev.q, g, dev.o, dev.den, c.H, c.d, per_head=per_head)
    ref, _, _ = ref_bwd_reduce(*dev.f64(dev.q, g, dev.o, dev.den), c.H, c.d, per_head)
    check_exact("dS0 | dz0 | 0", bstats, ref)
    assert torch.equal(bstats, again)
    assert dev.operands_untouched()


@pytest.mark.parametrize("dev", H1, indirect=True)
def test_h_bwd_reduce_exact(dev):
    """sgf_attn_h_bwd_reduce (kModeBwdH): [dM | dw | dm = sum dnum | dbeta = sum dden], exact."""
    c = dev.c
    assert c.pre["bwd"] < EXACT, f"abs-sum {c.pre['bwd']} >= 2^24 (broken test)"
    den = dev.den.contiguous()
    K = _K()
    hstats = K.attn_h_bwd_reduce(dev.q, dev.g, dev.o, den)
    again = K.attn_h_bwd_reduce(dev.q, dev.g, dev.o, den)
    ref = ref_h_bwd_reduce(*dev.f64(dev.q, dev.g, dev.o, den))
    check_exact("dM | dw | dm | dbeta", hstats, ref)
    assert torch.equal(hstats, again)


# ------------------------------------------------------------------------------------------------------------------------------
# row passes: per element, every row
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", ALL, indirect=True)
def test_fwd_apply_rows(dev):
    """sgf_attn_fwd_apply (kApplyFwd per head, k_head_mean): out, o_heads per element; den exact (c a power of two, q.z0 an
    integer: den = c q.z0 + 4 has no rounding in any order)."""
    c = dev.c
    K = _K()
    out, den, o_heads = K.attn_fwd_apply(dev.q, dev.v, dev.stats_in, NTOT, c.H, dev.vh, c.d)
    out2, den2, oh2 = K.attn_fwd_apply(dev.q, dev.v, dev.stats_in, NTOT, c.H, dev.vh, c.d)
    q, v, st = dev.f64(dev.q, dev.v, dev.stats_in)
    r_out, r_den, r_o, tabs, pair = ref_fwd_apply(q, v, st, NTOT, c.H, dev.vh, c.d)
    check_visible("o_heads", pair, r_o)
    assert float(r_den.min()) >= 2.0
    check_exact("den", den, r_den)
    if c.H > 1:
        check_rows("o_heads", o_heads, r_o, tabs, R_FWD, dev.bf16)
        mean_abs = sum(_head(r_o, h, c.d).abs() for h in range(c.H)) / c.H
        check_rows("out", out, r_out, sum(_head(tabs, h, c.d) for h in range(c.H)) / c.H, R_FWD, dev.bf16, twice=mean_abs)
        assert torch.equal(o_heads, oh2)
    else:
        check_rows("out", out, r_out, tabs, R_FWD, dev.bf16)
    assert torch.equal(out, out2) and torch.equal(den, den2)
    assert dev.operands_untouched()


@pytest.mark.parametrize("per_head", [False, True])
@pytest.mark.parametrize("dev", ALL, indirect=True)
def test_bwd_apply_rows(dev, per_head):
    """sgf_attn_bwd_apply / _heads (k_attn_sdot, then kApplyDQ / DK / DV per head): dq, dk, dv per element, written between
    sentinel columns; bstats[-1] = <S0, dS0> + <z0, dz0> exactly."""
    c = dev.c
    H, d, vh, n = c.H, c.d, dev.vh, c.n
    hd = H * d
    assert c.pre["sdot"] < EXACT, f"abs-sum {c.pre['sdot']} >= 2^24 (broken test)"
    g = dev.g_heads if per_head else dev.g
    K = _K()
    widths = {"dq": hd, "dk": hd, "dv": vh * d}

    def run():
        buf = torch.full((n + PAD_ROWS, 4 * GAP + 2 * hd + vh * d), SENTINEL, dtype=dev.dtype, device=dev.device)
        views, mask, col = {}, torch.ones_like(buf, dtype=torch.bool), GAP
        for name, w in widths.items():
            views[name] = buf[:n, col:col + w]
            mask[:n, col:col + w] = False
            col += w + GAP
        bstats = dev.bstats_in.clone()
        K.attn_bwd_apply(dev.q, dev.k, dev.v, g, dev.o, dev.den, dev.stats_in, bstats, NTOT, H, vh, d,
                         views["dq"], views["dk"], views["dv"], per_head=per_head)
        return buf, views, mask, bstats

    buf, views, mask, bstats = run()
    buf2, _, _, bstats2 = run()
    sdot, ref = ref_bwd_apply(*dev.f64(dev.q, dev.k, dev.v, g, dev.o, dev.den, dev.stats_in, dev.bstats_in), NTOT, H, vh, d,
                              per_head)
    assert float(bstats[-1]) == float(sdot), (float(bstats[-1]), float(sdot))
    assert torch.equal(bstats[:-1], dev.bstats_in[:-1])
    shared = vh == 1 and H > 1
    for name, R in (("dq", R_DQ), ("dk", R_DK), ("dv", R_DV * (H if shared else 1))):
        r, tabs, pair, twice = ref[name]
        check_visible(name, pair, r)
        check_rows(name, views[name], r, tabs, R, dev.bf16, twice=twice)
    assert bool((buf[mask] == SENTINEL).all()), "a sentinel column or a row behind N was written"
    assert torch.equal(buf, buf2) and torch.equal(bstats, bstats2)
    assert dev.operands_untouched()


def _h_views(dev, shifted):
    """h, g, o of the h form: the packed buffers' first columns, or h and g from column 4 on (rows 8 bytes off a 16-byte
    boundary in bf16: sgf_attn_h_fwd / _bwd_apply then run k_apply_bf16 instead of k_hrow_bf16)"""
    d, s = dev.c.d, 4 if shifted else 0
    wide = dev.bufs["qkv"][0][:dev.c.n]
    go = dev.bufs["go"][0][:dev.c.n]
    return wide[:, s:s + d], go[:, s:s + d], go[:, d:2 * d]


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("dev", H1, indirect=True)
def test_h_fwd_rows(dev, shifted):
    """sgf_attn_h_fwd: out = (h M + m) / (h.w + beta) per element; den = h.w + beta is an integer: exact.
    bf16 at d in {64, 128, 256}: k_hrow_bf16, three 32-row tiles per wave (one wave four); shifted or d = 100: k_apply_bf16."""
    h, _, _ = _h_views(dev, shifted)
    K = _K()
    out, den = K.attn_h_fwd(h, dev.hM, dev.hm, dev.hw, dev.hbeta)
    out2, den2 = K.attn_h_fwd(h, dev.hM, dev.hm, dev.hw, dev.hbeta)
    r, r_den, tabs, pair = ref_h_fwd(*dev.f64(h, dev.hM, dev.hm, dev.hw, dev.hbeta))
    check_visible("out", pair, r)
    assert float(r_den.min()) >= 2.0
    check_exact("den", den[:, 0], r_den)
    check_rows("out", out, r, tabs, R_HFWD, dev.bf16)
    assert torch.equal(out, out2) and torch.equal(den, den2)
    assert dev.operands_untouched()


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("dev", H1, indirect=True)
def test_h_bwd_apply_rows(dev, shifted):
    """sgf_attn_h_bwd_apply: dh = dnum M^T + dden w + h D + ds per element.  Both implementations store the first pass's
    dnum M^T + dden w in the storage type and the second pass reads it back: in bf16 that intermediate is rounded once more.
    bf16 at d in {64, 128, 256}: k_hrow_bf16 (kHB1, kHB2), three 32-row tiles per wave (one wave four); else k_apply_bf16."""
    h, g, o = _h_views(dev, shifted)
    den = dev.den.contiguous()
    K = _K()
    dh = K.attn_h_bwd_apply(h, g, o, den, dev.hM, dev.hw, dev.hD, dev.hds)
    dh2 = K.attn_h_bwd_apply(h, g, o, den, dev.hM, dev.hw, dev.hD, dev.hds)
    r, tabs, pair, first = ref_h_bwd_apply(*dev.f64(h, g, o, den, dev.hM, dev.hw, dev.hD, dev.hds))
    check_visible("dh", pair, r)
    check_rows("dh", dh, r, tabs, R_HBWD, dev.bf16, twice=first)
    assert torch.equal(dh, dh2)
    assert dev.operands_untouched()
