"""The persistent kernels of csrc/fused.hip where ONE workgroup iterates SEVERAL times: LayerNorm and BatchNorm forward and
backward, the column statistics, axpby, sum_n, dropout, the row gather and pad, the log-softmax NLL loss.

Their grids are capped at 2048 workgroups of 256 threads and every workgroup walks its rows in a grid-stride loop (the column
reductions and sgf_nll_fwd: in contiguous blocks).  sgf_ew_lap_rows reports the rows one loop iteration of the capped grid
covers ("lap") from the functions the entries size their grids with; every case here runs
    N = 2 lap + lap / 4 + 5
rows of the kernel it reaches: every workgroup iterates twice, a quarter of them a third time, and the last group of rows is
ragged (in the row-unrolled kernels the third iteration has early rows of the unroll in range and later ones out of range).
The blocked reductions run n = 131 073 (rows per workgroup 65: workgroups 2017 .. 2047 have no rows and must contribute exact
zeros) and n = 2 * 131 072 + 5; sgf_nll_fwd, whose grid stops growing at 65 536 training rows, also m = 65 537 and 131 077.
Laps as queried (tests/test_ew_laps_host.py asserts this table, so a retuned grid fails there instead of thinning this file):
    sgf_ln_fwd / sgf_ln_bwd, fp32 and 8-byte bf16      d <= 64: 32 768   d <= 128: 16 384   wider (to 1024): 8 192
    the same, 16-byte bf16                             d = 64: 262 144   128: 131 072   256: 65 536   512: 32 768
    sgf_bn_apply / sgf_bn_bwd_apply, fp32 and 8-byte   d = 64: 131 072   100: 81 920   128: 65 536   256: 32 768   512: 16 384
    the same, 16-byte bf16                             d = 64: 262 144   104: 155 648   128: 131 072   256: 65 536   512: 32 768
    axpby, sum_n, dropout, gather_rows (4-col chunks)  d = 64: 32 768   100: 20 971 (.52: ends inside a row)   256: 8 192   512: 4 096
    sum_n, 16-byte bf16                                d = 64: 65 536   128: 32 768   256: 16 384   512: 8 192
    sgf_pad_rows (elements)                            d_pad = 68: 7 710   104: 5 041
    sgf_nll_bwd                                        c <= 64: 32 768   c > 64: 8 192 training rows

Which kernel a case reaches ("path"): fp32 rows contiguous or as column slices of a buffer 4 columns wider; bf16 rows
contiguous or in a buffer 8 columns wider (16 bytes per lane where the width has such a kernel), in a buffer 4 columns wider
with the output 8 bytes into its row (rows only 8-byte aligned: the 8-byte kernels), and contiguous under SGF_EW8=0 (the 8-byte
kernels again; sgf_ln_fwd does not read that switch, so its lap stays the 16-byte one and N is taken from the longer lap).

EXACT wherever the arithmetic allows: operands are small integers times powers of two, so the fp64 formula of include/sgf.h
rounded ONCE to the storage type must be reproduced bit for bit whatever the compiler contracts; each check first asserts
that its reference is an fp32 value before that rounding, and the integer sums assert their abs-sums (in units of their
quantum) below 2^24 from the data.  A stale lap, a row written twice, a dropped or doubled row in a statistic, a non-zero
partial of an empty workgroup or a flipped keep bit changes an integer; no tolerance hides it.
  * axpby, sum_n (k = 2, 3, 7, 8), gather_rows / pad_rows (int32 / int64 indices, some outside [0, n_src): zero rows), LayerNorm
    with gamma = NULL (relu(a x + b res) and its backward), bn_apply / bn_bwd_apply with the power-of-two constants of bn_coefs,
    colstats (with and without shift), bn_bwd_stats / _stats2, colsum (d = 47), the NLL loss on one-hot logits (0 at one class,
    -128 elsewhere: exp(-128) is 0 in fp32, lse = 0, every training row adds 128, the gradient is scale (onehot(argmax) -
    onehot(label))).
  * dropout: the keep pattern against Philox4x32-10 restated in torch integer arithmetic (philox_keep: counter = (chunk lo,
    chunk hi, 0x5347464d, 0), one per 4 consecutive elements of the logical [n, d] tensor, key = seed; known-answer vectors in
    the host file) over the WHOLE tensor, element for element — the integer Philox runs on the device, so no row bands were
    needed — kept values x / (1 - p) (+ res) with p = 1/2 exactly, and the backward reproducing the pattern.
AGAINST fp64 of the same stored inputs (on the device) where exp, log, sqrt or a division is involved: LayerNorm with gamma
and the NLL loss on random logits.  Per element the project's bars: 0.51 ulp(bf16) + 1e-5 on bf16 outputs, 2e-5 absolute on
fp32 y, 1e-5 relative on fp32 dx / dres, test_fused_loss's bars on the loss.  mean, rstd, dgamma and dbeta are bounded by
derivation (ln_stat_bounds, ln_chain): L 2^-24 sum|terms| with L counted from the kernels at that N.

Memory contract in the same calls: streamed operands carry 64 poisoned rows behind row N (and poisoned columns where they are
column slices), row-major outputs lie between sentinel columns and in front of sentinel rows, mean / rstd / statistics have
sentinels behind their last element, workspaces sentinel bytes behind *_workspace_bytes; all must be unchanged.

294 tests, 14 s on an MI355X (the slowest 0.9 s).  Against a scratch build whose loops in fused.hip run a single pass (and whose
blocked reductions take 64 rows per workgroup whatever n is) 292 of them fail, each from the first row of the second lap on;
the two that pass are sgf_nll_fwd at m = 65 537 and c = 47, where that build drops one training row whose label is outside [0, c).
"""
import ctypes
import functools
import os

import pytest
import torch

from tests.test_gpu_attn_laps import EXACT, PAD_ROWS, POISON, SENTINEL, check_exact
from tests.test_gpu_row_laps import INV_N, Guarded, Opaque, Operands, _L, _ld, _p, _st, bn_coefs, check_bf16

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS32 = 2.0 ** -24
LN_EPS = 1e-5

# kinds of sgf_ew_lap_rows
K_LN_FWD, K_LN_BWD, K_BN_APPLY, K_BN_BWD_APPLY, K_AXPBY, K_SUM_N, K_DROPOUT, K_GATHER, K_PAD, K_NLL_BWD = range(10)
K_COLSTATS, K_COLSUM, K_NLL_FWD = 10, 11, 12

WIDTHS = [64, 128, 256, 512]
STAT_CAP = 131072                       # rows at which the grid of the column reductions stops growing
STAT_ROWS = [STAT_CAP + 1, 2 * STAT_CAP + 5]
NLL_CAP = 65536
NLL_FWD_ROWS = [NLL_CAP + 1, 2 * NLL_CAP + 5]
NLL_CLASSES = [47, 64, 172]
NLL_OFF = -128.0
NLL_INV_DENOM = 2.0 ** -16
SUM_K = [2, 3, 7, 8]
SEED = 0x9E3779B97F4A7C15               # a 64-bit dropout seed with bits in both halves
TAIL_ELEMS = 64                         # sentinel elements behind mean / rstd / a statistics vector

# path -> (storage dtype, extra columns of the operand buffers, sentinel columns each side of an output, SGF_EW8)
PATHS = {
    "f32": (F32, 0, 8, None), "f32_ld4": (F32, 4, 4, None),
    "bf16": (BF16, 0, 8, None), "bf16_ld8": (BF16, 8, 8, None), "bf16_ld4": (BF16, 4, 4, None), "bf16_env": (BF16, 0, 8, "0"),
}
MAIN, ALT = ["f32", "bf16"], ["f32_ld4", "bf16_ld8", "bf16_ld4", "bf16_env"]
ALT_AT = (64, 256)                      # the widths that also run the alternative paths


def ln8_width(d):
    return d in (64, 128, 256, 512)


def ew8_width(d):
    return d % 8 == 0


def no_wide(d):
    return False


def runs_wide(path, d, has_wide, reads_env=True):
    """does the entry launch its 16-byte bf16 kernel on this path"""
    dtype, extra, _gap, env = PATHS[path]
    return dtype == BF16 and has_wide(d) and extra % 8 == 0 and not (env == "0" and reads_env)


def lap_rows(kind, d, dtype, wide):
    L = _L()
    lap = L.load().sgf_ew_lap_rows(kind, d, L.SGF_BF16 if dtype == BF16 else L.SGF_F32, int(wide))
    assert lap > 0, (kind, d, dtype, wide, lap)
    return int(lap)


def rows_at(lap):
    return 2 * lap + lap // 4 + 5


def path_rows(kind, d, path, has_wide, reads_env=True):
    return rows_at(lap_rows(kind, d, PATHS[path][0], runs_wide(path, d, has_wide, reads_env)))


def width_cases(widths, has_wide, narrow=(), wide_only=()):
    """(d, path): fp32 and bf16 at every width, the alternative paths at ALT_AT; `narrow` widths have no 16-byte kernel, `wide_only`
    widths run bf16 alone"""
    out = []
    for d in list(widths) + list(narrow) + list(wide_only):
        for p in MAIN + (ALT if d in ALT_AT else []):
            if d in wide_only and PATHS[p][0] != BF16:
                continue
            if not has_wide(d) and p in ("bf16_ld8", "bf16_env"):
                continue
            out.append((d, p))
    if wide_only:
        out += [(d, "bf16_ld8") for d in wide_only]
    return out


def case_list(widths, has_wide, flags, narrow=(), wide_only=(), full_at=512):
    """every (d, path) with the first flag combination, and the whole flag matrix on fp32 and bf16 at the width with the shortest lap"""
    out = [(d, p) + tuple(flags[0]) for d, p in width_cases(widths, has_wide, narrow, wide_only)]
    out += [(full_at, p) + tuple(f) for p in MAIN for f in flags[1:]]
    return out


def _ids(v):
    """id of ONE parameter value (pytest joins them)"""
    return str(int(v)) if isinstance(v, bool) else str(v)


# ------------------------------------------------------------------------------------------------------------------------------
# host builders (seeded, integer-valued) and the restated formulas of include/sgf.h
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def ints(seed, n, d, lo, hi):
    """[n, d] int8, uniform in {lo .. hi}"""
    gen = torch.Generator().manual_seed(1000003 * seed + 31 * d + 7)
    return torch.randint(lo, hi + 1, (n, d), generator=gen, dtype=torch.int8)


def nonzero_ints(seed, n, d, hi):
    """[n, d] int8, uniform in {-hi .. -1, 1 .. hi}: no zero, so a kept element of the dropout is visibly kept"""
    t = ints(seed, n, d, 0, 2 * hi - 1)
    return torch.where(t < hi, t - hi, t - hi + 1)


def gather_index(seed, n_out, n_src, dtype):
    """indices in [-8, n_src + 8): about 16 / (n_src + 16) of them outside [0, n_src)"""
    gen = torch.Generator().manual_seed(7001 + seed)
    return torch.randint(-8, n_src + 8, (n_out,), generator=gen, dtype=torch.int64).to(dtype)


def nll_case(c, n, m, seed=0):
    """one-hot logits source (argmax per row), labels that differ from the argmax on every row, one label in 16 outside [0, c),
    and a seeded permutation's first m rows as the index"""
    gen = torch.Generator().manual_seed(9001 + 131 * c + seed)
    arg = torch.randint(0, c, (n,), generator=gen)
    labels = (arg + 1 + torch.randint(0, c - 1, (n,), generator=gen)) % c
    bad = torch.randint(0, 16, (n,), generator=gen) == 0
    wrong = torch.tensor([-1, c, c + 5, 2 ** 40])[torch.randint(0, 4, (n,), generator=gen)]
    labels = torch.where(bad, wrong, labels)
    idx = torch.randperm(n, generator=gen)[:m]
    return arg, labels, idx


def ref_axpby(x1, a, x2, b):
    return a * x1 + b * x2


def ref_ln_plain(x, res, a, b, relu):
    """sgf_ln_fwd with gamma = NULL: [relu](a x + b res)"""
    pre = a * x if res is None else a * x + b * res
    return torch.relu(pre) if relu else pre


def ref_ln_plain_bwd(gy, y, a, b, relu):
    dz = gy * (y > 0) if relu else gy
    return a * dz, b * dz


def ref_ln(x, res, a, b, gamma, beta, relu, eps=LN_EPS):
    """(y, mean, rstd, pre) of sgf_ln_fwd with gamma"""
    pre = a * x if res is None else a * x + b * res
    mean = pre.mean(1)
    rstd = 1.0 / torch.sqrt(((pre - mean[:, None]) ** 2).mean(1) + eps)
    z = (pre - mean[:, None]) * rstd[:, None] * gamma + beta
    return (torch.relu(z) if relu else z), mean, rstd, pre


def ref_ln_bwd(gy, y, pre, a, b, gamma, relu, mean, rstd):
    """(dx, dres, dgamma, dbeta, dz, xhat) of sgf_ln_bwd from the stored y (relu mask), mean and rstd"""
    dz = gy * (y > 0) if relu else gy
    xh = (pre - mean[:, None]) * rstd[:, None]
    dxh = dz * gamma
    dp = rstd[:, None] * (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True))
    return a * dp, b * dp, (dz * xh).sum(0), dz.sum(0), dz, xh


def ref_bn_apply(x, k, res, relu):
    t = lambda v: v.to(x)                                     # noqa: E731
    y = (x - t(k["mean"])) * t(k["rstd"]) * t(k["gamma"]) + t(k["beta"])
    if relu:
        y = torch.relu(y)
    return y if res is None else y + res


def ref_bn_bwd_apply(gy, x, k, relu, training, inv_n=INV_N):
    d = x.shape[1]
    t = lambda v: v.to(x)                                     # noqa: E731
    xh = (x - t(k["mean"])) * t(k["rstd"])
    g = gy * ((xh * t(k["gamma"]) + t(k["beta"])) > 0) if relu else gy
    if training:
        g = g - (t(k["stats"][:d]) * inv_n + xh * t(k["stats"][d:]) * inv_n)
    return t(k["gamma"]) * t(k["rstd"]) * g


def ref_colstats(x, shift):
    v = x if shift is None else x - shift
    return torch.cat([v.sum(0), (v * v).sum(0)])


def ref_bn_bwd_stats(gy, gy2, x, k, relu):
    """([sum g' | sum g' xhat], the same sums of absolute values in units of the quantum 1/8)"""
    t = lambda v: v.to(x)                                     # noqa: E731
    g = gy if gy2 is None else gy + gy2
    xh = (x - t(k["mean"])) * t(k["rstd"])
    if relu:
        g = g * ((xh * t(k["gamma"]) + t(k["beta"])) > 0)
    worst = max(float(g.abs().sum(0).max()), 8.0 * float((g * xh).abs().sum(0).max()))
    return torch.cat([g.sum(0), (g * xh).sum(0)]), worst


def ref_gather(src, idx, d_pad=None):
    """out[i] = src[idx[i]] (zero row for an index outside [0, n_src)), zero-padded to d_pad columns"""
    n_src, d = src.shape
    i = idx.long()
    ok = (i >= 0) & (i < n_src)
    out = src[i.clamp(0, n_src - 1)] * ok[:, None].to(src.dtype)
    if d_pad is not None and d_pad > d:
        out = torch.cat([out, torch.zeros((out.shape[0], d_pad - d), dtype=out.dtype, device=out.device)], 1)
    return out


def ref_nll_onehot(arg, labels, idx, c, scale, n):
    """(loss_sum, dlogits [n, c]) on the one-hot logits: 128 per training row with a label in [0, c)"""
    lab = labels[idx]
    ok = (lab >= 0) & (lab < c)
    rows = idx[ok]
    g = torch.zeros((n, c), dtype=F64, device=arg.device)
    g[rows, arg[rows]] = scale
    g[rows, lab[ok]] = -scale
    return -NLL_OFF * float(ok.sum()), g


# ---- Philox4x32-10 in integer tensors (every intermediate below 2^49: int64 never wraps) ----
_M32 = 0xFFFFFFFF


def _mulhilo(a, c):
    """(high, low) 32 bits of a * c for a Python int a < 2^32 and an int64 tensor c in [0, 2^32)"""
    a_lo, a_hi = a & 0xFFFF, a >> 16
    c_lo, c_hi = c & 0xFFFF, c >> 16
    t0, t1, t2 = c_lo * a_lo, c_lo * a_hi + c_hi * a_lo, c_hi * a_hi
    s = t0 + ((t1 & 0xFFFF) << 16)
    return t2 + (t1 >> 16) + (s >> 32), s & _M32


def philox4x32_10(ctr, key):
    """ctr: four int64 tensors in [0, 2^32); key: two Python ints.  The ten rounds with the Weyl key schedule."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key[0] & _M32, key[1] & _M32
    for _ in range(10):
        hi0, lo0 = _mulhilo(0xD2511F53, c0)
        hi1, lo1 = _mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def philox_keep(seed, n, d, p, device):
    """keep [n, d] bool of sgf_dropout: chunk i = 4 consecutive elements of the logical [n, d] tensor, counter (i lo, i hi,
    0x5347464d, 0), key (seed lo, seed hi); element j of the chunk is kept when (word_j >> 8) 2^-24 >= p in fp32"""
    assert d % 4 == 0
    i = torch.arange(n * d // 4, dtype=torch.int64, device=device)
    z = torch.zeros_like(i)
    words = philox4x32_10((i & _M32, i >> 32, z + 0x5347464D, z), (seed & _M32, (seed >> 32) & _M32))
    pf = torch.tensor(p, dtype=F32, device=device)
    keep = torch.stack([(w >> 8).to(F32) * (1.0 / 16777216.0) >= pf for w in words], 1)
    return keep.reshape(n, d)


def ref_dropout(x, res, keep, p):
    y = x * keep.to(x.dtype) * (1.0 / (1.0 - p))
    return y if res is None else y + res


# ---- derived bounds for the LayerNorm with gamma ----
def ln_row_chain(d):
    """fp32 operations behind a row sum of the LayerNorm kernels: a x and its fma (2), at most 16 elements added per lane
    (k_ln_fwd: 4 chunks of 4 at d = 1024; the 16-byte kernels: 8), the 6 levels of group_sum, one division"""
    return 2 + 16 + 6 + 1


def ln_stat_bounds(x, res, a, b, pre, mean, rstd, eps=LN_EPS):
    """|mean - ref| and |rstd - ref| per row, from the fp64 reference (x, res the stored inputs; pre, mean, rstd in fp64).
    u = 2^-24.  pre carries e_p <= 2 u (|a x| + |b res|) (one product, one fma).  mean: the chain of ln_row_chain on top,
    e_mu <= L u mean|pre|.  Each (pre - mean) then carries delta <= e_p + e_mu + u |pre - mean|, the mean square
    e_var <= 2 mean|pre - mean| delta + L u var, and rstd = 1 / sqrt(var + eps) e_var / (2 (var + eps)) relative plus three
    more roundings (the sum with eps, sqrt, the division).  (e_mu also takes the e_p of the row's elements, at their maximum.)"""
    L = ln_row_chain(x.shape[1])
    mag = (a * x).abs() if res is None else (a * x).abs() + (b * res).abs()
    e_p = 2 * EPS32 * mag.amax(1)
    e_mu = L * EPS32 * pre.abs().mean(1) + e_p
    dev = (pre - mean[:, None]).abs()
    delta = e_p + e_mu + EPS32 * dev.amax(1)
    var = (dev * dev).mean(1)
    e_var = 2 * dev.mean(1) * delta + L * EPS32 * var
    return e_mu, rstd * (e_var / (2 * (var + eps)) + 3 * EPS32)


def ln_chain(n, d, wide):
    """longest sequential fp32 chain behind one column of dgamma / dbeta at n rows.  A thread adds one term per row it
    visits: ceil(n / lap) iterations of 1 row (k_ln_bwd) or of 4 rows (k_ln_bwd_bf16x8); the block adds its row slots in
    order: 256 / lanes per row = 16, 8 or 4 (k_ln_bwd), 32, 16, 8 or 4 (bf16x8: 256 / (d / 8)); k_sum_partials over the 2048
    partials: 16 per chain, (s0 + s1) + (s2 + s3), then the 32 groups in order = 16 + 2 + 32."""
    lap = lap_rows(K_LN_BWD, d, BF16 if wide else F32, wide)
    iters = -(-n // lap)
    if wide:
        return 4 * iters + 256 // (d // 8) + 50
    lanes = 16 if d <= 64 else (32 if d <= 128 else 64)
    return iters + 256 // lanes + 50


def ulp_bf16(t):
    """one bf16 unit in the last place at the magnitude of t (fp64)"""
    return torch.clamp(t.abs(), min=2.0 ** -126).log2().floor().exp2() * 2.0 ** -7


# ------------------------------------------------------------------------------------------------------------------------------
# checkers
# ------------------------------------------------------------------------------------------------------------------------------
def check_stored(name, got, ref):
    """got equals the exact fp64 result rounded ONCE to got's storage type; the exact result must be an fp32 value"""
    if got.dtype == BF16:
        check_bf16(name, got, ref)
    else:
        assert got.dtype == F32 and got.shape == ref.shape, (name, got.dtype, got.shape, ref.shape)
        check_exact(name, got, ref)


def check_sums(name, got, ref, worst):
    """integer sums (in units of their quantum): exact, and the precondition that makes them so"""
    assert 0 < worst < EXACT, f"{name}: abs-sum {worst} outside (0, 2^24) (broken test)"
    check_exact(name, got, ref)


def check_keep(name, got_nonzero, keep):
    """the kernel's keep pattern (non-zero outputs of non-zero inputs) against the Philox pattern, element for element"""
    bad = got_nonzero != keep
    if bool(bad.any()):
        rows = bad.any(1).nonzero().reshape(-1)
        raise AssertionError(f"{name}: {int(bad.sum())} keep decisions in {rows.numel()} rows differ from Philox4x32-10; first row "
                             f"{int(rows[0])}, last row {int(rows[-1])}")
    rate = float(keep.float().mean())
    assert abs(rate - 0.5) < 0.01, f"{name}: keep rate {rate} (broken test)"


def check_close(name, got, ref, tol):
    """|got - ref| <= tol, every element (a NaN fails)"""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    if bool(bad.any()):
        rows = bad.reshape(bad.shape[0], -1).any(1).nonzero().reshape(-1)
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} values over the bound; first row {int(rows[0])}, last row "
                             f"{int(rows[-1])}, worst excess {float((err - tol)[bad].max())}, worst error {float(err.max())}")


def check_rel(name, got, ref, bound):
    rel = float((got.double() - ref).norm() / ref.norm().clamp_min(1e-300))
    assert rel <= bound, f"{name}: relative error {rel} > {bound}"


def check_per_element(name, got, ref, f32_abs=None, f32_rel=None):
    """the project's bars: 0.51 ulp(bf16) + 1e-5 on a bf16 output; on an fp32 one an absolute or a relative (norm) bar"""
    if got.dtype == BF16:
        check_close(name, got, ref, 0.51 * ulp_bf16(ref) + 1e-5)
    elif f32_abs is not None:
        check_close(name, got, ref, torch.full_like(ref, f32_abs))
    else:
        check_rel(name, got, ref, f32_rel)


# ------------------------------------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _restore_env():
    yield
    if os.environ.pop("SGF_EW8", None) is not None:
        _L().load().sgf_reload_env()


class Run(Operands):
    """One case on the device: operands and outputs laid out as its path says"""

    def __init__(self, path, device):
        super().__init__(device)
        self.path = path
        self.dtype, self.extra, self.gap, env = PATHS[path]
        if env is not None:
            os.environ["SGF_EW8"] = env
            _L().load().sgf_reload_env()
        self.code = _L().SGF_BF16 if self.dtype == BF16 else _L().SGF_F32
        self.guards = []

    def rows(self, name, t):
        view = self.up(name, t, extra_cols=self.extra, dtype=self.dtype)
        buf = self.bufs[name][0]
        assert buf.shape == (t.shape[0] + PAD_ROWS, t.shape[1] + self.extra) and float(buf[-1, -1]) == POISON
        return view

    def out(self, n, width, dtype=None, gap=None):
        g = Guarded(n, width, dtype or self.dtype, self.device, gap=self.gap if gap is None else gap)
        self.guards.append(g)
        return g

    def vec(self, n, dtype=F32):
        """a vector output of n elements with TAIL_ELEMS sentinels behind it"""
        buf = torch.full((n + TAIL_ELEMS,), SENTINEL, dtype=dtype, device=self.device)
        self.guards.append(_VecGuard(buf, n))
        return buf[:n]

    def workspace(self, nbytes):
        o = Opaque(max(int(nbytes), 16), self.device)
        self.guards.append(o)
        return o

    def contract(self):
        assert all(g.intact() for g in self.guards), "a sentinel (column, row, element or workspace byte) was written"
        assert self.operands_untouched(), "an operand, its poisoned rows or its poisoned columns changed"


class _VecGuard:
    def __init__(self, buf, n):
        self.buf, self.n = buf, n

    def intact(self):
        return bool((self.buf[self.n:] == SENTINEL).all())


def _consts(k, device):
    return {name: v.to(device) for name, v in k.items()}


# ---- sgf_axpby (k_axpby) ----
AXPBY_CASES = width_cases(WIDTHS, no_wide, narrow=(100,))


@pytest.mark.parametrize("d,path", AXPBY_CASES, ids=_ids)
def test_axpby(cuda, d, path):
    """y = 3 x1 + x2 / 4 with x in {-31 .. 31}: multiples of 1/4 up to 101, more than 8 significant bits, so the rounding to bf16 is real"""
    n, L = path_rows(K_AXPBY, d, path, no_wide), _L()
    r = Run(path, cuda)
    x1, x2 = r.rows("x1", ints(1, n, d, -31, 31)), r.rows("x2", ints(2, n, d, -31, 31))
    y = r.out(n, d)
    L.call("sgf_axpby", _p(x1), _ld(x1), 3.0, _p(x2), _ld(x2), 0.25, n, d, r.code, _p(y.out), _ld(y.out), _st(cuda))
    check_stored("y", y.out, ref_axpby(x1.double(), 3.0, x2.double(), 0.25))
    r.contract()


# ---- sgf_sum_n (k_sum_n, k_sum_n_bf16x8<K>) ----
SUM_CASES = [(d, p, 3) for d, p in width_cases(WIDTHS, ew8_width, narrow=(100,)) if p != "bf16_env"] + \
            [(512, p, k) for p in ("f32", "bf16", "bf16_ld4") for k in SUM_K if k != 3 or p not in MAIN]


@pytest.mark.parametrize("d,path,k", SUM_CASES, ids=_ids)
def test_sum_n(cuda, d, path, k):
    """y = x_1 + ... + x_k of integers in {-127 .. 127} (bf16 values; from k = 3 the sum needs rounding)"""
    n, L = path_rows(K_SUM_N, d, path, ew8_width, reads_env=False), _L()
    r = Run(path, cuda)
    xs = [r.rows(f"x{j}", ints(10 + j, n, d, -127, 127)) for j in range(k)]
    y = r.out(n, d)
    ptrs = (ctypes.c_void_p * k)(*[x.data_ptr() for x in xs])
    lds = (ctypes.c_int64 * k)(*[x.stride(0) for x in xs])
    L.call("sgf_sum_n", ptrs, lds, k, n, d, r.code, _p(y.out), _ld(y.out), _st(cuda))
    ref = xs[0].double()
    for x in xs[1:]:
        ref = ref + x.double()
    check_stored("y", y.out, ref)
    r.contract()


# ---- sgf_gather_rows (k_gather_rows), sgf_pad_rows (k_pad_rows) ----
GATHER_SRC = 5003
GATHER_CASES = [(d, "f32", "f32", 64) for d in WIDTHS + [100]] + [(d, "bf16", "bf16", 32) for d in WIDTHS + [100]] + \
               [(512, "f32", "bf16", 32), (512, "bf16", "f32", 64), (512, "f32", "f32", 32), (512, "bf16", "bf16", 64), (65, "f32", "bf16", 64)]


@pytest.mark.parametrize("d,src_t,dst_t,ibits", GATHER_CASES, ids=_ids)
def test_gather_rows(cuda, d, src_t, dst_t, ibits):
    """out[i] = cast(src[idx[i]]), a zero row for an index outside [0, n_src); d = 65: the element-wise path"""
    L = _L()
    sd, dd = PATHS[src_t][0], PATHS[dst_t][0]
    n = rows_at(lap_rows(K_GATHER, d, sd, 0))
    r = Run(dst_t, cuda)
    src = r.up("src", ints(20, GATHER_SRC, d, -127, 127), extra_cols=4 if d % 4 == 0 else 3, dtype=sd)
    idx = gather_index(d, n, GATHER_SRC, torch.int64 if ibits == 64 else torch.int32).to(cuda)
    keep_idx = idx.clone()
    assert int(((idx < 0) | (idx >= GATHER_SRC)).sum()) > 16, "no index outside [0, n_src) (broken test)"
    out = r.out(n, d, gap=4 if d % 4 == 0 else 3)
    L.call("sgf_gather_rows", _p(src), _ld(src), L.SGF_BF16 if sd == BF16 else L.SGF_F32, GATHER_SRC, _p(idx), int(ibits == 64), n, d,
           _p(out.out), _ld(out.out), r.code, _st(cuda))
    check_stored("out", out.out, ref_gather(src.double(), idx))
    assert torch.equal(idx, keep_idx)
    r.contract()


PAD_CASES = [(65, 68, "f32", "bf16", 64), (65, 68, "bf16", "bf16", 32), (100, 104, "f32", "f32", 0), (100, 104, "f32", "bf16", 32),
             (65, 68, "f32", "f32", 0)]


@pytest.mark.parametrize("d,d_pad,src_t,dst_t,ibits", PAD_CASES, ids=_ids)
def test_pad_rows(cuda, d, d_pad, src_t, dst_t, ibits):
    """out[i, :d] = cast(src[idx ? idx[i] : i, :d]), out[i, d:d_pad] = 0; ibits = 0: no index (n_out = n_src rows in order)"""
    L = _L()
    sd = PATHS[src_t][0]
    n = rows_at(lap_rows(K_PAD, d_pad, sd, 0))
    r = Run(dst_t, cuda)
    n_src = n if ibits == 0 else GATHER_SRC
    src = r.up("src", ints(21, n_src, d, -127, 127), extra_cols=3, dtype=sd)
    idx = None if ibits == 0 else gather_index(d, n, n_src, torch.int64 if ibits == 64 else torch.int32).to(cuda)
    out = r.out(n, d_pad, gap=4)
    L.call("sgf_pad_rows", _p(src), _ld(src), L.SGF_BF16 if sd == BF16 else L.SGF_F32, n_src, _p(idx), int(ibits == 64), n, d, d_pad,
           _p(out.out), _ld(out.out), r.code, _st(cuda))
    check_stored("out", out.out, ref_gather(src.double(), torch.arange(n, device=cuda) if idx is None else idx, d_pad))
    r.contract()


# ---- sgf_dropout / sgf_dropout_dev (k_dropout) ----
DROP_CASES = [(d, p, True, False) for d, p in width_cases(WIDTHS, no_wide, narrow=(100,))] + \
             [(512, p, res, dev) for p in MAIN for res, dev in ((False, False), (True, True), (False, True))]


@pytest.mark.parametrize("d,path,use_res,dev_seed", DROP_CASES, ids=_ids)
def test_dropout(cuda, d, path, use_res, dev_seed):
    """p = 1/2: y = 2 x keep (+ res), the keep pattern of the WHOLE tensor against Philox4x32-10, and the backward (the same call
    on the gradient, res = NULL) reproducing it; _dev reads the same seed from slot 2 of a bank of four"""
    n, L = path_rows(K_DROPOUT, d, path, no_wide), _L()
    r = Run(path, cuda)
    x, g = r.rows("x", nonzero_ints(30, n, d, 31)), r.rows("g", nonzero_ints(31, n, d, 31))
    res = r.rows("res", ints(32, n, d, -31, 31)) if use_res else None
    bank = torch.tensor([1, 2, SEED - 2 ** 64, 4], dtype=torch.int64, device=cuda)
    bank0 = bank.clone()

    def run(inp, rr):
        y = r.out(n, d)
        if dev_seed:
            L.call("sgf_dropout_dev", _p(inp), _ld(inp), _p(rr), _ld(rr), 0.5, ctypes.c_void_p(bank.data_ptr() + 16), n, d, r.code,
                   _p(y.out), _ld(y.out), _st(cuda))
        else:
            L.call("sgf_dropout", _p(inp), _ld(inp), _p(rr), _ld(rr), 0.5, SEED, n, d, r.code, _p(y.out), _ld(y.out), _st(cuda))
        return y

    y, dg = run(x, res), run(g, None)
    keep = philox_keep(SEED, n, d, 0.5, cuda)
    check_stored("y", y.out, ref_dropout(x.double(), None if res is None else res.double(), keep, 0.5))
    check_stored("dx", dg.out, ref_dropout(g.double(), None, keep, 0.5))
    fwd_kept = (y.out.double() - (res.double() if use_res else 0.0)) != 0
    check_keep("forward", fwd_kept, keep)
    check_keep("backward", dg.out != 0, keep)
    assert torch.equal(bank, bank0)
    r.contract()


# ---- sgf_ln_fwd / sgf_ln_bwd with gamma = NULL (k_ln_fwd, k_ln_bwd, k_ln_*_bf16x8: the residual mix and relu alone) ----
LN_WIDE_WIDTHS = WIDTHS
LN_PLAIN_FLAGS = [(True, True), (False, True), (True, False), (False, False)]
LN_PLAIN_CASES = case_list(WIDTHS, ln8_width, LN_PLAIN_FLAGS, narrow=(100, 768, 1024))


def ln_rows(d, path):
    """N of a LayerNorm case: from the longer of the forward's and the backward's lap (they differ only under SGF_EW8=0)"""
    return max(path_rows(K_LN_FWD, d, path, ln8_width, reads_env=False), path_rows(K_LN_BWD, d, path, ln8_width))


@pytest.mark.parametrize("d,path,relu,use_res", LN_PLAIN_CASES, ids=_ids)
def test_ln_without_gamma(cuda, d, path, relu, use_res):
    """y = [relu](3/2 x + res / 8) (multiples of 1/8 up to 51: 9 and more bits) and dx = 3/2 dz, dres = dz / 8 with dz = dy where y > 0;
    mean / rstd are NULL and no workspace is touched"""
    n, L = ln_rows(d, path), _L()
    a, b = 1.5, 0.125
    r = Run(path, cuda)
    x, gy = r.rows("x", ints(40, n, d, -31, 31)), r.rows("gy", ints(41, n, d, -31, 31))
    res = r.rows("res", ints(42, n, d, -31, 31)) if use_res else None
    y = r.out(n, d)
    L.call("sgf_ln_fwd", _p(x), _ld(x), _p(res), _ld(res), a, b, None, None, int(relu), LN_EPS, n, d, r.code, _p(y.out), _ld(y.out),
           None, None, _st(cuda))
    ref = ref_ln_plain(x.double(), None if res is None else res.double(), a, b, relu)
    check_stored("y", y.out, ref)
    dx, dres = r.out(n, d), (r.out(n, d) if use_res else None)
    dro = None if dres is None else dres.out
    ws = r.workspace(0)
    L.call("sgf_ln_bwd", _p(gy), _ld(gy), _p(y.out), _ld(y.out), _p(x), _ld(x), _p(res), _ld(res), a, b, None, int(relu), None, None, n,
           d, r.code, _p(dx.out), _ld(dx.out), _p(dro), _ld(dro), None, None, _p(ws.buf), 0, _st(cuda))
    rdx, rdres = ref_ln_plain_bwd(gy.double(), y.out.double(), a, b, relu)
    check_stored("dx", dx.out, rdx)
    if use_res:
        check_stored("dres", dres.out, rdres)
    r.contract()


# ---- sgf_ln_fwd / sgf_ln_bwd with gamma, against fp64 of the stored inputs ----
LN_FLAGS = [(True, True, 0.5, 0.5), (False, True, 0.3, 0.7), (True, False, 1.0, 0.0)]
LN_CASES = case_list(WIDTHS, ln8_width, LN_FLAGS, narrow=(100, 768, 1024))


def _ln_inputs(cuda, n, d, seed):
    g = torch.Generator(device=cuda).manual_seed(seed)
    rows = lambda: torch.randn(n, d, device=cuda, generator=g) * 1.5 + 0.3     # noqa: E731
    x, res, gy = rows(), rows(), rows()
    gamma = torch.rand(d, device=cuda, generator=g) + 0.5
    beta = torch.randn(d, device=cuda, generator=g) * 0.1
    return x, res, gy, gamma, beta


def _ln_fwd(cuda, r, n, d, relu, a, b, x, res, gamma, beta):
    """sgf_ln_fwd on operands already on the device in r's layout: (y, mean, rstd)"""
    y, mean, rstd = r.out(n, d), r.vec(n), r.vec(n)
    _L().call("sgf_ln_fwd", _p(x), _ld(x), _p(res), _ld(res), a, b, _p(gamma), _p(beta), int(relu), LN_EPS, n, d, r.code, _p(y.out),
              _ld(y.out), _p(mean), _p(rstd), _st(cuda))
    return y.out, mean, rstd


def _ln_bwd(cuda, r, n, d, relu, use_res, a, b, x, res, gy, gamma, y, mean, rstd):
    """sgf_ln_bwd from a forward's stored y, mean and rstd: (dx, dres, dgamma, dbeta)"""
    L = _L()
    dx, dres = r.out(n, d), (r.out(n, d) if use_res else None)
    dro = None if dres is None else dres.out
    dgamma, dbeta = r.vec(d), r.vec(d)
    ws = r.workspace(L.load().sgf_ln_bwd_workspace_bytes(n, d))
    L.call("sgf_ln_bwd", _p(gy), _ld(gy), _p(y), _ld(y), _p(x), _ld(x), _p(res), _ld(res), a, b, _p(gamma), int(relu), _p(mean),
           _p(rstd), n, d, r.code, _p(dx.out), _ld(dx.out), _p(dro), _ld(dro), _p(dgamma), _p(dbeta), _p(ws.buf), ws.nbytes, _st(cuda))
    return dx.out, dro, dgamma, dbeta


@pytest.mark.parametrize("d,path,relu,use_res,a,b", LN_CASES, ids=_ids)
def test_ln_with_gamma(cuda, d, path, relu, use_res, a, b):
    n = ln_rows(d, path)
    r = Run(path, cuda)
    x, res, gy, gamma, beta = _ln_inputs(cuda, n, d, 17 * d + len(path))
    x, gy = r.up("x", x, r.extra, r.dtype), r.up("gy", gy, r.extra, r.dtype)
    res = r.up("res", res, r.extra, r.dtype) if use_res else None
    y, mean, rstd = _ln_fwd(cuda, r, n, d, relu, a, b, x, res, gamma, beta)
    dx, dres, dgamma, dbeta = _ln_bwd(cuda, r, n, d, relu, use_res, a, b, x, res, gy, gamma, y, mean, rstd)
    x64, r64 = x.double(), (None if res is None else res.double())
    # ---- forward: fp64 of the stored x, res ----
    ry, rmean, rrstd, pre = ref_ln(x64, r64, a, b, gamma.double(), beta.double(), relu)
    check_per_element("y", y, ry, f32_abs=2e-5)
    e_mean, e_rstd = ln_stat_bounds(x64, r64, a, b, pre, rmean, rrstd)
    check_close("mean", mean, rmean, e_mean)
    check_close("rstd", rstd, rrstd, e_rstd)
    # ---- backward: fp64 of the stored dy, y (the relu mask), x, res, mean, rstd ----
    rdx, rdres, rdgamma, rdbeta, dz, xh = ref_ln_bwd(gy.double(), y.double(), pre, a, b, gamma.double(), relu, mean.double(), rstd.double())
    check_per_element("dx", dx, rdx, f32_rel=1e-5)
    if use_res:
        check_per_element("dres", dres, rdres, f32_rel=1e-5)
    # dbeta: the terms dz are stored values (exact), only the chain of additions rounds.  dgamma: a term dz xhat carries five
    # more roundings (a x, its fma, - mean, * rstd, * dz), the first two relative to |a x| + |b res| rather than to |xhat|.
    chain = ln_chain(n, d, runs_wide(path, d, ln8_width))
    mag = (a * x64).abs() if r64 is None else (a * x64).abs() + (b * r64).abs()
    terms = dz.abs() * rstd.double()[:, None] * (mag + mean.double().abs()[:, None])
    check_close("dbeta", dbeta, rdbeta, chain * EPS32 * dz.abs().sum(0))
    check_close("dgamma", dgamma, rdgamma, (chain + 5) * EPS32 * torch.maximum(terms, (dz * xh).abs()).sum(0))
    r.contract()


@pytest.mark.parametrize("d", LN_WIDE_WIDTHS)
def test_ln_bf16_kernels_agree(cuda, d):
    """k_ln_fwd_bf16x8 / k_ln_bwd_bf16x8 and the 8-byte kernels on the same rows (past two laps of the 16-byte kernels): they differ
    in the order of a row's sums only — one bf16 step at most (values near zero: the fp32 noise), rarely"""
    n = ln_rows(d, "bf16")
    x, res, gy, gamma, beta = _ln_inputs(cuda, n, d, 23 * d)
    fwd, bwd = {}, {}
    for path in ("bf16", "bf16_ld4"):
        r = Run(path, cuda)
        xs, rs, gs = (r.up(name, t, r.extra, r.dtype) for name, t in (("x", x), ("res", res), ("gy", gy)))
        fwd[path] = _ln_fwd(cuda, r, n, d, True, 0.5, 0.5, xs, rs, gamma, beta)
        # both backward kernels from the SAME forward (the 16-byte one's): a y that is a rounding away from zero in one forward
        # and zero in the other would flip a relu mask, which is not a difference between the backward kernels
        y, mean, rstd = fwd["bf16"]
        ys = y if path == "bf16" else r.up("y", y, r.extra, r.dtype)
        bwd[path] = _ln_bwd(cuda, r, n, d, True, True, 0.5, 0.5, xs, rs, gs, gamma, ys, mean, rstd)
        r.contract()
    pairs = [("y", fwd["bf16"][0], fwd["bf16_ld4"][0]), ("dx", bwd["bf16"][0], bwd["bf16_ld4"][0]),
             ("dres", bwd["bf16"][1], bwd["bf16_ld4"][1])]
    for name, w, s in pairs:
        w, s = w.double(), s.double()
        check_close(name, w, s, 1.01 * ulp_bf16(torch.maximum(w.abs(), s.abs())) + 1e-4)
        assert float((w != s).double().mean()) <= 0.02, name


# ---- sgf_bn_apply / sgf_bn_bwd_apply (k_bn_apply, k_bn_bwd_apply, k_bn_*_bf16x8) ----
BN_APPLY_CASES = case_list(WIDTHS, ew8_width, [(True, True), (False, False), (True, False), (False, True)], narrow=(100,), wide_only=(104,))
BN_BWD_CASES = case_list(WIDTHS, ew8_width, [(True, True), (False, True), (True, False), (False, False)], narrow=(100,), wide_only=(104,))


@pytest.mark.parametrize("d,path,relu,use_res", BN_APPLY_CASES, ids=_ids)
def test_bn_apply(cuda, d, path, relu, use_res):
    """y = [relu]((x - mean) rstd gamma + beta) [+ res] with rstd, gamma powers of two, mean a multiple of 1/4, beta of 1/2 and
    x, res in {-31 .. 31}: every intermediate is a multiple of 1/16 below 2^7, whatever is contracted; y has up to 11 bits"""
    n, L = path_rows(K_BN_APPLY, d, path, ew8_width), _L()
    r = Run(path, cuda)
    k = _consts(bn_coefs(d, 0), cuda)
    x = r.rows("x", ints(50, n, d, -31, 31))
    res = r.rows("res", ints(51, n, d, -31, 31)) if use_res else None
    y = r.out(n, d)
    L.call("sgf_bn_apply", _p(x), _ld(x), _p(k["mean"]), _p(k["rstd"]), _p(k["gamma"]), _p(k["beta"]), _p(res), _ld(res), int(relu), n, d,
           r.code, _p(y.out), _ld(y.out), _st(cuda))
    check_stored("y", y.out, ref_bn_apply(x.double(), k, None if res is None else res.double(), relu))
    r.contract()


@pytest.mark.parametrize("d,path,relu,training", BN_BWD_CASES, ids=_ids)
def test_bn_bwd_apply(cuda, d, path, relu, training):
    """dx = gamma rstd (g' - stats0 inv_n - xhat stats1 inv_n): with bn_coefs' constants and inv_n = 2^-18 the two coefficients
    are multiples of 1/4 and 1/16, xhat a multiple of 1/8 up to 32, the bracket a multiple of 1/128 below 64: 13 bits"""
    n, L = path_rows(K_BN_BWD_APPLY, d, path, ew8_width), _L()
    r = Run(path, cuda)
    k = _consts(bn_coefs(d, 1), cuda)
    x, gy = r.rows("x", ints(52, n, d, -31, 31)), r.rows("gy", ints(53, n, d, -31, 31))
    dx = r.out(n, d)
    L.call("sgf_bn_bwd_apply", _p(gy), _ld(gy), _p(x), _ld(x), _p(k["mean"]), _p(k["rstd"]), _p(k["gamma"]), _p(k["beta"]), int(relu),
           _p(k["stats"]), INV_N, int(training), n, d, r.code, _p(dx.out), _ld(dx.out), _st(cuda))
    check_stored("dx", dx.out, ref_bn_bwd_apply(gy.double(), x.double(), k, relu, training))
    r.contract()


# ---- the blocked column reductions: sgf_colstats, sgf_bn_bwd_stats / _stats2 (k_colreduce, k_bn_bwd_stats_bf16x8), sgf_colsum ----
COLSTATS_CASES = width_cases(WIDTHS, no_wide, narrow=(100,))


@pytest.mark.parametrize("n", STAT_ROWS)
@pytest.mark.parametrize("d,path", COLSTATS_CASES, ids=_ids)
def test_colstats(cuda, n, d, path):
    """[sum (x - shift) | sum (x - shift)^2] of x in {-3 .. 3}, shift in {-1, 0, 1}: integers below 2^24, with and without shift"""
    L = _L()
    r = Run(path, cuda)
    x = r.rows("x", ints(60, n, d, -3, 3))
    shift = torch.randint(-1, 2, (d,), generator=torch.Generator().manual_seed(d)).float().to(cuda)
    x64 = x.double()
    for sh in (shift, None):
        stats = r.vec(2 * d)
        ws = r.workspace(L.load().sgf_colstats_workspace_bytes(n, d))
        L.call("sgf_colstats", _p(x), _ld(x), _p(sh), n, d, r.code, _p(stats), _p(ws.buf), ws.nbytes, _st(cuda))
        v = x64 if sh is None else x64 - sh.double()
        check_sums("stats", stats, ref_colstats(x64, None if sh is None else sh.double()),
                   max(float(v.abs().sum(0).max()), float((v * v).sum(0).max())))
    r.contract()


BN_STATS_CASES = [(d, p, True, False) for d, p in width_cases(WIDTHS, ew8_width, narrow=(100,))] + \
                 [(512, p, relu, two) for p in MAIN for relu, two in ((True, True), (False, False), (False, True))]


@pytest.mark.parametrize("n", STAT_ROWS)
@pytest.mark.parametrize("d,path,relu,two", BN_STATS_CASES, ids=_ids)
def test_bn_bwd_stats(cuda, n, d, path, relu, two):
    """[sum g' | sum g' xhat] with g, g2, x in {-2 .. 2}: the first integers, the second multiples of 1/8; abs-sums in eighths
    below 2^24 (asserted)"""
    L = _L()
    r = Run(path, cuda)
    k = _consts(bn_coefs(d, 2), cuda)
    x, gy = r.rows("x", ints(61, n, d, -2, 2)), r.rows("gy", ints(62, n, d, -2, 2))
    gy2 = r.rows("gy2", ints(63, n, d, -2, 2)) if two else None
    stats = r.vec(2 * d)
    ws = r.workspace(L.load().sgf_colstats_workspace_bytes(n, d))
    head = (_p(gy), _ld(gy))
    tail = (_p(x), _ld(x), _p(k["mean"]), _p(k["rstd"]), _p(k["gamma"]), _p(k["beta"]), int(relu), n, d, r.code, _p(stats), _p(ws.buf),
            ws.nbytes, _st(cuda))
    if two:
        L.call("sgf_bn_bwd_stats2", *head, _p(gy2), _ld(gy2), *tail)
    else:
        L.call("sgf_bn_bwd_stats", *head, *tail)
    ref, worst = ref_bn_bwd_stats(gy.double(), None if gy2 is None else gy2.double(), x.double(), k, relu)
    check_sums("stats", stats, ref, worst)
    r.contract()


@pytest.mark.parametrize("n", STAT_ROWS)
@pytest.mark.parametrize("path", MAIN)
def test_colsum_any_width(cuda, n, path):
    """out[j] = sum_n x[n, j] at d = 47 (k_colsum_any: 5 row slots per pass, 21 idle threads), rows as a slice of a 50-column buffer"""
    L, d = _L(), 47
    r = Run(path, cuda)
    x = r.up("x", ints(64, n, d, -3, 3), extra_cols=3, dtype=r.dtype)
    out = r.vec(d)
    ws = r.workspace(L.load().sgf_colsum_workspace_bytes(n, d))
    L.call("sgf_colsum", _p(x), _ld(x), n, d, r.code, _p(out), _p(ws.buf), ws.nbytes, _st(cuda))
    check_sums("colsum", out, x.double().sum(0), float(x.double().abs().sum(0).max()))
    r.contract()


# ---- sgf_nll_fwd / sgf_nll_bwd (k_nll_fwd16, k_nll_fwd, k_nll_bwd16, k_nll_bwd) ----
def _nll_device(cuda, r, c, n, m, seed=0):
    arg, labels, idx = (t.to(cuda) for t in nll_case(c, n, m, seed))
    logits = torch.full((n, c), NLL_OFF, dtype=F32, device=cuda)
    logits[torch.arange(n, device=cuda), arg] = 0.0
    lg = r.up("logits", logits, extra_cols=1, dtype=r.dtype)
    assert bool((labels != arg).all())
    return arg, labels, idx, lg


def _nll_fwd(cuda, r, lg, labels, idx, n, c):
    L = _L()
    loss = r.vec(1)
    ws = r.workspace(L.load().sgf_nll_workspace_bytes(idx.numel()))
    L.call("sgf_nll_fwd", _p(lg), _ld(lg), n, c, r.code, _p(labels), _p(idx), idx.numel(), _p(loss), _p(ws.buf), ws.nbytes, _st(cuda))
    return loss


@pytest.mark.parametrize("c", NLL_CLASSES)
@pytest.mark.parametrize("path", MAIN)
def test_nll_onehot_index(cuda, c, path):
    """index tensor (a seeded permutation: a lap seam is not a memory seam), the C entries with a guarded dlogits"""
    L = _L()
    m = rows_at(lap_rows(K_NLL_BWD, c, PATHS[path][0], 0))
    n = m + 4099
    r = Run(path, cuda)
    arg, labels, idx, lg = _nll_device(cuda, r, c, n, m)
    labels0, idx0 = labels.clone(), idx.clone()
    loss = _nll_fwd(cuda, r, lg, labels, idx, n, c)
    gout = torch.ones(1, dtype=F32, device=cuda)
    dl = r.out(n, c, gap=1)
    L.call("sgf_nll_bwd", _p(lg), _ld(lg), n, c, r.code, _p(labels), _p(idx), m, _p(gout), NLL_INV_DENOM, _p(dl.out), _ld(dl.out),
           _st(cuda))
    want_loss, want_g = ref_nll_onehot(arg, labels, idx, c, NLL_INV_DENOM, n)
    assert 0 < want_loss < EXACT * 128 and want_loss < -NLL_OFF * m, "some labels must be outside [0, c) (broken test)"
    assert float(loss[0]) == want_loss, (float(loss[0]), want_loss)
    check_stored("dlogits", dl.out, want_g)
    assert torch.equal(labels, labels0) and torch.equal(idx, idx0)
    r.contract()


@pytest.mark.parametrize("c", NLL_CLASSES)
@pytest.mark.parametrize("path", MAIN)
def test_nll_onehot_mask(cuda, c, path):
    """bool mask through sgformer_amd.loss.log_softmax_nll with an explicit power-of-two divisor: loss * denom = 128 per valid
    training row exactly, and the gradient of the mean"""
    from sgformer_amd.loss import log_softmax_nll
    m = rows_at(lap_rows(K_NLL_BWD, c, PATHS[path][0], 0))
    n = m + 4099
    r = Run(path, cuda)
    arg, labels, idx, lg = _nll_device(cuda, r, c, n, m, seed=1)
    mask = torch.zeros(n, dtype=torch.bool, device=cuda)
    mask[idx] = True
    leaf = lg.detach().clone().requires_grad_(True)
    denom = 2 ** 16
    loss = log_softmax_nll(leaf, labels.reshape(n, 1), mask, denom=denom)
    loss.backward()
    want_loss, want_g = ref_nll_onehot(arg, labels, mask.nonzero().view(-1), c, 1.0 / denom, n)
    got_loss = float(loss.detach())
    assert got_loss * denom == want_loss, (got_loss * denom, want_loss)
    check_stored("dlogits", leaf.grad, want_g)
    r.contract()


@pytest.mark.parametrize("m", NLL_FWD_ROWS)
@pytest.mark.parametrize("c,path", [(47, "f32"), (47, "bf16"), (172, "f32"), (172, "bf16")], ids=_ids)
def test_nll_fwd_blocked(cuda, m, c, path):
    """sgf_nll_fwd past its grid cap: m = 65 537 gives 65 training rows per workgroup and leaves workgroups 1009 .. 1023 empty"""
    n = m + 4099
    r = Run(path, cuda)
    arg, labels, idx, lg = _nll_device(cuda, r, c, n, m, seed=2)
    loss = _nll_fwd(cuda, r, lg, labels, idx, n, c)
    want_loss, _ = ref_nll_onehot(arg, labels, idx, c, 1.0, n)
    assert float(loss[0]) == want_loss, (float(loss[0]), want_loss)
    r.contract()


@pytest.mark.parametrize("c", [47, 172])
@pytest.mark.parametrize("path", MAIN)
def test_nll_random_logits(cuda, c, path):
    """random logits against fp64 of the stored logits, under test_fused_loss's bars"""
    from sgformer_amd.loss import log_softmax_nll
    dtype = PATHS[path][0]
    m = rows_at(lap_rows(K_NLL_BWD, c, dtype, 0))
    n = m + 4099
    g = torch.Generator(device=cuda).manual_seed(c)
    logits = (torch.randn(n, c, device=cuda, generator=g) * 3).to(dtype)
    y = torch.randint(0, c, (n, 1), device=cuda, generator=g)
    idx = torch.randperm(n, device=cuda, generator=g)[:m]
    ld = logits.double().requires_grad_(True)
    ref = -torch.log_softmax(ld, 1)[idx, y.view(-1)[idx]].mean()
    ref.backward()
    lg = logits.clone().requires_grad_(True)
    loss = log_softmax_nll(lg, y, idx)
    loss.backward()
    got_loss, want = float(loss.detach()), float(ref.detach())
    assert abs(got_loss - want) <= 2e-6 * abs(want) + 1e-6, (got_loss, want)
    check_rel("dlogits", lg.grad.float(), ld.grad, 2e-6 if dtype == F32 else 5e-3)
    off = torch.ones(n, dtype=torch.bool, device=cuda)
    off[idx] = False
    assert torch.count_nonzero(lg.grad[off]) == 0
