"""The persistent bf16 row kernels where ONE wave walks SEVERAL tiles (csrc/rowgemm.hip: k_rowgemm_bf16, k_rowgemm2_bf16,
k_dx2acc_bf16, k_bn_bwd_dx_bf16, k_stem_bf16; csrc/head.hip: k_head_fwd_bf16, k_head_bwd_bf16).

Every wave of these kernels streams 32-row tiles t, t + waves, ... and requests the next tile (k_head_bwd_bf16: the next two)
while it works on the current one; `cur = nxt`, the 4-slot fragment ring of k_bn_bwd_dx_bf16 that refills "with step s + RING
of this tile or of the next one" and the raw_nxt / row_nn hand-over of the head backward run only when a wave HAS a second
and a third tile.  Every case here runs N = 3 * 65 536 + 5 rows = 6145 tiles (the head forward, whose lap is twice as long,
N = 3 * 131 072 + 5).  Rows one lap of all waves covers at the grid cap (sgf_row_lap_rows) and tiles per wave at N:
    kind  entry                                   d = 64          d = 128         d = 256
    0     gcn_epilogue_stats / dx / partial / add  65 536: 3-4     65 536: 3-4     65 536: 3-4
    1     gcn_epilogue_dx2, paired                 32 768: 6-7     32 768: 6-7     32 768: 6-7
    2     gcn_epilogue_dx2_acc                     65 536: 3-4     65 536: 3-4     32 768: 6-7
    3     gcn_bn_bwd_dx                            65 536: 3-4     32 768: 6-7     16 384: 12-13
    4     gcn_epilogue_cat                         65 536: 3-4     65 536: 3-4     32 768: 6-7
    5     stem_pair (d = d_out)                    65 536: 3-4                     65 536: 3-4
    6     combine_fc_fwd (N = 393 221)            131 072: 3-4    131 072: 3-4    131 072: 3-4
    7     combine_fc_bwd                           65 536: 3-4     65 536: 3-4     65 536: 3-4
("3-4": exactly one wave gets a fourth tile, the ragged one of five rows.)  tests/test_row_laps_host.py asserts this from the
library's own query, so a retuned grid fails there instead of thinning this file out.

Everything is pinned BIT FOR BIT.  The operands are small integers (times powers of two), so every product and every partial
sum in any order is an fp32 value and the fp64 reference, rounded to bf16 ONCE where the kernel stores bf16, must be
reproduced exactly; a stale tile, one dropped or doubled row in the column statistics, or a second rounding changes a value
and no tolerance hides it.  Each test asserts its precondition from the data first (the reference before its rounding is an
fp32 value; the worst abs-sum behind a statistic, in units of its quantum, is below 2^24).  No stage needed the per-element
bound of tests/test_gpu_attn_laps.py.

The references are the formulas of include/sgf.h as plain torch code, run in fp64 on the device here and against
tests/cpu_kernels.py and oracle/sgformer_oracle.py on the CPU in tests/test_row_laps_host.py.  Memory contract, in the same
calls: streamed operands carry 64 poisoned rows behind row N (and 8 poisoned columns where they are column slices) and must be
unchanged; row-major outputs are written between sentinel columns and in front of sentinel rows (the C entries are called
directly for that: the kernels.py wrappers allocate their outputs); the opaque accumulator buffers carry sentinel bytes
behind sgf_gcn_epilogue_partial_bytes.
"""
import ctypes
import functools
import os

import pytest
import torch

from tests.test_gpu_attn_laps import EXACT, PAD_ROWS, POISON, SENTINEL, _tri, check_exact

pytestmark = pytest.mark.gpu

N = 3 * 65536 + 5            # every rowgemm entry and the head backward
N_FWD = 3 * 131072 + 5       # the head forward: 1024 workgroups x 4 waves
WIDTHS = [64, 128, 256]
STEM = [(100, 64), (128, 256), (100, 256), (128, 64)]      # (f, d); f = 100: rows of x are only 8-byte aligned
HEAD = [(256, 47), (128, 64), (64, 7)]                     # (d, classes)
HEAD_AB = [(0.5, 0.5), (0.75, 0.25)]                       # a x1 + b x2 of integers in {-2 .. 2} is a bf16 value
GAP = 8                      # sentinel columns around a row-major output (16 bytes in bf16: the outputs stay 16-byte aligned)
TAIL = 256                   # sentinel bytes behind an opaque accumulator buffer
TAIL_BYTE = 0xA5
INV_N = 2.0 ** -18           # sgf_gcn_bn_bwd_dx's inv_n: a free argument, a power of two near 1 / N
DZ_UNITS = 512               # dz of sgf_gcn_bn_bwd_dx is a multiple of 1 / DZ_UNITS (bn_coefs)
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def rnd(x):
    """rounded ONCE to bf16 (round to nearest even), in x's own dtype"""
    return x.float().bfloat16().to(x.dtype)


# ------------------------------------------------------------------------------------------------------------------------------
# host builders (seeded, integer-valued)
# ------------------------------------------------------------------------------------------------------------------------------
class Case:
    pass


def build_case(d, n=N):
    """Operands of the rowgemm entries at width d.  int8 streamed operands, fp32 constants.
    a  [n, 2 d]  ternary, nonzero with probability 1/4: a1 = a[:, :d], a2 = a[:, d:] of the Linear forms (with the ternary ws of
                 density 1/4, y = a1 W1^T is an integer of variance d / 16: sum (y - shift)^2 over n rows stays below 2^24)
    g  [n, 2 d]  uniform in {-2 .. 2}: dy / dz = g[:, :d] and gadd = g[:, d:] of the gradient forms; gy and z of bn_bwd_dx
    ai [n, d]    ternary, nonzero with probability 1/2: acc_in of dx2_acc
    ws [d, 2 d]  ternary (density 1/4): the Linear forms;  wg [d, 2 d] uniform in {-31 .. 31}: dx / dx2 / dx2_acc, whose results
                 reach several hundred, so their rounding to bf16 is a real one;  wd [d, 2 d] uniform in {-3 .. 3}: bn_bwd_dx
                 (its dz already carries up to 13 bits);  bias in {-2 .. 2}, shift in {-1, 0, 1}"""
    c = Case()
    gen = torch.Generator().manual_seed(104729 + d)
    c.d, c.n = d, n
    c.a = _tri(gen, (n, 2 * d), 8)
    c.g = torch.randint(-2, 3, (n, 2 * d), generator=gen, dtype=torch.int8)
    c.ai = _tri(gen, (n, d), 4)
    c.ws = _tri(gen, (d, 2 * d), 8).float()
    c.wd = torch.randint(-3, 4, (d, 2 * d), generator=gen).float()
    c.wg = torch.randint(-31, 32, (d, 2 * d), generator=gen).float()
    c.bias = torch.randint(-2, 3, (d,), generator=gen).float()
    c.shift = torch.randint(-1, 2, (d,), generator=gen).float()
    c.bn = [bn_coefs(d, i) for i in range(3)]
    return c


def bn_coefs(d, call):
    """BatchNorm constants of one sgf_gcn_bn_bwd_dx call: rstd in {1/2, 1} and gamma in {1/2, 1, 2} (powers of two), mean a
    multiple of 1/4 and beta one of 1/2 in [-1, 1], stats = [sum g' | sum g' xhat] integers times a power of two so that
    k0 = stats INV_N is a multiple of 1/4 in [-1, 1] and k1 a multiple of 1/16 in [-1/2, 1/2].  The prologue of
    k_bn_bwd_dx_bf16 then forms, all exactly (a power of two times a number of at most 8 bits): m = -mean rstd (multiples of
    1/8), T1 = rstd gamma, T0 = m gamma + beta (1/16), cs = gamma rstd in [1/4, 2], Z1 = -cs k1 rstd (1/128),
    Z0 = -cs (k0 + k1 m) (k1 m: 1/128, the sum: 1/128 below 2, Z0: 1/512); with g and z integers in {-2 .. 2}
    act = fma(z, T1, T0) and dz = fma(cs, g', fma(z, Z1, Z0)) are multiples of 1/512 below 16: fp32 values whatever is
    contracted, and up to 13 significant bits, so the rounding of dz to bf16 is a real one."""
    gen = torch.Generator().manual_seed(7 * d + call)
    pick = lambda vals: torch.tensor(vals)[torch.randint(0, len(vals), (d,), generator=gen)].float()   # noqa: E731
    k = {"rstd": pick([0.5, 1.0]), "gamma": pick([0.5, 1.0, 2.0]),
         "mean": torch.randint(-4, 5, (d,), generator=gen).float() / 4, "beta": torch.randint(-2, 3, (d,), generator=gen).float() / 2}
    k["stats"] = torch.cat([torch.randint(-4, 5, (d,), generator=gen) * 4, torch.randint(-8, 9, (d,), generator=gen)]).float() * 2.0 ** 14
    return k


@functools.lru_cache(maxsize=1)
def get_case(d):
    return build_case(d)


def build_stem(f, d, n=N):
    """x [n, f] and both weight matrices [d, f] ternary of density 1/4 (y an integer of variance f / 16), integer biases, shift"""
    c = Case()
    gen = torch.Generator().manual_seed(15485863 + 1000 * f + d)
    c.f, c.d, c.n = f, d, n
    c.x = _tri(gen, (n, f), 8)
    c.w0, c.w1 = _tri(gen, (d, f), 8).float(), _tri(gen, (d, f), 8).float()
    c.b0, c.b1 = (torch.randint(-2, 3, (d,), generator=gen).float() for _ in range(2))
    c.shift = torch.randint(-1, 2, (d,), generator=gen).float()
    return c


def build_head(d, classes, n_fwd=N_FWD, n_bwd=N):
    """x1, x2 [n_fwd, d] uniform in {-2 .. 2}; W [classes, d] in {-3 .. 3} and an integer bias (fp32: the kernels round W to
    bf16 themselves); dlogits [n_bwd, classes] in {-2 .. 2}; one seeded permutation per row count"""
    c = Case()
    gen = torch.Generator().manual_seed(32452843 + 100 * d + classes)
    c.d, c.c, c.n_fwd, c.n_bwd = d, classes, n_fwd, n_bwd
    c.x = torch.randint(-2, 3, (n_fwd, 2 * d), generator=gen, dtype=torch.int8)
    c.w = torch.randint(-3, 4, (classes, d), generator=gen).float()
    c.bias = torch.randint(-4, 5, (classes,), generator=gen).float()
    c.dl = torch.randint(-2, 3, (n_bwd, classes), generator=gen, dtype=torch.int8)
    c.map_fwd = torch.randperm(n_fwd, generator=gen).to(torch.int32)
    c.map_bwd = torch.randperm(n_bwd, generator=gen).to(torch.int32)
    return c


# ------------------------------------------------------------------------------------------------------------------------------
# references: the formulas of include/sgf.h.  Plain torch in the operands' dtype (fp64 everywhere but the host file's full-N
# precondition pass, which uses fp32 where the values are integers below 2^24)
# ------------------------------------------------------------------------------------------------------------------------------
def ref_linear(a, w, bias=None):
    """y = a W^T + bias"""
    y = a @ w.T
    return y if bias is None else y + bias


def ref_stats(y, shift=None):
    """[sum_i (y_ij - shift_j) | sum_i (y_ij - shift_j)^2] of the ROUNDED y"""
    v = rnd(y) if shift is None else rnd(y) - shift
    return torch.cat([v.sum(0), (v * v).sum(0)])


def stats_abs_sum(y, shift=None):
    """worst abs-sum behind a statistic, in units of one (the values are integers; asserted)"""
    v = rnd(y) if shift is None else rnd(y) - shift
    assert bool((v == v.round()).all()), "y - shift is not integer-valued (broken test)"
    return float(max(v.abs().sum(0).max(), (v * v).sum(0).max()))


def ref_two_pass(a1, a2, w, bias=None):
    """sgf_gcn_epilogue_partial + _stats_add: a2 W2^T + round(a1 W1^T + bias), before its own rounding"""
    d = a1.shape[1]
    return a2 @ w[:, d:].T + rnd(ref_linear(a1, w[:, :d], bias))


def ref_cat(a1, a2, w, bias=None):
    """sgf_gcn_epilogue_cat: [a1 | a2] W^T + bias, rounded once"""
    d = a1.shape[1]
    y = a1 @ w[:, :d].T + a2 @ w[:, d:].T
    return y if bias is None else y + bias


def ref_dx(dy, w):
    """dx = dy W"""
    return dy @ w


def ref_dx2_acc(dz, w, gadd=None, acc_in=None):
    """(dz W[:, :d],  round(dz W[:, d:]) + gadd + acc_in): the second product is rounded before the addends (k_dx2acc_bf16
    takes it back from the staging patch) and the sum once more"""
    d = dz.shape[1]
    acc = rnd(dz @ w[:, d:])
    if gadd is not None:
        acc = acc + gadd
    if acc_in is not None:
        acc = acc + acc_in
    return dz @ w[:, :d], acc


def ref_bn_bwd(gy, z, k, relu, training, inv_n=INV_N):
    """dz of sgf_gcn_bn_bwd_dx (= sgf_bn_bwd_apply) before its rounding:
    gamma rstd (g' - stats[:d] inv_n - xhat stats[d:] inv_n),  xhat = (z - mean) rstd,  g' = gy where xhat gamma + beta > 0"""
    d = z.shape[1]
    t = lambda v: v.to(z)                                     # noqa: E731
    xh = (z - t(k["mean"])) * t(k["rstd"])
    g = gy * ((xh * t(k["gamma"]) + t(k["beta"])) > 0) if relu else gy
    if training:
        g = g - t(k["stats"][:d]) * inv_n - xh * t(k["stats"][d:]) * inv_n
    return t(k["gamma"]) * t(k["rstd"]) * g


def ref_bn_chain(gy, z, w, coefs, relu, training, add_gy):
    """the three chained calls: per call (dz, dy = round(dz) W[:, :d]) before rounding, and the running sum
    t_i = round(t_(i-1)) + round(dz_i) W[:, d:] (+ gy) before ITS rounding"""
    d = z.shape[1]
    out, run = [], None
    for k, add in zip(coefs, add_gy):
        dz = ref_bn_bwd(gy, z, k, relu, training)
        dzr = rnd(dz)
        acc = dzr @ w[:, d:]
        if add:
            acc = acc + gy
        if run is not None:
            acc = acc + rnd(run)
        out.append((dz, dzr @ w[:, :d], acc))
        run = acc
    return out


def ref_head_fwd(x1, a, x2, b, w, bias):
    """logits = (a x1 + b x2) W^T + bias; the combined row (returned too) is rounded once before the product"""
    xc = a * x1 + b * x2
    return rnd(xc) @ w.T + bias, xc


def ref_head_bwd(g, w, a, b):
    """dx1 = a (g W), dx2 = b (g W) before their rounding"""
    dx = g @ w
    return a * dx, b * dx


def wave_tile_rows(lap_rows, wave, lap, n):
    """rows of the tile that wave `wave` of a kernel with `lap_rows` rows per lap takes on lap `lap` (0-based)"""
    t = wave + lap * (lap_rows // 32)
    return slice(min(32 * t, n), min(32 * t + 32, n))


def check_bf16(name, got, ref):
    """got (bf16) equals the exact result rounded ONCE; the exact result must be an fp32 value"""
    assert got.dtype == BF16, (name, got.dtype)
    ref32 = ref.float()
    assert torch.equal(ref32.double(), ref.double()), f"{name}: the reference itself is not an fp32 value (broken test)"
    want = ref32.bfloat16()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = got != want
    if bool(bad.any()):
        rows = bad.reshape(bad.shape[0], -1).any(1).nonzero().reshape(-1)
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} values in {rows.numel()} rows differ from the exact result "
                             f"rounded once; first row {int(rows[0])}, last row {int(rows[-1])}, worst |diff| "
                             f"{float((got.double() - want.double()).abs().max())}")


# ------------------------------------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------------------------------------
def _L():
    from sgformer_amd import _lib
    return _lib


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _ld(t):
    return 0 if t is None else t.stride(0)


def _st(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Operands:
    """Streamed operands on the device, each with PAD_ROWS poisoned rows behind its last row (and, for a column slice, the
    poisoned columns of the wider buffer next to it), and a copy to compare with afterwards."""

    def __init__(self, device):
        self.device, self.bufs = device, {}

    def up(self, name, t, extra_cols=0, dtype=BF16, fill=POISON):
        n, w = t.shape
        buf = torch.full((n + PAD_ROWS, w + extra_cols), fill, dtype=dtype, device=self.device)
        buf[:n, :w] = t.to(self.device).to(dtype)
        self.bufs[name] = (buf, buf.clone())
        return buf[:n, :w]

    def operands_untouched(self):
        return all(torch.equal(a, b) for a, b in self.bufs.values())


class Guarded:
    """A row-major output between GAP sentinel columns and in front of PAD_ROWS sentinel rows"""

    def __init__(self, n, width, dtype, device, gap=GAP):
        self.buf = torch.full((n + PAD_ROWS, width + 2 * gap), SENTINEL, dtype=dtype, device=device)
        self.out = self.buf[:n, gap:gap + width]
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        self.mask[:n, gap:gap + width] = False

    def intact(self):
        return bool((self.buf[self.mask] == SENTINEL).all())


class Opaque:
    """An opaque accumulator buffer of `nbytes` bytes with TAIL sentinel bytes behind it"""

    def __init__(self, nbytes, device):
        self.nbytes = int(nbytes)
        self.buf = torch.full((self.nbytes + TAIL,), TAIL_BYTE, dtype=torch.uint8, device=device)

    def intact(self):
        return bool((self.buf[self.nbytes:] == TAIL_BYTE).all())


class Dev(Operands):
    """One width of the rowgemm entries on the device"""

    def __init__(self, case, device):
        super().__init__(device)
        d = case.d
        self.c, self.d, self.n = case, d, case.n
        a = self.up("a", case.a, extra_cols=8)                # ld = 2 d + 8: the operands are column slices of a wider buffer
        g = self.up("g", case.g, extra_cols=8)
        self.a1, self.a2 = a[:, :d], a[:, d:]
        self.g1, self.g2 = g[:, :d], g[:, d:]
        self.ai = self.up("ai", case.ai)
        self.ws = case.ws.to(device).to(BF16)
        for name in ("wd", "wg"):                             # ldw = 2 d + 8
            w = torch.full((d, 2 * d + 8), POISON, dtype=BF16, device=device)
            w[:, :2 * d] = getattr(case, name).to(device).to(BF16)
            self.bufs[name] = (w, w.clone())
            setattr(self, name, w[:, :2 * d])
        self.bias, self.shift = case.bias.to(device), case.shift.to(device)
        self.bn = [{k: v.to(device) for k, v in coefs.items()} for coefs in case.bn]
        self.ws_bytes = _L().load().sgf_gcn_epilogue_workspace_bytes(self.n, d)

    def stats_ws(self):
        return torch.empty(max(self.ws_bytes, 256), dtype=torch.uint8, device=self.device)


@pytest.fixture(scope="module", params=WIDTHS, ids=lambda d: f"d{d}")
def dev(request, cuda):
    return Dev(get_case(request.param), cuda)


def _stats_args(dv, want):
    """(shift, stats, workspace, workspace bytes) of an entry that returns the column statistics"""
    if not want:
        return None, None, None, 0
    ws = dv.stats_ws()
    return dv.shift, torch.full((2 * dv.d,), SENTINEL, dtype=F32, device=dv.device), ws, ws.numel()


def _check_stats(name, stats, y64, shift):
    assert torch.equal(rnd(y64), y64), f"{name}: the exact y is not a bf16 value: its statistics would be those of another tensor"
    worst = stats_abs_sum(y64, shift.double())
    assert worst < EXACT, f"{name}: abs-sum {worst} >= 2^24 (broken test)"
    check_exact(name, stats, ref_stats(y64, shift.double()))


# ---- sgf_gcn_epilogue_stats / _dx (k_rowgemm_bf16, IO 0) ----
@pytest.mark.parametrize("with_bias", [True, False])
def test_epilogue_stats(dev, with_bias):
    """y = a1 W1^T (+ bias) and its column statistics against the fp64 sums of the EXACT y (which is a bf16 value here, so they
    are also those of the stored one): one dropped or doubled row among 196 613 changes them."""
    d, n, L = dev.d, dev.n, _L()
    bias = dev.bias if with_bias else None
    w = dev.ws[:, :d]

    def run():
        y = Guarded(n, d, BF16, dev.device)
        shift, stats, ws, wsb = _stats_args(dev, True)
        L.call("sgf_gcn_epilogue_stats", _p(dev.a1), _ld(dev.a1), _p(w), _ld(w), _p(bias), n, d, d, L.SGF_BF16, _p(y.out),
               _ld(y.out), _p(shift), _p(stats), _p(ws), wsb, _st(dev.device))
        return y, stats

    y, stats = run()
    y2, stats2 = run()
    ref = ref_linear(dev.a1.double(), w.double(), None if bias is None else bias.double())
    check_bf16("y", y.out, ref)
    _check_stats("stats", stats, ref, dev.shift)
    assert y.intact(), "a sentinel column or a row behind N was written"
    assert torch.equal(y.buf, y2.buf) and torch.equal(stats, stats2)
    assert dev.operands_untouched()


def test_epilogue_dx(dev):
    """dx = dy W (W loaded transposed, a column slice with ldw = 2 d + 8): values of several hundred, so the rounding is real"""
    d, n, L = dev.d, dev.n, _L()
    w = dev.wg[:, :d]

    def run():
        dx = Guarded(n, d, BF16, dev.device)
        L.call("sgf_gcn_epilogue_dx", _p(dev.g1), _ld(dev.g1), _p(w), _ld(w), n, d, d, L.SGF_BF16, _p(dx.out), _ld(dx.out),
               _st(dev.device))
        return dx

    dx, dx2 = run(), run()
    check_bf16("dx", dx.out, ref_dx(dev.g1.double(), w.double()))
    assert dx.intact(), "a sentinel column or a row behind N was written"
    assert torch.equal(dx.buf, dx2.buf)
    assert dev.operands_untouched()


# ---- sgf_gcn_epilogue_partial + _stats_add (k_rowgemm_bf16, IO 1 / 2) ----
def test_two_pass(dev):
    """y = round(a2 W2^T + round(a1 W1^T + b)) and its statistics; the opaque partial buffer keeps its sentinel bytes"""
    d, n, L = dev.d, dev.n, _L()
    w1, w2 = dev.ws[:, :d], dev.ws[:, d:]
    nbytes = L.load().sgf_gcn_epilogue_partial_bytes(n, d)

    def run():
        part, y = Opaque(nbytes, dev.device), Guarded(n, d, BF16, dev.device)
        shift, stats, ws, wsb = _stats_args(dev, True)
        L.call("sgf_gcn_epilogue_partial", _p(dev.a1), _ld(dev.a1), _p(w1), _ld(w1), _p(dev.bias), n, d, d, L.SGF_BF16,
               _p(part.buf), nbytes, _st(dev.device))
        L.call("sgf_gcn_epilogue_stats_add", _p(dev.a2), _ld(dev.a2), _p(w2), _ld(w2), _p(part.buf), nbytes, n, d, d, L.SGF_BF16,
               _p(y.out), _ld(y.out), _p(shift), _p(stats), _p(ws), wsb, _st(dev.device))
        return part, y, stats

    part, y, stats = run()
    part2, y2, stats2 = run()
    ref = ref_two_pass(dev.a1.double(), dev.a2.double(), dev.ws.double(), dev.bias.double())
    check_bf16("y", y.out, ref)
    _check_stats("stats", stats, ref, dev.shift)
    assert y.intact() and part.intact(), "a sentinel was written"
    assert torch.equal(y.buf, y2.buf) and torch.equal(stats, stats2) and torch.equal(part.buf, part2.buf)
    assert dev.operands_untouched()


# ---- sgf_gcn_epilogue_cat (k_rowgemm2_bf16; d = 256: paired) ----
@pytest.mark.parametrize("want_stats", [True, False])
def test_epilogue_cat(dev, want_stats):
    """y = [a1 | a2] W^T + bias rounded once, and its statistics; a1, a2 are column slices of one buffer with ld = 2 d + 8"""
    d, n, L = dev.d, dev.n, _L()
    assert dev.a1.stride(0) == 2 * d + 8 and dev.a2.data_ptr() == dev.a1.data_ptr() + 2 * d

    def run():
        y = Guarded(n, d, BF16, dev.device)
        shift, stats, ws, wsb = _stats_args(dev, want_stats)
        L.call("sgf_gcn_epilogue_cat", _p(dev.a1), _ld(dev.a1), _p(dev.a2), _ld(dev.a2), _p(dev.ws), _ld(dev.ws), _p(dev.bias), n, d,
               L.SGF_BF16, _p(y.out), _ld(y.out), _p(shift), _p(stats), _p(ws), wsb, _st(dev.device))
        return y, stats

    y, stats = run()
    y2, stats2 = run()
    ref = ref_cat(dev.a1.double(), dev.a2.double(), dev.ws.double(), dev.bias.double())
    check_bf16("y", y.out, ref)
    if want_stats:
        _check_stats("stats", stats, ref, dev.shift)
        assert torch.equal(stats, stats2)
    assert y.intact(), "a sentinel column or a row behind N was written"
    assert torch.equal(y.buf, y2.buf)
    assert dev.operands_untouched()


# ---- sgf_gcn_epilogue_dx2 (k_rowgemm_bf16 with pair = 1: two workgroups per tile) ----
def test_epilogue_dx2(dev):
    """dx1 = dy W[:, :d], dx2 = dy W[:, d:]: the paired launch and the two plain ones equal each other and the reference"""
    d, n, L = dev.d, dev.n, _L()
    w1, w2 = dev.wg[:, :d], dev.wg[:, d:]

    def run(pair):
        o1, o2 = Guarded(n, d, BF16, dev.device), Guarded(n, d, BF16, dev.device)
        L.call("sgf_gcn_epilogue_dx2", _p(dev.g1), _ld(dev.g1), _p(w1), _p(w2), _ld(w1), n, d, L.SGF_BF16, _p(o1.out), _ld(o1.out),
               _p(o2.out), _ld(o2.out), int(pair), _st(dev.device))
        return o1, o2

    p1, p2 = run(True)
    q1, q2 = run(True)
    s1, s2 = run(False)
    g64, w64 = dev.g1.double(), dev.wg.double()
    check_bf16("dx1", p1.out, ref_dx(g64, w64[:, :d]))
    check_bf16("dx2", p2.out, ref_dx(g64, w64[:, d:]))
    for o in (p1, p2, s1, s2):
        assert o.intact(), "a sentinel column or a row behind N was written"
    assert torch.equal(p1.buf, s1.buf) and torch.equal(p2.buf, s2.buf), "pair and no-pair differ"
    assert torch.equal(p1.buf, q1.buf) and torch.equal(p2.buf, q2.buf)
    assert dev.operands_untouched()


# ---- sgf_gcn_epilogue_dx2_acc (k_dx2acc_bf16; d = 256: paired) ----
@pytest.mark.parametrize("with_gadd,with_acc", [(False, False), (True, False), (False, True), (True, True)])
def test_epilogue_dx2_acc(dev, with_gadd, with_acc):
    """dy = dz W[:, :d], acc_out = round(dz W[:, d:]) + gadd + acc_in rounded once more; with acc_in also the aliased form
    (acc_out == acc_in), which must give the same bits"""
    d, n, L = dev.d, dev.n, _L()
    gadd = dev.g2 if with_gadd else None
    acc_in = dev.ai if with_acc else None

    def run(alias=False):
        dy, acc = Guarded(n, d, BF16, dev.device), Guarded(n, d, BF16, dev.device)
        src = acc_in
        if alias:
            acc.out.copy_(acc_in)
            src = acc.out
        L.call("sgf_gcn_epilogue_dx2_acc", _p(dev.g1), _ld(dev.g1), _p(dev.wg), _ld(dev.wg), n, d, L.SGF_BF16, _p(dy.out),
               _ld(dy.out), _p(gadd), _ld(gadd), _p(src), _ld(src), _p(acc.out), _ld(acc.out), _st(dev.device))
        return dy, acc

    dy, acc = run()
    dy2, acc2 = run()
    r_dy, r_acc = ref_dx2_acc(dev.g1.double(), dev.wg.double(), None if gadd is None else gadd.double(),
                              None if acc_in is None else acc_in.double())
    check_bf16("dy", dy.out, r_dy)
    check_bf16("acc_out", acc.out, r_acc)
    assert dy.intact() and acc.intact(), "a sentinel column or a row behind N was written"
    assert torch.equal(dy.buf, dy2.buf) and torch.equal(acc.buf, acc2.buf)
    if with_acc:
        dy3, acc3 = run(alias=True)
        assert torch.equal(dy.buf, dy3.buf) and torch.equal(acc.buf, acc3.buf), "the aliased form differs"
    assert dev.operands_untouched()


# ---- sgf_gcn_bn_bwd_dx (k_bn_bwd_dx_bf16: 1, 2 or 4 workgroups per tile, a 4-slot fragment ring across tiles) ----
@pytest.fixture
def bwd_sync_env():
    yield
    os.environ.pop("SGF_GCN_BWD_SYNC", None)
    _L().load().sgf_reload_env()


def _bwd_sync(value):
    if value is None:
        os.environ.pop("SGF_GCN_BWD_SYNC", None)
    else:
        os.environ["SGF_GCN_BWD_SYNC"] = str(value)
    _L().load().sgf_reload_env()


ADD_GY = (True, False, True)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu", [True, False])
def test_bn_bwd_dx_chain(dev, relu, training, bwd_sync_env):
    """Three chained calls as the products recipe issues them (acc_in = None, then chained, then the last one with dx0), each
    with its own BatchNorm constants, add_gy on the first and the last.  Per call dz (rounded once: up to 13 bits before)
    and dy = round(dz) W[:, :d]; after the chain the total, whose running sum was rounded to bf16 three times, in the places
    the reference rounds.  The rendezvous is timing only: SGF_GCN_BWD_SYNC=0 and a call without workspace give the same bits."""
    d, n, L = dev.d, dev.n, _L()
    lib = L.load()
    gy, z = dev.g1, dev.g2
    nbytes = lib.sgf_gcn_epilogue_partial_bytes(n, d)
    wsb = lib.sgf_gcn_bn_bwd_dx_workspace_bytes(n, d)

    def run(with_ws=True):
        outs, acc_in = [], None
        for i, (k, add) in enumerate(zip(dev.bn, ADD_GY)):
            last = i == 2
            dz, dy = Guarded(n, d, BF16, dev.device), Guarded(n, d, BF16, dev.device)
            acc = None if last else Opaque(nbytes, dev.device)
            dx0 = Guarded(n, d, BF16, dev.device) if last else None
            ws = torch.zeros(max(wsb, 256), dtype=torch.uint8, device=dev.device) if with_ws else None
            L.call("sgf_gcn_bn_bwd_dx", _p(gy), _ld(gy), _p(z), _ld(z), _p(k["mean"]), _p(k["rstd"]), _p(k["gamma"]), _p(k["beta"]),
                   int(relu), _p(k["stats"]) if training else None, INV_N, int(training), _p(dev.wd), _ld(dev.wd), n, d, L.SGF_BF16,
                   _p(dz.out), _ld(dz.out), _p(dy.out), _ld(dy.out), None if acc_in is None else _p(acc_in.buf),
                   None if acc is None else _p(acc.buf), nbytes, None if dx0 is None else _p(dx0.out),
                   0 if dx0 is None else _ld(dx0.out), int(add), None if ws is None else _p(ws), 0 if ws is None else ws.numel(),
                   _st(dev.device))
            outs.append((dz, dy, dx0 if last else acc))
            acc_in = acc
        return outs

    outs = run()
    again = run()
    refs = ref_bn_chain(gy.double(), z.double(), dev.wd.double(), dev.bn, relu, training, ADD_GY)
    # the dz W sums: dz a multiple of 1/512 (asserted), so the worst abs-sum in units of 1/512 must stay below 2^24
    for i, ((dz, dy, acc), (r_dz, r_dy, r_acc)) in enumerate(zip(outs, refs)):
        assert bool((r_dz * DZ_UNITS == (r_dz * DZ_UNITS).round()).all()), "dz is not a multiple of 1/512 (broken test)"
        worst = float((rnd(r_dz).abs() @ dev.wd.double().abs()).max() + 2 + r_acc.abs().max()) * DZ_UNITS
        assert worst < EXACT, f"call {i}: abs-sum {worst} >= 2^24 (broken test)"
        check_bf16(f"dz[{i}]", dz.out, r_dz)
        check_bf16(f"dy[{i}]", dy.out, r_dy)
        assert dz.intact() and dy.intact() and acc.intact(), f"call {i}: a sentinel was written"
    if training:                                              # (without the mean terms dz = gamma rstd g': a bf16 value)
        assert int((rnd(refs[0][0]) != refs[0][0]).sum()) > 0, "no dz value needs rounding (broken test)"
    check_bf16("dx0 total", outs[2][2].out, refs[2][2])
    for (dz, dy, acc), (dz2, dy2, acc2) in zip(outs, again):
        assert torch.equal(dz.buf, dz2.buf) and torch.equal(dy.buf, dy2.buf) and torch.equal(acc.buf, acc2.buf)
    _bwd_sync(0)
    free = run()
    _bwd_sync(None)
    bare = run(with_ws=False)
    for other, what in ((free, "SGF_GCN_BWD_SYNC=0"), (bare, "no workspace")):
        for (dz, dy, acc), (dz2, dy2, acc2) in zip(outs, other):
            assert torch.equal(dz.buf, dz2.buf) and torch.equal(dy.buf, dy2.buf) and torch.equal(acc.buf, acc2.buf), what
    assert dev.operands_untouched()


# ---- sgf_stem_pair (k_stem_bf16) ----
class StemDev(Operands):
    def __init__(self, case, device):
        super().__init__(device)
        self.c, self.f, self.d, self.n = case, case.f, case.d, case.n
        self.x = self.up("x", case.x)                         # contiguous: ld = f (f = 100: 200-byte rows, 8-byte aligned)
        self.w0, self.w1 = case.w0.to(device).to(BF16), case.w1.to(device).to(BF16)
        self.b0, self.b1, self.shift = case.b0.to(device), case.b1.to(device), case.shift.to(device)
        self.ws_bytes = _L().load().sgf_gcn_epilogue_workspace_bytes(self.n, self.d)

    stats_ws = Dev.stats_ws


@pytest.fixture(scope="module", params=STEM, ids=lambda p: "f%d-d%d" % p)
def stem(request, cuda):
    return StemDev(build_stem(*request.param), cuda)


@pytest.mark.parametrize("pair", [True, False])
def test_stem_pair(stem, pair):
    """y0 = x W0^T + b0 with its statistics and y1 = x W1^T + b1 from one read of x; pair = False: the one-output form"""
    f, d, n, L = stem.f, stem.d, stem.n, _L()
    if f == 100:
        assert stem.x.stride(0) * 2 % 16 == 8, "rows of x should be only 8-byte aligned"

    def run():
        y0 = Guarded(n, d, BF16, stem.device)
        y1 = Guarded(n, d, BF16, stem.device) if pair else None
        shift, stats, ws, wsb = _stats_args(stem, True)
        L.call("sgf_stem_pair", _p(stem.x), _ld(stem.x), n, f, _p(stem.w0), _ld(stem.w0), _p(stem.b0),
               _p(stem.w1) if pair else None, _ld(stem.w1) if pair else 0, _p(stem.b1) if pair else None, d, L.SGF_BF16, _p(y0.out),
               _ld(y0.out), None if y1 is None else _p(y1.out), 0 if y1 is None else _ld(y1.out), _p(shift), _p(stats), _p(ws), wsb,
               _st(stem.device))
        return y0, y1, stats

    y0, y1, stats = run()
    z0, z1, stats2 = run()
    x64 = stem.x.double()
    r0 = ref_linear(x64, stem.w0.double(), stem.b0.double())
    check_bf16("y0", y0.out, r0)
    _check_stats("stats0", stats, r0, stem.shift)
    assert y0.intact(), "a sentinel column or a row behind N was written"
    assert torch.equal(y0.buf, z0.buf) and torch.equal(stats, stats2)
    if pair:
        check_bf16("y1", y1.out, ref_linear(x64, stem.w1.double(), stem.b1.double()))
        assert y1.intact(), "a sentinel column or a row behind N was written"
        assert torch.equal(y1.buf, z1.buf)
    assert stem.operands_untouched()


# ---- no rows: the statistics are the empty sums, nothing else is read or written ----
@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("entry", ["sgf_gcn_epilogue_stats", "sgf_gcn_epilogue_stats_add", "sgf_gcn_epilogue_cat", "sgf_stem_pair"])
def test_no_rows_zero_the_statistics(cuda, entry, d):
    """n == 0 with a statistics pointer: every operand, output and workspace null; stats comes back as 2 d zero words between
    its sentinels"""
    L = _L()
    buf = torch.full((2 * d + 2 * GAP,), SENTINEL, dtype=F32, device=cuda)
    stats, st = ctypes.c_void_p(buf[GAP:].data_ptr()), _st(cuda)
    if entry == "sgf_gcn_epilogue_stats":
        L.call(entry, None, 0, None, 0, None, 0, d, d, L.SGF_BF16, None, 0, None, stats, None, 0, st)
    elif entry == "sgf_gcn_epilogue_stats_add":
        L.call(entry, None, 0, None, 0, None, 0, 0, d, d, L.SGF_BF16, None, 0, None, stats, None, 0, st)
    elif entry == "sgf_gcn_epilogue_cat":
        L.call(entry, None, 0, None, 0, None, 0, None, 0, d, L.SGF_BF16, None, 0, None, stats, None, 0, st)
    else:
        L.call(entry, None, 0, 0, 100, None, 0, None, None, 0, None, d, L.SGF_BF16, None, 0, None, 0, None, stats, None, 0, st)
    assert bool((buf[GAP:GAP + 2 * d].view(torch.int32) == 0).all()), "the empty sums are not all zero words"
    assert bool((buf[:GAP] == SENTINEL).all()) and bool((buf[GAP + 2 * d:] == SENTINEL).all()), "a word next to stats was written"


# ---- sgf_combine_fc_fwd / _bwd and their _mapped / _g forms (csrc/head.hip) ----
class HeadDev(Operands):
    def __init__(self, case, device):
        super().__init__(device)
        d = case.d
        self.c, self.d, self.classes = case, d, case.c
        x = self.up("x", case.x, extra_cols=8)
        self.x1, self.x2 = x[:, :d], x[:, d:]
        self.dl = self.up("dl", case.dl, extra_cols=3, dtype=F32)   # lddl = classes + 3: the rows of dlogits have no alignment
        self.w, self.bias = case.w.to(device), case.bias.to(device)
        self.map_fwd, self.map_bwd = case.map_fwd.to(device), case.map_bwd.to(device)


@pytest.fixture(scope="module", params=HEAD, ids=lambda p: "d%d-c%d" % p)
def head(request, cuda):
    return HeadDev(build_head(*request.param), cuda)


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("ab", HEAD_AB, ids=["half-half", "3q-1q"])
def test_head_fwd(head, ab, mapped):
    """logits = (a x1 + b x2) W^T + bias, fp32, exact: the combined row is a bf16 value (asserted), every sum a multiple of 1/4.
    _mapped: row j of the product lands in row row_map[j] (a seeded random permutation)."""
    (a, b), d, c, L = ab, head.d, head.classes, _L()
    n = head.x1.shape[0]

    def run():
        lg = Guarded(n, c, F32, head.device, gap=4)
        if mapped:
            L.call("sgf_combine_fc_fwd_mapped", _p(head.x1), _ld(head.x1), a, _p(head.x2), _ld(head.x2), b, _p(head.w), _p(head.bias),
                   n, d, c, L.SGF_BF16, _p(lg.out), _ld(lg.out), _p(head.map_fwd), _st(head.device))
        else:
            L.call("sgf_combine_fc_fwd", _p(head.x1), _ld(head.x1), a, _p(head.x2), _ld(head.x2), b, _p(head.w), _p(head.bias), n, d,
                   c, L.SGF_BF16, _p(lg.out), _ld(lg.out), _st(head.device))
        return lg

    lg, lg2 = run(), run()
    ref, xc = ref_head_fwd(head.x1.double(), a, head.x2.double(), b, head.w.double(), head.bias.double())
    assert torch.equal(rnd(xc), xc), "the combined row is not a bf16 value (broken test)"
    if mapped:
        out = torch.empty_like(ref)
        out[head.map_fwd.long()] = ref
        ref = out
    check_exact("logits", lg.out, ref)
    assert lg.intact(), "a sentinel column or a row behind N was written"
    assert torch.equal(lg.buf, lg2.buf)
    assert head.operands_untouched()


@pytest.mark.parametrize("form", ["plain", "mapped", "g", "g-mapped"])
@pytest.mark.parametrize("ab", HEAD_AB, ids=["half-half", "3q-1q"])
def test_head_bwd(head, ab, form):
    """dx1 = a (g W), dx2 = b (g W) rounded once (g W reaches a few hundred: 3/4 of it needs more than 8 bits); the _g forms also
    return g in bf16, zero-padded to 16 ceil(c / 16) columns, exactly; the mapped forms read row row_map[j] of dlogits for row j"""
    (a, b), d, c, L = ab, head.d, head.classes, _L()
    n = head.dl.shape[0]
    rmap = head.map_bwd if "mapped" in form else None
    cp = (c + 15) // 16 * 16

    def run():
        dx1, dx2 = Guarded(n, d, BF16, head.device), Guarded(n, d, BF16, head.device)
        gp = Guarded(n, cp, BF16, head.device) if form.startswith("g") else None
        tail = (_p(dx1.out), _ld(dx1.out), _p(dx2.out), _ld(dx2.out))
        args = (_p(head.dl), _ld(head.dl), _p(head.w), n, d, c, a, b, L.SGF_BF16) + tail
        if gp is not None:
            L.call("sgf_combine_fc_bwd_g", *args, _p(rmap), _p(gp.out), _ld(gp.out), _st(head.device))
        elif rmap is not None:
            L.call("sgf_combine_fc_bwd_mapped", *args, _p(rmap), _st(head.device))
        else:
            L.call("sgf_combine_fc_bwd", *args, _st(head.device))
        return dx1, dx2, gp

    dx1, dx2, gp = run()
    e1, e2, gp2 = run()
    g64 = head.dl.double()
    if rmap is not None:
        g64 = g64[rmap.long()]
    r1, r2 = ref_head_bwd(g64, head.w.double(), a, b)
    check_bf16("dx1", dx1.out, r1)
    check_bf16("dx2", dx2.out, r2)
    assert dx1.intact() and dx2.intact(), "a sentinel column or a row behind N was written"
    assert torch.equal(dx1.buf, e1.buf) and torch.equal(dx2.buf, e2.buf)
    if gp is not None:
        want = torch.zeros((n, cp), dtype=F64, device=head.device)
        want[:, :c] = g64
        check_exact("g_out", gp.out, want)
        assert gp.intact(), "a sentinel column or a row behind N was written"
        assert torch.equal(gp.buf, gp2.buf)
    assert head.operands_untouched()
