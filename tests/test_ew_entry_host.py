"""Argument checks of the row-wise and element-wise entries of csrc/fused.hip (LayerNorm, BatchNorm, column statistics, axpby,
gather / pad, sum_n, dropout, NLL, colsum), through ctypes on the CPU.

Every call here is rejected (or returns SGF_OK for an empty problem that has no output to zero) on the host BEFORE any HIP call,
so the file runs without a GPU.  Pointer arguments are dummy, suitably aligned host addresses that are never dereferenced (the
operand tables of sgf_sum_n, which the host reads, are real).  The status values are those of include/sgf.h; after a rejection
sgf_last_error() starts with the name of the entry that was called.
"""
import ctypes

import pytest

SGF_OK, SGF_E_INVALID, SGF_E_WORKSPACE, SGF_E_UNSUPPORTED = 0, -1, -2, -4
F32, BF16, F32X = 0, 1, 2
A = 0x10000              # a 64 KiB-aligned dummy address
N = 65536
BIG = 1 << 40            # a workspace size that is never the reason for a rejection
MAX_STAT_BLOCKS = 2048   # partial rows of the column reductions

# argument names in the order of include/sgf.h; a name that is not a scalar below is a leading dimension (ld*) or a pointer
SIGS = {
    "sgf_ln_fwd": "x ldx res ldr a b gamma beta relu eps n d dtype y ldy mean rstd stream",
    "sgf_ln_bwd": "dy lddy y ldy x ldx res ldr a b gamma relu mean rstd n d dtype dx lddx dres lddres dgamma dbeta workspace "
                  "workspace_bytes stream",
    "sgf_colstats": "x ldx shift n d dtype stats workspace workspace_bytes stream",
    "sgf_bn_finalize": "sums shift n_total eps momentum running_mean running_var d mean rstd stream",
    "sgf_bn_apply": "x ldx mean rstd gamma beta res ldr relu n d dtype y ldy stream",
    "sgf_bn_apply_packed": "x ldx mean rstd gamma beta res ldr relu n d dtype y ldy packed slot_bytes overflow stream",
    "sgf_bn_bwd_stats": "dy lddy x ldx mean rstd gamma beta relu n d dtype stats workspace workspace_bytes stream",
    "sgf_bn_bwd_stats2": "dy lddy dy2 lddy2 x ldx mean rstd gamma beta relu n d dtype stats workspace workspace_bytes stream",
    "sgf_bn_bwd_apply": "dy lddy x ldx mean rstd gamma beta relu stats inv_n training n d dtype dx lddx stream",
    "sgf_axpby": "x1 ld1 a x2 ld2 b n d dtype y ldy stream",
    "sgf_gather_rows": "src lds src_dtype n_src idx idx_is_int64 n_out d dst ldd dst_dtype stream",
    "sgf_pad_rows": "src lds src_dtype n_src idx idx_is_int64 n_out d d_pad dst ldd dst_dtype stream",
    "sgf_sum_n": "xs ldxs k n d dtype y ldy stream",
    "sgf_dropout": "x ldx res ldr p seed n d dtype y ldy stream",
    "sgf_dropout_dev": "x ldx res ldr p seed_slot n d dtype y ldy stream",
    "sgf_nll_fwd": "logits ldl n c dtype labels idx m loss_sum workspace workspace_bytes stream",
    "sgf_nll_bwd": "logits ldl n c dtype labels idx m gout inv_denom dlogits ldd stream",
    "sgf_colsum": "x ldx n d dtype out workspace workspace_bytes stream",
}
SCALARS = dict(n=N, d=64, dtype=BF16, relu=0, training=1, inv_n=1.0, a=1.0, b=1.0, eps=1e-5, momentum=0.1, n_total=float(N), p=0.5,
               seed=1234, k=3, c=40, m=1000, inv_denom=1.0, src_dtype=BF16, dst_dtype=BF16, n_src=N, n_out=N, d_pad=64,
               idx_is_int64=1, slot_bytes=384, workspace_bytes=BIG, stream=None)
DEFAULTS = {"sgf_bn_apply_packed": dict(d=256)}

# the entries that open with the shared (n, d, dtype) check, and the pointers each refuses as null when n > 0
CHECK_EW = ["sgf_ln_fwd", "sgf_ln_bwd", "sgf_colstats", "sgf_bn_apply", "sgf_bn_apply_packed", "sgf_bn_bwd_stats",
            "sgf_bn_bwd_stats2", "sgf_bn_bwd_apply", "sgf_axpby", "sgf_sum_n", "sgf_dropout", "sgf_dropout_dev"]
REQUIRED = {
    "sgf_ln_fwd": "x y",
    "sgf_ln_bwd": "dy dx",
    "sgf_colstats": "stats x",
    "sgf_bn_finalize": "sums mean rstd",
    "sgf_bn_apply": "x y mean rstd",
    "sgf_bn_apply_packed": "x y mean rstd packed overflow",
    "sgf_bn_bwd_stats": "stats dy x mean rstd",
    "sgf_bn_bwd_stats2": "stats dy x mean rstd",
    "sgf_bn_bwd_apply": "dy x dx mean rstd stats",
    "sgf_axpby": "x1 x2 y",
    "sgf_gather_rows": "src idx dst",
    "sgf_pad_rows": "src dst",
    "sgf_sum_n": "xs ldxs y",
    "sgf_dropout": "x y",
    "sgf_dropout_dev": "x y seed_slot",
    "sgf_nll_fwd": "loss_sum logits labels idx",
    "sgf_nll_bwd": "dlogits gout",
}
# leading dimensions that must be multiples of 4 elements (with the optional operand each belongs to, if any)
LD4 = {
    "sgf_ln_fwd": "ldx ldy ldr",
    "sgf_bn_apply": "ldx ldy ldr",
    "sgf_colstats": "ldx",
    "sgf_bn_bwd_stats": "lddy ldx",
    "sgf_bn_bwd_stats2": "lddy ldx lddy2",
    "sgf_bn_bwd_apply": "lddy ldx lddx",
    "sgf_axpby": "ld1 ld2 ldy",
    "sgf_sum_n": "ldy",
    "sgf_dropout": "ldx ldy ldr",
    "sgf_dropout_dev": "ldx ldy ldr",
}
# sgf_bn_bwd_stats is a forwarder: its messages carry the name of sgf_bn_bwd_stats2
PREFIX = {"sgf_bn_bwd_stats": "sgf_bn_bwd_stats2"}


@pytest.fixture(scope="module")
def lib():
    from sgformer_amd import _lib
    if not _lib.available():
        pytest.skip("libsgf.so not built (run `make`)")
    return _lib.load()


class _Table:
    """The operand table of sgf_sum_n: k pointers and k leading dimensions in host memory."""

    def __init__(self, ptrs=(A, A, A, A, A, A, A, A), lds=(256,) * 8):
        self.xs = (ctypes.c_void_p * len(ptrs))(*ptrs)
        self.lds = (ctypes.c_int64 * len(lds))(*lds)


_TABLE = _Table()


def _call(lib, entry, **kw):
    """One call of `entry` with plausible arguments (every pointer A, every leading dimension 256) except those in `kw`."""
    names = SIGS[entry].split()
    assert set(kw) <= set(names), (entry, sorted(set(kw) - set(names)))
    kw = {**DEFAULTS.get(entry, {}), **kw}
    if entry == "sgf_sum_n":
        kw.setdefault("xs", ctypes.addressof(_TABLE.xs))
        kw.setdefault("ldxs", ctypes.addressof(_TABLE.lds))
    args = [kw[a] if a in kw else SCALARS[a] if a in SCALARS else 256 if a.startswith("ld") else A for a in names]
    return getattr(lib, entry)(*args)


def _rejected(lib, entry, code, prefix=None, **kw):
    assert _call(lib, entry, **kw) == code, lib.sgf_last_error()
    assert lib.sgf_last_error().startswith((prefix or PREFIX.get(entry, entry)).encode() + b":"), lib.sgf_last_error()


# ---- sizes, widths and dtype codes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", CHECK_EW)
def test_common_checks(lib, entry):
    _rejected(lib, entry, SGF_E_INVALID, n=-1)
    assert b"bad sizes n=-1" in lib.sgf_last_error()
    _rejected(lib, entry, SGF_E_INVALID, d=0)
    _rejected(lib, entry, SGF_E_INVALID, d=-4)
    _rejected(lib, entry, SGF_E_UNSUPPORTED, d=6)                    # not a multiple of 4
    _rejected(lib, entry, SGF_E_UNSUPPORTED, d=1028)                 # wider than 1024
    for dtype in (F32X, 7):
        _rejected(lib, entry, SGF_E_INVALID, dtype=dtype)
        assert b"unknown dtype %d" % dtype in lib.sgf_last_error()
    _rejected(lib, entry, SGF_E_UNSUPPORTED, d=1028, dtype=7)        # the width is judged before the dtype code
    _rejected(lib, entry, SGF_E_INVALID, n=-1, d=6)                  # and a negative n before the width
    if entry != "sgf_bn_apply_packed":                               # (which looks at its pointers first)
        first = REQUIRED[entry].split()[0]
        _rejected(lib, entry, SGF_E_UNSUPPORTED, d=6, **{first: None})
        _rejected(lib, entry, SGF_E_INVALID, dtype=7, **{first: None})
        assert b"unknown dtype 7" in lib.sgf_last_error()


def test_uncommon_size_checks(lib):
    _rejected(lib, "sgf_bn_finalize", SGF_E_INVALID, d=0)
    _rejected(lib, "sgf_bn_finalize", SGF_E_INVALID, n_total=-1.0)
    _rejected(lib, "sgf_bn_finalize", SGF_E_INVALID, d=0, sums=None)
    assert b"bad sizes" in lib.sgf_last_error()
    for e in ("sgf_gather_rows", "sgf_pad_rows"):
        for kw in (dict(n_out=-1), dict(d=-1), dict(n_src=-1)):
            _rejected(lib, e, SGF_E_INVALID, **kw)
            _rejected(lib, e, SGF_E_INVALID, src_dtype=7, **kw)
            assert b"unknown dtype" not in lib.sgf_last_error()     # the sizes first
        for kw in (dict(src_dtype=7), dict(dst_dtype=7), dict(src_dtype=F32X), dict(dst_dtype=F32X)):
            _rejected(lib, e, SGF_E_INVALID, **kw)
            assert b"unknown dtype" in lib.sgf_last_error()
            _rejected(lib, e, SGF_E_INVALID, n_out=0, **kw)          # also with nothing to copy
    _rejected(lib, "sgf_pad_rows", SGF_E_INVALID, d=64, d_pad=60)
    for e in ("sgf_nll_fwd", "sgf_nll_bwd"):
        for kw in (dict(n=-1), dict(m=-1), dict(c=0), dict(ldl=32)):
            _rejected(lib, e, SGF_E_INVALID, **kw)
            assert b"bad sizes" in lib.sgf_last_error()
            _rejected(lib, e, SGF_E_INVALID, dtype=7, **kw)
            assert b"bad sizes" in lib.sgf_last_error()
        for dtype in (F32X, 7):
            _rejected(lib, e, SGF_E_INVALID, dtype=dtype)
            assert b"unknown dtype" in lib.sgf_last_error()
    _rejected(lib, "sgf_nll_bwd", SGF_E_INVALID, ldd=32)
    assert b"bad sizes" in lib.sgf_last_error()
    e = "sgf_colsum"                                                 # its sizes are a matter of support
    for kw in (dict(n=-1), dict(d=0), dict(d=257)):
        _rejected(lib, e, SGF_E_UNSUPPORTED, **kw)
        _rejected(lib, e, SGF_E_UNSUPPORTED, dtype=7, out=None, **kw)
    for dtype in (F32X, 7):
        _rejected(lib, e, SGF_E_INVALID, dtype=dtype)
        _rejected(lib, e, SGF_E_INVALID, dtype=dtype, out=None)
        assert b"unknown dtype" in lib.sgf_last_error()
    _rejected(lib, e, SGF_E_INVALID, d=6, dtype=7)                   # any width up to 256


def test_sum_n_operand_count(lib):
    for k in (0, -1, 9):
        _rejected(lib, "sgf_sum_n", SGF_E_INVALID, k=k)
        _rejected(lib, "sgf_sum_n", SGF_E_INVALID, k=k, n=0)         # judged with no rows too
        assert b"need 1 <= k <= 8" in lib.sgf_last_error()
    _rejected(lib, "sgf_sum_n", SGF_E_INVALID, y=None, n=0)


def test_dropout_probability(lib):
    for e in ("sgf_dropout", "sgf_dropout_dev"):
        for p in (-0.25, 1.5):
            _rejected(lib, e, SGF_E_INVALID, p=p)
            assert b"p must be in [0, 1]" in lib.sgf_last_error()
            _rejected(lib, e, SGF_E_INVALID, p=p, n=0)               # judged with no rows too
            _rejected(lib, e, SGF_E_INVALID, p=p, x=None)
            assert b"p must be in [0, 1]" in lib.sgf_last_error()
        _rejected(lib, e, SGF_E_UNSUPPORTED, p=1.5, d=6)             # after the shared check


def test_packed_apply_supported_set(lib):
    e = "sgf_bn_apply_packed"
    for kw in (dict(dtype=F32), dict(d=64), dict(d=128), dict(d=512)):
        _rejected(lib, e, SGF_E_UNSUPPORTED, **kw)
        assert b"packed rows are bf16 rows of 256 columns" in lib.sgf_last_error()
    for s in (0, 256, 400, 512):
        _rejected(lib, e, SGF_E_UNSUPPORTED, slot_bytes=s)
        assert b"slot_bytes must be 384 or 448" in lib.sgf_last_error()
    _rejected(lib, e, SGF_E_UNSUPPORTED, d=64, slot_bytes=400, x=A + 8)
    assert b"packed rows" in lib.sgf_last_error()
    _rejected(lib, e, SGF_E_UNSUPPORTED, slot_bytes=400, x=A + 8)    # before the alignment
    for name in REQUIRED[e].split():                                 # its pointers come before everything, rows or not
        for kw in (dict(), dict(d=6), dict(n=-1), dict(dtype=7), dict(n=0), dict(slot_bytes=400)):
            _rejected(lib, e, SGF_E_INVALID, **{name: None}, **kw)
            assert b"null pointer" in lib.sgf_last_error()


# ---- empty problems -----------------------------------------------------------------------------------------------------------
EMPTY_OK = ["sgf_ln_fwd", "sgf_ln_bwd", "sgf_bn_apply", "sgf_bn_bwd_apply", "sgf_axpby", "sgf_dropout", "sgf_dropout_dev",
            "sgf_gather_rows", "sgf_pad_rows"]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("entry", EMPTY_OK)
def test_no_rows_is_ok_before_the_pointer_checks(lib, entry, dtype):
    """n == 0 with no output to zero: SGF_OK with every pointer null, every leading dimension 0 and no workspace."""
    names = SIGS[entry].split()
    kw = {a: (0 if a.startswith("ld") or a.endswith("_bytes") else None) for a in names if a not in SCALARS or a.endswith("_bytes")}
    kw.update({"n_out": 0} if "n_out" in names else {"n": 0})
    kw.update({a: dtype for a in ("dtype", "src_dtype", "dst_dtype") if a in names})
    assert _call(lib, entry, **kw) == SGF_OK, lib.sgf_last_error()


def test_other_empty_problems(lib):
    assert _call(lib, "sgf_ln_bwd", n=0, gamma=None, dy=None, dx=None) == SGF_OK           # no gamma: dgamma / dbeta untouched
    assert _call(lib, "sgf_sum_n", n=0) == SGF_OK
    assert _call(lib, "sgf_gather_rows", d=0, src=None, idx=None, dst=None) == SGF_OK
    assert _call(lib, "sgf_pad_rows", d=0, d_pad=0, src=None, dst=None) == SGF_OK
    assert _call(lib, "sgf_nll_bwd", n=0, m=5, dlogits=None, gout=None) == SGF_OK
    # an output that would be zeroed is asked for first
    _rejected(lib, "sgf_colstats", SGF_E_INVALID, n=0, stats=None)
    _rejected(lib, "sgf_bn_bwd_stats2", SGF_E_INVALID, n=0, stats=None)
    _rejected(lib, "sgf_bn_bwd_stats", SGF_E_INVALID, n=0, stats=None)
    _rejected(lib, "sgf_nll_fwd", SGF_E_INVALID, m=0, loss_sum=None)
    _rejected(lib, "sgf_colsum", SGF_E_INVALID, n=0, out=None)


# ---- null pointers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("entry", sorted(REQUIRED))
def test_null_pointers(lib, entry, dtype):
    if entry == "sgf_bn_apply_packed":                               # bf16 only; its pointers come first in any case
        dtype = BF16
    dt = {a: dtype for a in ("dtype", "src_dtype", "dst_dtype") if a in SIGS[entry].split()}
    for name in REQUIRED[entry].split():
        _rejected(lib, entry, SGF_E_INVALID, **dt, **{name: None})
        if "workspace" in SIGS[entry].split():                       # judged before the workspace
            _rejected(lib, entry, SGF_E_INVALID, workspace=None, **dt, **{name: None})


def test_null_pointers_that_depend_on_an_argument(lib):
    for name in ("beta", "mean", "rstd"):                            # LayerNorm with an affine part
        _rejected(lib, "sgf_ln_fwd", SGF_E_INVALID, **{name: None})
        _rejected(lib, "sgf_ln_fwd", SGF_E_INVALID, gamma=None, ldx=6, **{name: None})
        assert b"leading dims" in lib.sgf_last_error()
    _rejected(lib, "sgf_ln_fwd", SGF_E_INVALID, res=None, ldr=6, ldx=6)
    for name in ("x", "mean", "rstd"):
        _rejected(lib, "sgf_ln_bwd", SGF_E_INVALID, **{name: None})
        assert b"null pointer" in lib.sgf_last_error()
    _rejected(lib, "sgf_ln_bwd", SGF_E_INVALID, relu=1, y=None)
    _rejected(lib, "sgf_ln_bwd", SGF_E_WORKSPACE, relu=0, y=None, res=None, dres=None, dgamma=None, dbeta=None, workspace=None)
    _rejected(lib, "sgf_bn_bwd_apply", SGF_E_INVALID, training=0, stats=None, lddy=6)
    assert b"leading dims" in lib.sgf_last_error()
    for kw in (dict(gamma=None, beta=None), dict(res=None)):
        _rejected(lib, "sgf_bn_apply", SGF_E_INVALID, ldx=6, **kw)
        assert b"leading dims" in lib.sgf_last_error()
    _rejected(lib, "sgf_bn_bwd_stats2", SGF_E_WORKSPACE, dy2=None, lddy2=6, workspace=None)
    _rejected(lib, "sgf_pad_rows", SGF_E_INVALID, idx=None, ldd=32)            # identity rows: idx is optional
    assert b"bad pointer / ld" in lib.sgf_last_error()
    _rejected(lib, "sgf_dropout_dev", SGF_E_INVALID, seed_slot=A + 4)
    assert b"8-byte aligned device address" in lib.sgf_last_error()
    _rejected(lib, "sgf_dropout_dev", SGF_E_INVALID, seed_slot=None, x=None)
    assert b"bad pointer / ld" in lib.sgf_last_error()              # the rows before the seed slot


def test_sum_n_operand_table(lib):
    e = "sgf_sum_n"
    t = _Table(ptrs=(A, None, A))
    _rejected(lib, e, SGF_E_INVALID, xs=ctypes.addressof(t.xs))
    assert b"bad operand 1" in lib.sgf_last_error()
    t = _Table(lds=(256, 256, 258))
    _rejected(lib, e, SGF_E_INVALID, ldxs=ctypes.addressof(t.lds))
    assert b"bad operand 2" in lib.sgf_last_error()
    _rejected(lib, e, SGF_E_INVALID, ldxs=ctypes.addressof(t.lds), ldy=6)
    assert b"bad operand 2" in lib.sgf_last_error()                  # the operands before y
    assert _call(lib, e, k=2, ldxs=ctypes.addressof(t.lds), ldy=6) == SGF_E_INVALID      # only the first k are read
    assert b"bad ldy" in lib.sgf_last_error()


# ---- leading dimensions and alignment -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("entry", sorted(LD4))
def test_leading_dimension_not_a_multiple_of_four(lib, entry, dtype):
    for ld in LD4[entry].split():
        _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **{ld: 258})
        _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **{ld: 6})
        if "workspace" in SIGS[entry].split():                       # judged before the workspace
            _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, workspace=None, **{ld: 258})


def test_copy_rows_hold_the_width(lib):
    for e in ("sgf_gather_rows", "sgf_pad_rows"):
        _rejected(lib, e, SGF_E_INVALID, lds=32)
        _rejected(lib, e, SGF_E_INVALID, ldd=32)
    _rejected(lib, "sgf_pad_rows", SGF_E_INVALID, d=60, d_pad=64, ldd=60)      # the destination holds the padded width
    _rejected(lib, "sgf_pad_rows", SGF_E_INVALID, d=60, d_pad=64, lds=56)


def test_packed_apply_alignment(lib):
    e = "sgf_bn_apply_packed"
    for kw in (dict(ldx=260), dict(ldy=260), dict(ldr=260), dict(x=A + 8), dict(y=A + 8), dict(res=A + 8), dict(packed=A + 64),
               dict(packed=A + 16)):
        _rejected(lib, e, SGF_E_INVALID, **kw)
        assert b"rows must be 16-byte aligned, the packed buffer 128-byte aligned" in lib.sgf_last_error()
        _rejected(lib, e, SGF_E_INVALID, n=0, **kw)                  # judged with no rows too
    _rejected(lib, e, SGF_E_INVALID, res=None, ldr=260, x=A + 8)


# ---- workspaces ---------------------------------------------------------------------------------------------------------------
def test_workspace_queries(lib):
    for q in (lib.sgf_ln_bwd_workspace_bytes, lib.sgf_colstats_workspace_bytes):
        assert q(N, 0) == 0 and q(N, -4) == 0
        assert q(0, 64) == q(N, 64) == q(-1, 64) == MAX_STAT_BLOCKS * 2 * 64 * 4
        assert q(N, 1024) == MAX_STAT_BLOCKS * 2 * 1024 * 4
    q = lib.sgf_colsum_workspace_bytes
    assert q(N, 0) == 0 and q(0, 37) == q(N, 37) == MAX_STAT_BLOCKS * 37 * 4
    assert lib.sgf_nll_workspace_bytes(0) == lib.sgf_nll_workspace_bytes(N) == 1024 * 4


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("entry,query", [("sgf_ln_bwd", "sgf_ln_bwd_workspace_bytes"), ("sgf_colstats", "sgf_colstats_workspace_bytes"),
                                         ("sgf_bn_bwd_stats", "sgf_colstats_workspace_bytes"),
                                         ("sgf_bn_bwd_stats2", "sgf_colstats_workspace_bytes"),
                                         ("sgf_colsum", "sgf_colsum_workspace_bytes")])
def test_workspace(lib, entry, query, dtype):
    for d in (64, 256):
        need = getattr(lib, query)(N, d)
        _rejected(lib, entry, SGF_E_WORKSPACE, d=d, dtype=dtype, workspace=None, workspace_bytes=need)
        _rejected(lib, entry, SGF_E_WORKSPACE, d=d, dtype=dtype, workspace_bytes=need - 1)
        _rejected(lib, entry, SGF_E_WORKSPACE, d=d, dtype=dtype, workspace_bytes=0)
        assert b"workspace too small" in lib.sgf_last_error()


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_nll_and_colsum_workspace(lib, dtype):
    need = lib.sgf_nll_workspace_bytes(1000)
    for c in (40, 100):                                              # both kernels of the forward
        _rejected(lib, "sgf_nll_fwd", SGF_E_WORKSPACE, c=c, dtype=dtype, workspace=None, workspace_bytes=need)
        _rejected(lib, "sgf_nll_fwd", SGF_E_WORKSPACE, c=c, dtype=dtype, workspace_bytes=need - 1)
    _rejected(lib, "sgf_colsum", SGF_E_WORKSPACE, dtype=dtype, x=None)         # a missing x is reported with the workspace
    assert b"null x or workspace too small" in lib.sgf_last_error()
