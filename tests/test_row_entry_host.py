"""Argument checks of the row-kernel entries of csrc/rowgemm.hip (sgf_gcn_epilogue_*, sgf_gcn_bn_bwd_dx, sgf_stem_pair), through
ctypes on the CPU.

Every call here is rejected (or returns SGF_OK for an empty problem that has no statistics to zero) on the host BEFORE any HIP
call, so the file runs without a GPU.  Pointer arguments are dummy, suitably aligned host addresses that are never dereferenced.
The status values are those of include/sgf.h; after a rejection sgf_last_error() starts with the name of the entry that was
called.  (sgf_row_lap_rows and the launch geometry: tests/test_row_laps_host.py.)
"""
import re

import pytest

SGF_OK, SGF_E_INVALID, SGF_E_WORKSPACE, SGF_E_UNSUPPORTED = 0, -1, -2, -4
F32, BF16, F32X = 0, 1, 2
A = 0x10000              # a 64 KiB-aligned dummy address
N = 65536                # rows: past every "too few tiles" threshold of the paired launches
BIG = 1 << 40            # a buffer size that is never the reason for a rejection
LD = 512                 # default leading dimension: holds [W1 | W2] at d = 256

# argument names in the order of include/sgf.h; a name that is not a scalar below is a leading dimension (ld*) or a pointer
SIGS = {
    "sgf_gcn_epilogue_stats": "a lda w ldw bias n d_in d_out dtype y ldy shift stats workspace workspace_bytes stream",
    "sgf_gcn_epilogue_dx": "dy lddy w ldw n d_in d_out dtype dx lddx stream",
    "sgf_gcn_epilogue_dx2": "dy lddy w1 w2 ldw n d dtype dx1 lddx1 dx2 lddx2 pair stream",
    "sgf_gcn_epilogue_dx2_acc": "dz lddz w ldw n d dtype dy lddy gadd ldg acc_in ldai acc_out ldao stream",
    "sgf_gcn_bn_bwd_dx": "gy ldg z ldz mean rstd gamma beta relu stats inv_n training w ldw n d dtype dz lddz dy lddy acc_in "
                         "acc_out acc_bytes dx0 lddx0 add_gy workspace workspace_bytes stream",
    "sgf_gcn_epilogue_cat": "a1 lda1 a2 lda2 w ldw bias n d dtype y ldy shift stats workspace workspace_bytes stream",
    "sgf_gcn_epilogue_partial": "a lda w ldw bias n d_in d_out dtype partial partial_bytes stream",
    "sgf_gcn_epilogue_stats_add": "a lda w ldw partial partial_bytes n d_in d_out dtype y ldy shift stats workspace "
                                  "workspace_bytes stream",
    "sgf_gcn_epilogue_apply": "y ldy mean rstd gamma beta res ldr relu n d dtype out ldo stream",
    "sgf_stem_pair": "x ldx n d_in w0 ldw0 bias0 w1 ldw1 bias1 d_out dtype y0 ldy0 y1 ldy1 shift0 stats0 workspace "
                     "workspace_bytes stream",
}
SCALARS = dict(n=N, d=64, d_in=64, d_out=64, dtype=BF16, relu=0, training=1, inv_n=1.0, pair=1, add_gy=0, acc_bytes=BIG,
               partial_bytes=BIG, workspace_bytes=BIG, stream=None)
# sgf_gcn_bn_bwd_dx takes exactly one of dx0 and acc_out: the plain form writes dx0
DEFAULTS = {"sgf_gcn_bn_bwd_dx": dict(acc_in=None, acc_out=None)}

COMMON = ["sgf_gcn_epilogue_stats", "sgf_gcn_epilogue_dx", "sgf_gcn_epilogue_dx2", "sgf_gcn_epilogue_partial",
          "sgf_gcn_epilogue_stats_add"]                              # the entries that take fp32 storage too
BF16_ONLY = ["sgf_gcn_epilogue_dx2_acc", "sgf_gcn_bn_bwd_dx", "sgf_gcn_epilogue_cat"]
WITH_STATS = {"sgf_gcn_epilogue_stats": "stats", "sgf_gcn_epilogue_stats_add": "stats", "sgf_gcn_epilogue_cat": "stats",
              "sgf_stem_pair": "stats0"}

# per entry: the pointers refused as null when n > 0, the row operands (pointer, its leading dimension) and W's
REQUIRED = {
    "sgf_gcn_epilogue_stats": "a w y",
    "sgf_gcn_epilogue_dx": "dy w dx",
    "sgf_gcn_epilogue_dx2": "dy w1 w2 dx1 dx2",
    "sgf_gcn_epilogue_partial": "a w partial",
    "sgf_gcn_epilogue_stats_add": "a w y partial",
    "sgf_gcn_epilogue_dx2_acc": "dz w dy acc_out",
    "sgf_gcn_bn_bwd_dx": "gy z mean rstd w dz dy stats",
    "sgf_gcn_epilogue_cat": "a1 a2 w y",
    "sgf_gcn_epilogue_apply": "y mean rstd out",
    "sgf_stem_pair": "x w0 y0 y1",
}
ROWS = {
    "sgf_gcn_epilogue_stats": "a:lda y:ldy w:ldw",
    "sgf_gcn_epilogue_dx": "dy:lddy dx:lddx w:ldw",
    "sgf_gcn_epilogue_dx2": "dy:lddy dx1:lddx1 dx2:lddx2 w1:ldw w2:ldw",
    "sgf_gcn_epilogue_partial": "a:lda w:ldw",
    "sgf_gcn_epilogue_stats_add": "a:lda y:ldy w:ldw",
    "sgf_gcn_epilogue_dx2_acc": "dz:lddz w:ldw dy:lddy gadd:ldg acc_in:ldai acc_out:ldao",
    "sgf_gcn_bn_bwd_dx": "gy:ldg z:ldz w:ldw dz:lddz dy:lddy dx0:lddx0",
    "sgf_gcn_epilogue_cat": "a1:lda1 a2:lda2 w:ldw y:ldy",
}


def _rows(entry):
    return [tuple(t.split(":")) for t in ROWS[entry].split()]


@pytest.fixture(scope="module")
def lib():
    from sgformer_amd import _lib
    if not _lib.available():
        pytest.skip("libsgf.so not built (run `make`)")
    return _lib.load()


def _call(lib, entry, **kw):
    """One call of `entry` with plausible arguments (every pointer A, every leading dimension LD) except those in `kw`."""
    names = SIGS[entry].split()
    assert set(kw) <= set(names), (entry, sorted(set(kw) - set(names)))
    kw = {**DEFAULTS.get(entry, {}), **kw}
    args = [kw[a] if a in kw else SCALARS[a] if a in SCALARS else LD if a.startswith("ld") else A for a in names]
    return getattr(lib, entry)(*args)


def _rejected(lib, entry, code, prefix=None, **kw):
    assert _call(lib, entry, **kw) == code, lib.sgf_last_error()
    assert lib.sgf_last_error().startswith((prefix or entry).encode() + b":"), lib.sgf_last_error()


def _width(entry, d):
    return dict(d=d) if "d" in SIGS[entry].split() else dict(d_in=d, d_out=d)


# ---- the queries --------------------------------------------------------------------------------------------------------------
WIDTHS = (0, 32, 64, 100, 128, 256, 512)
DTYPES = (F32, BF16, F32X, 7)


def test_supported_queries(lib):
    row = {64, 128, 256}
    for d in WIDTHS:
        for dtype in DTYPES:
            bf16 = int(dtype == BF16 and d in row)
            f32 = int(dtype in (F32, F32X) and 0 < d <= 256 and d % 4 == 0)
            assert lib.sgf_gcn_epilogue_supported(d, d, dtype) == (bf16 or f32), (d, dtype)
            assert lib.sgf_gcn_epilogue_dx2_acc_supported(d, dtype) == bf16, (d, dtype)
            assert lib.sgf_gcn_bn_bwd_dx_supported(d, dtype) == bf16, (d, dtype)
            assert lib.sgf_gcn_epilogue_cat_supported(d, dtype) == bf16, (d, dtype)
            assert lib.sgf_stem_pair_supported(64, d, dtype) == bf16, (d, dtype)
            assert lib.sgf_stem_pair_supported(d, 64, dtype) == int(dtype == BF16 and 0 < d <= 128 and d % 4 == 0), (d, dtype)
            assert lib.sgf_row_lap_rows(0, d, dtype) == (256 * 8 * 32 if bf16 else -1), (d, dtype)
    # bf16 rows are square, fp32 rows need not be
    assert lib.sgf_gcn_epilogue_supported(64, 128, BF16) == 0
    assert lib.sgf_gcn_epilogue_supported(64, 128, F32) == 1 and lib.sgf_gcn_epilogue_supported(64, 128, F32X) == 1
    assert lib.sgf_gcn_epilogue_supported(64, 260, F32) == 0 and lib.sgf_gcn_epilogue_supported(6, 64, F32) == 0
    assert lib.sgf_stem_pair_supported(132, 64, BF16) == 0 and lib.sgf_stem_pair_supported(6, 64, BF16) == 0


def test_size_queries(lib):
    ws = lib.sgf_gcn_epilogue_workspace_bytes
    assert ws(-1, 64) == 0 and ws(10, 0) == 0 and ws(10, -4) == 0
    # one [2 * d_out] fp32 row per block: 32 rows a block, at least 8 and at most 256 of them
    assert ws(0, 64) == ws(1, 64) == ws(256, 64) == 8 * 2 * 64 * 4
    assert ws(257, 64) == 9 * 2 * 64 * 4
    assert ws(8192, 256) == ws(N, 256) == ws(1 << 40, 256) == 256 * 2 * 256 * 4
    pb, dpb = lib.sgf_gcn_epilogue_partial_bytes, lib.sgf_gcn_epilogue_dtype_partial_bytes
    assert pb(-1, 64) == 0 and pb(10, 0) == 0 and pb(0, 64) == 0
    assert pb(1, 64) == pb(32, 64) == 32 * 64 * 2 and pb(33, 128) == 64 * 128 * 2      # whole 32-row tiles of bf16
    for dtype in (BF16, 7):
        assert dpb(1000, 64, dtype) == pb(1000, 64) == 1024 * 64 * 2
    for dtype in (F32, F32X):
        assert dpb(1000, 64, dtype) == 1000 * 64 * 4                                   # a plain [n, d_out] fp32 matrix
        assert dpb(-1, 64, dtype) == 0 and dpb(10, 0, dtype) == 0
    for n, d in ((0, 64), (N, 256), (-1, 0)):
        assert lib.sgf_gcn_bn_bwd_dx_workspace_bytes(n, d) == 256 * 8 * 4              # one counter per wave of a full grid


# ---- sizes, widths and dtype codes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", COMMON)
def test_common_checks(lib, entry):
    _rejected(lib, entry, SGF_E_INVALID, n=-1)
    assert b"negative n" in lib.sgf_last_error()
    for d in (0, 32, 100, 512):
        _rejected(lib, entry, SGF_E_UNSUPPORTED, **_width(entry, d))
    for dtype in (F32, F32X):
        for d in (0, 6, 260, 512):
            _rejected(lib, entry, SGF_E_UNSUPPORTED, dtype=dtype, **_width(entry, d))
    _rejected(lib, entry, SGF_E_UNSUPPORTED, dtype=7)                # an unknown dtype code supports no width
    assert b"dtype 7" in lib.sgf_last_error()
    _rejected(lib, entry, SGF_E_INVALID, n=-1, dtype=7)              # a negative n is judged first
    _rejected(lib, entry, SGF_E_INVALID, n=-1, **_width(entry, 100))
    if "d_in" in SIGS[entry].split():
        _rejected(lib, entry, SGF_E_UNSUPPORTED, d_in=64, d_out=128)  # bf16 rows are square
        assert (b"got 128 -> 64, dtype 1" if entry == "sgf_gcn_epilogue_dx" else b"got 64 -> 128, dtype 1") in lib.sgf_last_error()


@pytest.mark.parametrize("entry", BF16_ONLY)
def test_bf16_only_checks(lib, entry):
    _rejected(lib, entry, SGF_E_INVALID, n=-1)
    assert b"negative n" in lib.sgf_last_error()
    for d in (0, 32, 100, 512):
        _rejected(lib, entry, SGF_E_UNSUPPORTED, d=d)
    for dtype in (F32, F32X, 7):
        _rejected(lib, entry, SGF_E_UNSUPPORTED, dtype=dtype)
    assert b"got d = 64, dtype 7" in lib.sgf_last_error()
    _rejected(lib, entry, SGF_E_INVALID, n=-1, d=100)                # a negative n is judged first
    _rejected(lib, entry, SGF_E_INVALID, n=-1, dtype=7)
    _rejected(lib, entry, SGF_E_UNSUPPORTED, d=100, **{REQUIRED[entry].split()[0]: None})   # the width before the pointers


def test_stem_pair_sizes(lib):
    e = "sgf_stem_pair"
    _rejected(lib, e, SGF_E_INVALID, n=-1)
    _rejected(lib, e, SGF_E_INVALID, n=-1, d_out=100)
    for kw in (dict(d_in=0), dict(d_in=6), dict(d_in=132), dict(d_in=256), dict(d_out=32), dict(d_out=100), dict(d_out=512),
               dict(dtype=F32), dict(dtype=F32X), dict(dtype=7)):
        _rejected(lib, e, SGF_E_UNSUPPORTED, **kw)
        _rejected(lib, e, SGF_E_UNSUPPORTED, x=None, **kw)           # before the pointers
    _rejected(lib, e, SGF_E_UNSUPPORTED, d_in=132, d_out=100, dtype=7)
    assert b"d_in <= 128" in lib.sgf_last_error() and b"got 132 -> 100, dtype 7" in lib.sgf_last_error()


# ---- empty problems -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", sorted(SIGS))
def test_no_rows_is_ok_before_the_pointer_checks(lib, entry):
    """n == 0 with no statistics to zero: SGF_OK with every pointer null, every leading dimension 0 and no workspace."""
    names = SIGS[entry].split()
    kw = {a: (0 if a.startswith("ld") or a.endswith("_bytes") else None) for a in names if a not in SCALARS or a.endswith("_bytes")}
    dtypes = (BF16,) if entry in BF16_ONLY + ["sgf_stem_pair"] else (BF16, F32) if entry == "sgf_gcn_epilogue_apply" else (BF16, F32, F32X)
    for dtype in dtypes:
        assert _call(lib, entry, n=0, dtype=dtype, **kw) == SGF_OK, lib.sgf_last_error()


@pytest.mark.parametrize("entry", sorted(SIGS))
def test_no_rows_still_judges_width_and_dtype(lib, entry):
    if entry == "sgf_gcn_epilogue_apply":
        _rejected(lib, entry, SGF_E_UNSUPPORTED, "sgf_bn_apply", n=0, d=6)
    else:
        _rejected(lib, entry, SGF_E_UNSUPPORTED, n=0, dtype=7)


# ---- null pointers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", sorted(REQUIRED))
def test_null_pointers(lib, entry):
    dtypes = (BF16, F32) if entry in COMMON + ["sgf_gcn_epilogue_apply"] else (BF16,)
    for dtype in dtypes:
        for name in REQUIRED[entry].split():
            _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **{name: None})
            assert b"null pointer" in lib.sgf_last_error() or name == "partial", (name, lib.sgf_last_error())
            # reported before a leading dimension, an alignment or a workspace (sgf_gcn_epilogue_dx2 judges (w1, dx1) whole first)
            if entry in ROWS and name not in ("partial", "w2", "dx2"):
                kw = {name: None, _rows(entry)[0][1]: 8}
                if "workspace" in SIGS[entry].split():
                    kw["workspace"] = None
                _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **kw)
                assert b"null pointer" in lib.sgf_last_error(), (name, lib.sgf_last_error())


def test_null_pointers_that_depend_on_an_argument(lib):
    e = "sgf_gcn_bn_bwd_dx"
    _rejected(lib, e, SGF_E_INVALID, training=0, stats=None, ldg=32)           # eval mode reads no stats: the next check speaks
    assert b"leading dimension" in lib.sgf_last_error()
    for kw in (dict(gamma=None, beta=None), dict(acc_in=None)):                # optional operands
        _rejected(lib, e, SGF_E_INVALID, ldg=32, **kw)
        assert b"leading dimension" in lib.sgf_last_error()
    _rejected(lib, e, SGF_E_INVALID, dx0=A, acc_out=A)
    assert b"exactly one of dx0" in lib.sgf_last_error()
    _rejected(lib, e, SGF_E_INVALID, dx0=None, acc_out=None)
    assert b"exactly one of dx0" in lib.sgf_last_error()
    _rejected(lib, e, SGF_E_INVALID, dx0=None, acc_out=None, ldg=32)           # judged before the leading dimensions
    assert b"exactly one of dx0" in lib.sgf_last_error()
    _rejected(lib, e, SGF_E_INVALID, dx0=None, acc_out=None, gy=None)          # and after the null pointers
    assert b"null pointer" in lib.sgf_last_error()
    e = "sgf_gcn_epilogue_dx2_acc"
    _rejected(lib, e, SGF_E_INVALID, gadd=None, acc_in=None, ldg=8, ldai=8, dz=A + 8)   # absent operands: their ld is not read
    assert b"16-byte aligned" in lib.sgf_last_error()
    e = "sgf_stem_pair"
    _rejected(lib, e, SGF_E_INVALID, w1=None, y1=None, ldw1=2, ldy1=2, ldy0=32)         # one stem only: w1 / y1 are not read
    assert b"rows of y" in lib.sgf_last_error()
    _rejected(lib, e, SGF_E_INVALID, w1=None, ldy0=32)                                  # y1 without w1 is ignored
    assert b"rows of y" in lib.sgf_last_error()
    for name in ("bias0", "bias1", "shift0"):
        _rejected(lib, e, SGF_E_INVALID, ldy0=32, **{name: None})
        assert b"rows of y" in lib.sgf_last_error()


def test_apply_forwards_to_bn_apply(lib):
    """sgf_gcn_epilogue_apply makes its own null check, everything after it is sgf_bn_apply's."""
    e = "sgf_gcn_epilogue_apply"
    _rejected(lib, e, SGF_E_INVALID, y=None, d=6)                    # its null check comes before the width
    _rejected(lib, e, SGF_E_INVALID, "sgf_bn_apply", n=-1, y=None)   # ... but only when there are rows
    for kw, code in ((dict(n=-1), SGF_E_INVALID), (dict(d=0), SGF_E_INVALID), (dict(d=6), SGF_E_UNSUPPORTED),
                     (dict(d=1028), SGF_E_UNSUPPORTED), (dict(dtype=7), SGF_E_INVALID), (dict(dtype=F32X), SGF_E_INVALID),
                     (dict(ldy=6), SGF_E_INVALID), (dict(ldo=6), SGF_E_INVALID), (dict(ldr=6), SGF_E_INVALID)):
        _rejected(lib, e, code, "sgf_bn_apply", **kw)
    _rejected(lib, e, SGF_E_UNSUPPORTED, "sgf_bn_apply", d=6, dtype=7)         # the width before the dtype code


# ---- leading dimensions and alignment -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("entry", sorted(ROWS))
def test_bf16_leading_dimension_smaller_than_the_width(lib, entry, d):
    for ptr, ld in _rows(entry):
        need = 2 * d if ptr == "w" and entry in BF16_ONLY else d
        kw = {**_width(entry, d), ld: need - 8}
        if entry == "sgf_gcn_bn_bwd_dx" and ptr == "dx0":
            kw.update(dx0=A, acc_out=None)
        _rejected(lib, entry, SGF_E_INVALID, **kw)
        assert b"leading dimension smaller than the width" in lib.sgf_last_error(), (ld, lib.sgf_last_error())
        _rejected(lib, entry, SGF_E_INVALID, **{**kw, ptr: A + 8})   # judged before the alignment
        assert b"leading dimension smaller than the width" in lib.sgf_last_error(), (ld, lib.sgf_last_error())


@pytest.mark.parametrize("entry", sorted(ROWS))
def test_bf16_rows_are_16_byte_aligned(lib, entry):
    for ptr, ld in _rows(entry):
        for kw in ({ptr: A + 8}, {ptr: A + 2}, {ld: LD + 4}, {ld: LD + 1}):
            _rejected(lib, entry, SGF_E_INVALID, **kw)
            assert b"rows must be 16-byte aligned" in lib.sgf_last_error(), (kw, lib.sgf_last_error())
            if "workspace" in SIGS[entry].split():
                _rejected(lib, entry, SGF_E_INVALID, workspace=None, **kw)     # judged before the workspace


@pytest.mark.parametrize("entry", COMMON)
def test_bf16_alignment_message_is_well_formed(lib, entry):
    ptr, ld = _rows(entry)[0]
    for kw in ({ptr: A + 8}, {ld: LD + 4}):
        _rejected(lib, entry, SGF_E_INVALID, **kw)
        assert lib.sgf_last_error() == (entry + ": rows must be 16-byte aligned (pointers % 16, leading dims % 8 elements)").encode()


@pytest.mark.parametrize("entry", BF16_ONLY)
def test_bf16_only_alignment_message(lib, entry):
    ptr, _ = _rows(entry)[0]
    _rejected(lib, entry, SGF_E_INVALID, **{ptr: A + 8})
    assert lib.sgf_last_error() == (entry + ": rows must be 16-byte aligned (pointers % 16, leading dims % 8 elements)").encode()


@pytest.mark.parametrize("dtype", [F32, F32X])
@pytest.mark.parametrize("entry", COMMON)
def test_fp32_rows(lib, entry, dtype):
    """fp32 storage: one message for width and alignment of the row operands; W's pointer and its width are not judged here."""
    for ptr, ld in _rows(entry):
        if ptr.startswith("w"):
            _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, ldw=LD + 2)
            continue
        for kw in ({ptr: A + 8}, {ptr: A + 4}, {ld: LD + 2}, {ld: 60}):
            _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **kw)
            assert lib.sgf_last_error() == (entry + ": rows must be 16-byte aligned (pointers % 16, leading dims % 4 "
                                                    "elements)").encode(), (kw, lib.sgf_last_error())
    if entry in ("sgf_gcn_epilogue_stats", "sgf_gcn_epilogue_stats_add"):
        # a misaligned or narrow W passes the argument checks: the workspace is what is refused
        for kw in (dict(w=A + 4), dict(ldw=32)):
            _rejected(lib, entry, SGF_E_WORKSPACE, dtype=dtype, workspace=None, **kw)
    if entry == "sgf_gcn_epilogue_partial":
        for kw in (dict(w=A + 4), dict(ldw=32)):
            _rejected(lib, entry, SGF_E_WORKSPACE, dtype=dtype, partial_bytes=0, **kw)


def test_dx_takes_its_widths_swapped(lib):
    """dx [n, d_in] = dy [n, d_out] W: dy is d_out wide, dx d_in."""
    e = "sgf_gcn_epilogue_dx"
    _rejected(lib, e, SGF_E_INVALID, dtype=F32, d_in=64, d_out=128, lddy=64)
    _rejected(lib, e, SGF_E_INVALID, dtype=F32, d_in=128, d_out=64, lddx=64)


def test_stem_pair_rows(lib):
    e = "sgf_stem_pair"
    for kw in (dict(ldx=32), dict(ldx=66), dict(x=A + 4), dict(x=A + 2), dict(ldw0=32), dict(ldw0=66), dict(w0=A + 4),
               dict(ldw1=32), dict(ldw1=66), dict(w1=A + 4)):
        _rejected(lib, e, SGF_E_INVALID, **kw)
        assert b"rows of x / W must be 8-byte aligned" in lib.sgf_last_error(), (kw, lib.sgf_last_error())
        _rejected(lib, e, SGF_E_INVALID, ldy0=32, workspace=None, **kw)        # before y and before the workspace
        assert b"rows of x / W must be 8-byte aligned" in lib.sgf_last_error(), (kw, lib.sgf_last_error())
    for kw in (dict(ldy0=32), dict(ldy0=LD + 4), dict(y0=A + 8), dict(ldy1=32), dict(ldy1=LD + 4), dict(y1=A + 8)):
        _rejected(lib, e, SGF_E_INVALID, **kw)
        assert b"rows of y must be 16-byte aligned" in lib.sgf_last_error(), (kw, lib.sgf_last_error())
        _rejected(lib, e, SGF_E_INVALID, workspace=None, **kw)
    for kw in (dict(x=A + 8), dict(ldx=68), dict(w0=A + 8), dict(ldw1=68)):    # 8-byte rows of x / W are enough
        _rejected(lib, e, SGF_E_WORKSPACE, workspace=None, **kw)


# ---- 32-bit byte offsets ------------------------------------------------------------------------------------------------------
def test_bn_bwd_dx_operands_stay_below_4_gib(lib):
    e = "sgf_gcn_bn_bwd_dx"
    small = dict(n=1 << 23, ldg=64, ldz=64, lddz=64, lddy=64, lddx0=64, ldw=128)          # 2^23 rows x 128 bytes = 1 GiB each
    for ld in ("ldg", "ldz", "lddz", "lddy", "lddx0"):
        _rejected(lib, e, SGF_E_UNSUPPORTED, **{**small, ld: 256})
        assert b"beyond 4 GiB" in lib.sgf_last_error()
        _rejected(lib, e, SGF_E_UNSUPPORTED, acc_in=A + 8, acc_bytes=0, **{**small, ld: 256})   # before the running sums
    _rejected(lib, e, SGF_E_WORKSPACE, dx0=None, acc_out=A, acc_bytes=0, **{**small, "lddx0": 256})   # no dx0: its ld is not read
    _rejected(lib, e, SGF_E_INVALID, gy=A + 8, **{**small, "ldg": 256})                   # the alignment comes first


# ---- partial sums, running sums and workspaces --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32, F32X])
def test_partial_buffer(lib, dtype):
    n, d = 1000, 64
    need = lib.sgf_gcn_epilogue_dtype_partial_bytes(n, d, dtype)
    e = "sgf_gcn_epilogue_partial"                                   # too small: a workspace error
    _rejected(lib, e, SGF_E_WORKSPACE, n=n, dtype=dtype, partial_bytes=need - 1)
    assert b"partial buffer %d < %d" % (need - 1, need) in lib.sgf_last_error()
    _rejected(lib, e, SGF_E_INVALID, n=n, dtype=dtype, partial_bytes=need - 1, partial=A + 8)     # after the rows
    e = "sgf_gcn_epilogue_stats_add"                                 # missing, misaligned or small: an invalid argument
    for kw in (dict(partial=None), dict(partial=A + 8), dict(partial_bytes=need - 1), dict(partial_bytes=0)):
        _rejected(lib, e, SGF_E_INVALID, n=n, dtype=dtype, **kw)
        assert b"partial buffer missing, misaligned or too small" in lib.sgf_last_error()
        _rejected(lib, e, SGF_E_INVALID, n=n, dtype=dtype, workspace=None, **kw)                  # before the workspace
    _rejected(lib, e, SGF_E_INVALID, n=n, dtype=dtype, partial=None, a=A + 8)                     # after the rows
    assert b"rows must be 16-byte aligned" in lib.sgf_last_error()


def test_bn_bwd_dx_running_sums(lib):
    e = "sgf_gcn_bn_bwd_dx"
    for d in (64, 256):
        need = lib.sgf_gcn_epilogue_partial_bytes(N, d)
        for kw in (dict(dx0=None, acc_out=A), dict(dx0=None, acc_out=A, acc_in=A), dict(acc_in=A)):
            _rejected(lib, e, SGF_E_WORKSPACE, d=d, acc_bytes=need - 1, **kw)
            assert b"running-sum buffer %d < %d" % (need - 1, need) in lib.sgf_last_error()
            _rejected(lib, e, SGF_E_WORKSPACE, d=d, acc_bytes=0, **{**kw, "acc_in" if "acc_in" in kw else "acc_out": A + 8})
    for kw in (dict(dx0=None, acc_out=A + 8), dict(dx0=None, acc_out=A, acc_in=A + 8), dict(acc_in=A + 4)):
        _rejected(lib, e, SGF_E_INVALID, **kw)
        assert b"running-sum buffers must be 16-byte aligned" in lib.sgf_last_error()


@pytest.mark.parametrize("entry,dtype", [(e, BF16) for e in sorted(WITH_STATS)] +
                         [(e, t) for e in ("sgf_gcn_epilogue_stats", "sgf_gcn_epilogue_stats_add") for t in (F32, F32X)])
def test_statistics_workspace(lib, entry, dtype):
    for n, d in ((1000, 64), (N, 256)):
        need = lib.sgf_gcn_epilogue_workspace_bytes(n, d)
        kw = dict(n=n, dtype=dtype, **({"d_out": d} if entry == "sgf_stem_pair" else _width(entry, d)))
        _rejected(lib, entry, SGF_E_WORKSPACE, workspace=None, workspace_bytes=need, **kw)
        _rejected(lib, entry, SGF_E_WORKSPACE, workspace_bytes=need - 1, **kw)
        _rejected(lib, entry, SGF_E_WORKSPACE, workspace_bytes=0, **kw)


@pytest.mark.parametrize("entry,dtype", [(e, BF16) for e in sorted(WITH_STATS)] +
                         [(e, t) for e in ("sgf_gcn_epilogue_stats", "sgf_gcn_epilogue_stats_add") for t in (F32, F32X)])
def test_statistics_workspace_message(lib, entry, dtype):
    need = lib.sgf_gcn_epilogue_workspace_bytes(1000, 64)
    _rejected(lib, entry, SGF_E_WORKSPACE, n=1000, dtype=dtype, workspace_bytes=need - 1)
    assert re.fullmatch(b"%s: workspace %d < %d" % (entry.encode(), need - 1, need), lib.sgf_last_error()), lib.sgf_last_error()
