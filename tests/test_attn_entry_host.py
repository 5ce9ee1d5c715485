"""Argument checks of the attention stages (sgf_attn_*), the attention-from-h stages (sgf_attn_h_*) and the Gram family
(sgf_gram, sgf_gram2, sgf_gram_bn_bwd, sgf_gram_ln_bwd, sgf_gram2_bn_bwd), through ctypes on the CPU.

Every call here is rejected (or returns SGF_OK for an empty product that needs no memset) on the host BEFORE any HIP call, so
the file runs without a GPU.  Pointer arguments are dummy, suitably aligned host addresses that are never dereferenced.  The
status values are those of include/sgf.h; after a rejection sgf_last_error() starts with the name of the entry that was called.
(sgf_attn_tile_rows / sgf_attn_max_blocks: tests/test_attn_laps_host.py.)
"""
import pytest

SGF_OK, SGF_E_INVALID, SGF_E_WORKSPACE, SGF_E_UNSUPPORTED = 0, -1, -2, -4
F32, BF16, F32X = 0, 1, 2
A = 0x10000              # a 64 KiB-aligned dummy address
N = 65536                # rows: past every "too few tiles" threshold (sgf_gram2 pairs from 16 tiles, gramx from 4096 rows)
BIG = 1 << 40            # a workspace size that is never the reason for a rejection

# argument names in the order of include/sgf.h; a name that is not a scalar below is a leading dimension (ld*) or a pointer
SIGS = {
    "sgf_attn_fwd_reduce": "q ldq k ldk v ldv n heads v_heads d dtype stats workspace workspace_bytes stream",
    "sgf_attn_fwd_apply": "q ldq v ldv n n_total heads v_heads d dtype stats out ldo den o_heads stream",
    "sgf_attn_bwd_reduce": "q ldq g ldg o ldo den n heads d dtype bstats workspace workspace_bytes stream",
    "sgf_attn_bwd_apply": "q ldq k ldk v ldv g ldg o ldo den n n_total heads v_heads d dtype stats bstats dq lddq dk lddk dv "
                          "lddv stream",
    "sgf_attn_h_fwd": "h ldh n d dtype M m_vec w beta out ldo den stream",
    "sgf_attn_h_bwd_reduce": "h ldh g ldg o ldo den n d dtype hstats workspace workspace_bytes stream",
    "sgf_attn_h_bwd_apply": "h ldh g ldg o ldo den n d dtype M w D ds dh lddh workspace workspace_bytes stream",
    "sgf_attn_h_bwd_pre": "g ldg o ldo den n d dtype M w workspace workspace_bytes rowscal stream",
    "sgf_attn_h_bwd_reduce_scaled": "h ldh g ldg rowscal n d dtype hstats workspace workspace_bytes stream",
    "sgf_attn_h_bwd_post": "h ldh n d dtype D ds workspace workspace_bytes addend ldadd dh lddh stream",
    "sgf_gram": "a lda m b ldb k n dtype c ldc colsum workspace workspace_bytes stream",
    "sgf_gram2": "a lda m b1 ldb1 b2 ldb2 k n dtype c1 ldc1 c2 ldc2 colsum workspace workspace_bytes stream",
    "sgf_gram_bn_bwd": "g1 ldg1 g2 ldg2 z ldz mean rstd gamma beta relu stats inv_n training m b ldb k n dtype c ldc colsum "
                       "workspace workspace_bytes stream",
    "sgf_gram_ln_bwd": "g ldg xin ldx mean rstd gamma beta relu m b ldb k n dtype c ldc colsum dgamma dbeta workspace "
                       "workspace_bytes stream",
    "sgf_gram2_bn_bwd": "g ldg z ldz mean rstd gamma beta relu stats inv_n training m b1 ldb1 b2 ldb2 k n dtype dz lddz c1 ldc1 "
                        "c2 ldc2 colsum workspace workspace_bytes stream",
}
SIGS["sgf_attn_bwd_reduce_heads"] = SIGS["sgf_attn_bwd_reduce"]
SIGS["sgf_attn_bwd_apply_heads"] = SIGS["sgf_attn_bwd_apply"]
SCALARS = dict(n=N, n_total=float(N), heads=1, v_heads=1, d=64, m=64, k=64, dtype=BF16, relu=0, training=1, inv_n=1.0,
               workspace_bytes=BIG, stream=None)

ATTN = ["sgf_attn_fwd_reduce", "sgf_attn_fwd_apply", "sgf_attn_bwd_reduce", "sgf_attn_bwd_apply", "sgf_attn_bwd_reduce_heads",
        "sgf_attn_bwd_apply_heads"]
ATTN_H = ["sgf_attn_h_fwd", "sgf_attn_h_bwd_reduce", "sgf_attn_h_bwd_apply"]
ATTN_H_SPLIT = ["sgf_attn_h_bwd_pre", "sgf_attn_h_bwd_reduce_scaled", "sgf_attn_h_bwd_post"]
GRAM_PLAIN = ["sgf_gram", "sgf_gram2"]
GRAM_FUSED = ["sgf_gram_bn_bwd", "sgf_gram_ln_bwd", "sgf_gram2_bn_bwd"]

# the pointers each entry refuses as null when n > 0 (outputs, statistics and operands)
REQUIRED = {
    "sgf_attn_fwd_reduce": "stats q k v",
    "sgf_attn_fwd_apply": "stats q v out den",
    "sgf_attn_bwd_reduce": "bstats q g o den",
    "sgf_attn_bwd_reduce_heads": "bstats q g o den",
    "sgf_attn_bwd_apply": "stats bstats q k v g o den dq dk dv",
    "sgf_attn_bwd_apply_heads": "stats bstats q k v g o den dq dk dv",
    "sgf_attn_h_fwd": "h M m_vec w beta out den",
    "sgf_attn_h_bwd_reduce": "hstats h g o den",
    "sgf_attn_h_bwd_apply": "h g o den M w D ds dh",
    "sgf_attn_h_bwd_pre": "g o den M w rowscal",
    "sgf_attn_h_bwd_reduce_scaled": "hstats h g rowscal",
    "sgf_attn_h_bwd_post": "h D ds dh",
    "sgf_gram": "c a b",
    "sgf_gram2": "c1 c2 a b1 b2",
    "sgf_gram_bn_bwd": "c g1 z b mean rstd stats",
    "sgf_gram_ln_bwd": "c g xin b mean rstd",
}


@pytest.fixture(scope="module")
def lib():
    from sgformer_amd import _lib
    if not _lib.available():
        pytest.skip("libsgf.so not built (run `make`)")
    return _lib.load()


def _call(lib, entry, **kw):
    """One call of `entry` with plausible arguments (every pointer A, every leading dimension 256) except those in `kw`."""
    names = SIGS[entry].split()
    assert set(kw) <= set(names), (entry, sorted(set(kw) - set(names)))
    args = [kw[a] if a in kw else SCALARS[a] if a in SCALARS else 256 if a.startswith("ld") else A for a in names]
    return getattr(lib, entry)(*args)


def _rejected(lib, entry, code, prefix=None, **kw):
    assert _call(lib, entry, **kw) == code, lib.sgf_last_error()
    assert lib.sgf_last_error().startswith((prefix or entry).encode() + b":"), lib.sgf_last_error()


# ---- sizes, widths and dtype codes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ATTN + ATTN_H + ATTN_H_SPLIT)
def test_attention_common_checks(lib, entry):
    _rejected(lib, entry, SGF_E_INVALID, dtype=7)
    assert b"unknown dtype 7" in lib.sgf_last_error()
    _rejected(lib, entry, SGF_E_INVALID, n=-1)
    _rejected(lib, entry, SGF_E_INVALID, d=0)
    if entry in ATTN:
        _rejected(lib, entry, SGF_E_INVALID, heads=0)
    _rejected(lib, entry, SGF_E_UNSUPPORTED, d=6)                    # not a multiple of 4
    _rejected(lib, entry, SGF_E_UNSUPPORTED, d=260)                  # wider than 256
    _rejected(lib, entry, SGF_E_UNSUPPORTED, d=260, dtype=7)         # the width is judged before the dtype code
    if entry not in ATTN_H:                                          # only the three row passes from h take SGF_F32_BF16X3
        _rejected(lib, entry, SGF_E_INVALID, dtype=F32X)
        assert b"unknown dtype 2" in lib.sgf_last_error()


@pytest.mark.parametrize("entry", GRAM_PLAIN)
def test_gram_common_checks(lib, entry):
    _rejected(lib, entry, SGF_E_INVALID, dtype=7)
    assert b"unknown dtype 7" in lib.sgf_last_error()
    _rejected(lib, entry, SGF_E_INVALID, m=0)
    _rejected(lib, entry, SGF_E_INVALID, k=0)
    _rejected(lib, entry, SGF_E_INVALID, n=-1)
    _rejected(lib, entry, SGF_E_UNSUPPORTED, m=6)
    _rejected(lib, entry, SGF_E_UNSUPPORTED, k=6)
    _rejected(lib, entry, SGF_E_UNSUPPORTED, k=6, dtype=7)           # the sizes are judged before the dtype code
    _rejected(lib, entry, SGF_E_INVALID, ldc=60) if entry == "sgf_gram" else _rejected(lib, entry, SGF_E_INVALID, ldc2=60)


@pytest.mark.parametrize("entry", GRAM_FUSED)
def test_fused_gram_supported_set(lib, entry):
    """bf16 storage only, m and k multiples of 4 (sgf_gram2_bn_bwd: of 8) up to 256; everything else is UNSUPPORTED."""
    for kw in (dict(dtype=F32), dict(dtype=F32X), dict(dtype=7), dict(m=0), dict(m=6), dict(k=6), dict(m=260), dict(k=260)):
        _rejected(lib, entry, SGF_E_UNSUPPORTED, **kw)
    if entry != "sgf_gram2_bn_bwd":
        _rejected(lib, entry, SGF_E_INVALID, n=-1)
        _rejected(lib, entry, SGF_E_INVALID, n=-1, dtype=F32)        # a negative n is reported first
        _rejected(lib, entry, SGF_E_INVALID, ldc=60)


def test_gram_ln_bwd_needs_a_whole_lane_group_per_row(lib):
    _rejected(lib, "sgf_gram_ln_bwd", SGF_E_UNSUPPORTED, m=96)
    _rejected(lib, "sgf_gram_ln_bwd", SGF_E_UNSUPPORTED, m=32)
    assert [lib.sgf_gram_ln_bwd_supported(m, 64, BF16) for m in (32, 64, 96, 128, 256)] == [0, 1, 0, 1, 1]
    assert lib.sgf_gram_bn_bwd_supported(96, 64, BF16) == 1 and lib.sgf_gram_bn_bwd_supported(96, 64, F32) == 0


def test_gram2_bn_bwd_is_opt_in(lib):
    assert lib.sgf_gram2_bn_bwd_supported(64, 64, N, BF16) == 0      # SGF_GRAM_BN2 unset
    _rejected(lib, "sgf_gram2_bn_bwd", SGF_E_UNSUPPORTED)


@pytest.mark.parametrize("entry", ATTN_H_SPLIT)
def test_split_backward_supported_set(lib, entry):
    """bf16 storage; sgf_attn_h_bwd_pre / _post also need d in {64, 128, 256}."""
    _rejected(lib, entry, SGF_E_UNSUPPORTED, dtype=F32)
    if entry != "sgf_attn_h_bwd_reduce_scaled":
        _rejected(lib, entry, SGF_E_UNSUPPORTED, d=32)
        _rejected(lib, entry, SGF_E_UNSUPPORTED, d=192)
    assert [lib.sgf_attn_h_bwd_split_supported(d, BF16) for d in (32, 64, 128, 192, 256)] == [0, 1, 1, 0, 1]
    assert lib.sgf_attn_h_bwd_split_supported(64, F32) == 0


@pytest.mark.parametrize("entry", ["sgf_attn_fwd_reduce", "sgf_attn_fwd_apply", "sgf_attn_bwd_apply", "sgf_attn_bwd_apply_heads"])
def test_v_heads_is_one_or_all(lib, entry):
    _rejected(lib, entry, SGF_E_INVALID, heads=4, v_heads=2)
    _rejected(lib, entry, SGF_E_INVALID, heads=2, v_heads=3)
    _rejected(lib, entry, SGF_E_INVALID, heads=2, v_heads=0)
    assert b"v_heads must be H or 1" in lib.sgf_last_error()


@pytest.mark.parametrize("entry", ["sgf_attn_bwd_reduce_heads", "sgf_attn_bwd_apply_heads"])
def test_per_head_gradient_rows_hold_every_head(lib, entry):
    _rejected(lib, entry, SGF_E_INVALID, heads=2, d=64, ldg=64)
    assert b"ldg < H * d" in lib.sgf_last_error()
    _rejected(lib, entry, SGF_E_INVALID, heads=2, d=64, ldg=124)
    if entry == "sgf_attn_bwd_reduce_heads":                         # reported before the workspace
        _rejected(lib, entry, SGF_E_INVALID, heads=2, d=64, ldg=64, workspace=None)


# ---- null pointers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", sorted(REQUIRED))
def test_null_pointers(lib, entry):
    for name in REQUIRED[entry].split():
        _rejected(lib, entry, SGF_E_INVALID, **{name: None})
        assert b"null" in lib.sgf_last_error(), (name, lib.sgf_last_error())


def test_null_pointers_that_depend_on_a_flag(lib):
    _rejected(lib, "sgf_attn_fwd_apply", SGF_E_INVALID, heads=2, o_heads=None)
    _rejected(lib, "sgf_gram_bn_bwd", SGF_E_WORKSPACE, training=0, stats=None, workspace=None)   # eval mode reads no stats
    _rejected(lib, "sgf_gram_bn_bwd", SGF_E_WORKSPACE, g2=None, workspace=None)                  # g2 is optional


@pytest.mark.parametrize("entry", ["sgf_attn_fwd_reduce", "sgf_attn_bwd_reduce", "sgf_attn_bwd_reduce_heads"])
def test_null_statistics_with_no_rows(lib, entry):
    """n == 0 makes the operands optional, never the output."""
    out = "stats" if entry == "sgf_attn_fwd_reduce" else "bstats"
    _rejected(lib, entry, SGF_E_INVALID, n=0, **{out: None})


# ---- workspace --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("entry", ["sgf_attn_fwd_reduce", "sgf_attn_bwd_reduce", "sgf_attn_bwd_reduce_heads"])
def test_attention_reduce_workspace(lib, entry, heads):
    need = lib.sgf_attn_workspace_bytes(N, heads, 64)
    assert need == heads * lib.sgf_attn_workspace_bytes(N, 1, 64) > 0
    _rejected(lib, entry, SGF_E_WORKSPACE, heads=heads, workspace=None, workspace_bytes=need)
    _rejected(lib, entry, SGF_E_WORKSPACE, heads=heads, workspace_bytes=need - 1)
    _rejected(lib, entry, SGF_E_WORKSPACE, heads=heads, workspace_bytes=need - 1, n=0)     # asked for with no rows too


@pytest.mark.parametrize("dtype", [F32, BF16, F32X])
def test_h_bwd_reduce_workspace(lib, dtype):
    need = lib.sgf_attn_workspace_bytes(N, 1, 64)
    _rejected(lib, "sgf_attn_h_bwd_reduce", SGF_E_WORKSPACE, dtype=dtype, workspace=None, workspace_bytes=need)
    _rejected(lib, "sgf_attn_h_bwd_reduce", SGF_E_WORKSPACE, dtype=dtype, workspace_bytes=need - 1)


def test_h_bwd_reduce_scaled_workspace(lib):
    need = lib.sgf_attn_workspace_bytes(N, 1, 64)
    _rejected(lib, "sgf_attn_h_bwd_reduce_scaled", SGF_E_WORKSPACE, workspace=None, workspace_bytes=need)
    _rejected(lib, "sgf_attn_h_bwd_reduce_scaled", SGF_E_WORKSPACE, workspace_bytes=need - 1)


@pytest.mark.parametrize("entry,dtype", [(e, t) for e in GRAM_PLAIN for t in (F32, BF16, F32X)] +
                         [("sgf_gram_bn_bwd", BF16), ("sgf_gram_ln_bwd", BF16)])
def test_gram_workspace(lib, entry, dtype):
    need = lib.sgf_gram_workspace_bytes(N, 64, 64)
    assert need > 0
    # sgf_gram2 hands fp32 storage to sgf_gram, whose name the message then carries
    prefix = "sgf_gram" if entry == "sgf_gram2" and dtype != BF16 else entry
    _rejected(lib, entry, SGF_E_WORKSPACE, prefix, dtype=dtype, workspace=None, workspace_bytes=need)
    _rejected(lib, entry, SGF_E_WORKSPACE, prefix, dtype=dtype, workspace_bytes=need - 1)


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("entry", ["sgf_attn_h_bwd_apply", "sgf_attn_h_bwd_pre", "sgf_attn_h_bwd_post"])
def test_row_kernel_workspace(lib, entry, d):
    n = 1000                                                         # rounded up to whole 32-row tiles of bf16
    need = lib.sgf_attn_h_bwd_apply_workspace_bytes(n, d, BF16)
    assert need == 1024 * d * 2
    _rejected(lib, entry, SGF_E_WORKSPACE, n=n, d=d, workspace=None, workspace_bytes=need)
    _rejected(lib, entry, SGF_E_WORKSPACE, n=n, d=d, workspace_bytes=need - 1)
    _rejected(lib, entry, SGF_E_WORKSPACE, n=n, d=d, workspace=A + 8, workspace_bytes=need)      # not 16-byte aligned


def test_row_kernel_workspace_bytes_outside_the_row_kernels(lib):
    q = lib.sgf_attn_h_bwd_apply_workspace_bytes
    assert q(0, 64, BF16) == 0 and q(-1, 64, BF16) == 0 and q(1000, 64, F32) == 0 and q(1000, 32, BF16) == 0


# ---- alignment: one entry of each shared body, fp32 and bf16 -------------------------------------------------------------
def _esz(dtype):
    return 2 if dtype == BF16 else 4


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("entry,operand,after_workspace", [
    ("sgf_gram", "a", True), ("sgf_gram", "b", True),
    ("sgf_attn_h_fwd", "h", None), ("sgf_attn_h_fwd", "out", None),
    ("sgf_attn_h_bwd_reduce", "g", True),
    ("sgf_attn_h_bwd_apply", "o", None), ("sgf_attn_h_bwd_apply", "dh", None),
    ("sgf_attn_fwd_reduce", "k", True),
    ("sgf_attn_fwd_apply", "q", None),
    ("sgf_attn_bwd_reduce", "o", True), ("sgf_attn_bwd_reduce_heads", "o", True),
    ("sgf_attn_bwd_apply", "g", None), ("sgf_attn_bwd_apply_heads", "g", None),
])
def test_operand_misaligned_by_one_element(lib, entry, operand, after_workspace, dtype):
    _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **{operand: A + _esz(dtype)})
    assert b"align" in lib.sgf_last_error()
    if after_workspace:
        _rejected(lib, entry, SGF_E_WORKSPACE, dtype=dtype, workspace=None, **{operand: A + _esz(dtype)})


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("entry,ld", [("sgf_gram", "lda"), ("sgf_attn_h_fwd", "ldh"), ("sgf_attn_h_bwd_reduce", "ldo"),
                                      ("sgf_attn_h_bwd_apply", "ldg"), ("sgf_attn_fwd_reduce", "ldv"),
                                      ("sgf_attn_fwd_apply", "ldq"), ("sgf_attn_bwd_reduce", "ldq"),
                                      ("sgf_attn_bwd_reduce_heads", "ldq"), ("sgf_attn_bwd_apply", "ldk"),
                                      ("sgf_attn_bwd_apply_heads", "ldv")])
def test_leading_dimension_not_a_multiple_of_four(lib, entry, ld, dtype):
    _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **{ld: 258})


def test_gram_f32x_operand_alignment(lib):
    _rejected(lib, "sgf_gram", SGF_E_INVALID, dtype=F32X, b=A + 4)


def test_fwd_apply_checks_alignment_before_its_empty_return(lib):
    _rejected(lib, "sgf_attn_fwd_apply", SGF_E_INVALID, n=0, q=A + 2)


def test_bf16_only_bodies_alignment(lib):
    for operand in ("a", "b1", "b2"):
        _rejected(lib, "sgf_gram2", SGF_E_INVALID, **{operand: A + 2})
        _rejected(lib, "sgf_gram2", SGF_E_WORKSPACE, workspace=None, **{operand: A + 2})
    for operand in ("g1", "g2", "z", "b"):
        _rejected(lib, "sgf_gram_bn_bwd", SGF_E_INVALID, **{operand: A + 2})
        _rejected(lib, "sgf_gram_bn_bwd", SGF_E_WORKSPACE, workspace=None, **{operand: A + 2})
    for operand in ("g", "xin", "b"):
        _rejected(lib, "sgf_gram_ln_bwd", SGF_E_INVALID, **{operand: A + 2})
        _rejected(lib, "sgf_gram_ln_bwd", SGF_E_WORKSPACE, workspace=None, **{operand: A + 2})
    # the scaled reduce judges alignment BEFORE its workspace
    for kw in (dict(h=A + 2), dict(g=A + 2), dict(rowscal=A + 4), dict(ldh=258)):
        _rejected(lib, "sgf_attn_h_bwd_reduce_scaled", SGF_E_INVALID, workspace=None, **kw)


def test_row_kernel_entries_need_16_byte_rows(lib):
    """sgf_attn_h_bwd_pre / _post: rows before the workspace, the optional addend after it."""
    for kw in (dict(g=A + 2), dict(g=A + 8), dict(o=A + 8), dict(ldg=260), dict(rowscal=A + 4)):
        _rejected(lib, "sgf_attn_h_bwd_pre", SGF_E_INVALID, workspace=None, **kw)
    for kw in (dict(h=A + 8), dict(dh=A + 2), dict(lddh=260)):
        _rejected(lib, "sgf_attn_h_bwd_post", SGF_E_INVALID, workspace=None, **kw)
    for kw in (dict(addend=A + 8), dict(ldadd=260), dict(ldadd=32)):
        _rejected(lib, "sgf_attn_h_bwd_post", SGF_E_INVALID, **kw)
        _rejected(lib, "sgf_attn_h_bwd_post", SGF_E_WORKSPACE, workspace=None, **kw)


# ---- sgf_gram2 that has nothing to pair becomes two sgf_gram calls, before its own null and workspace checks ------------------
@pytest.mark.parametrize("kw", [dict(dtype=F32), dict(dtype=F32X), dict(m=260, ldc1=512, ldc2=512), dict(k=260, ldc1=512, ldc2=512),
                                dict(n=8)], ids=["f32", "f32x", "m>256", "k>256", "few-tiles"])
def test_gram2_without_a_pair_reports_as_gram(lib, kw):
    _rejected(lib, "sgf_gram2", SGF_E_INVALID, "sgf_gram", a=None, **kw)
    _rejected(lib, "sgf_gram2", SGF_E_INVALID, "sgf_gram", b1=None, **kw)
    _rejected(lib, "sgf_gram2", SGF_E_WORKSPACE, "sgf_gram", workspace=None, **kw)
    _rejected(lib, "sgf_gram2", SGF_E_INVALID, "sgf_gram", a=A + 2, **kw)
    _rejected(lib, "sgf_gram2", SGF_E_INVALID, c2=None, **kw)        # its own output check comes first


# ---- sgf_gram2_bn_bwd with its switch on ------------------------------------------------------------------------------------
@pytest.fixture
def gram_bn2(lib, monkeypatch):
    monkeypatch.setenv("SGF_GRAM_BN2", "1")
    monkeypatch.delenv("SGF_GRAMX", raising=False)
    lib.sgf_reload_env()
    yield "sgf_gram2_bn_bwd"
    monkeypatch.undo()
    lib.sgf_reload_env()


def test_gram2_bn_bwd_checks(lib, gram_bn2):
    assert lib.sgf_gram2_bn_bwd_supported(64, 64, N, BF16) == 1
    _rejected(lib, gram_bn2, SGF_E_UNSUPPORTED, n=16383)
    _rejected(lib, gram_bn2, SGF_E_UNSUPPORTED, m=68)                # multiples of 8
    _rejected(lib, gram_bn2, SGF_E_UNSUPPORTED, dtype=F32)
    for name in "g z b1 b2 dz c1 c2 mean rstd stats".split():
        _rejected(lib, gram_bn2, SGF_E_INVALID, **{name: None})
    _rejected(lib, gram_bn2, SGF_E_WORKSPACE, training=0, stats=None, workspace=None)
    for kw in (dict(ldc1=60), dict(ldc2=60), dict(lddz=60)):
        _rejected(lib, gram_bn2, SGF_E_INVALID, **kw)
    for kw in (dict(g=A + 8), dict(z=A + 2), dict(b1=A + 8), dict(b2=A + 8), dict(dz=A + 8), dict(ldg=260)):
        _rejected(lib, gram_bn2, SGF_E_INVALID, workspace=None, **kw)       # alignment before the workspace
    need = lib.sgf_gram_workspace_bytes(N, 64, 64)
    _rejected(lib, gram_bn2, SGF_E_WORKSPACE, workspace=None, workspace_bytes=need)
    _rejected(lib, gram_bn2, SGF_E_WORKSPACE, workspace_bytes=need - 1)


# ---- empty products that need no memset -------------------------------------------------------------------------------------
def test_empty_row_passes_are_ok_with_null_pointers(lib):
    nulls = dict(h=None, g=None, o=None, den=None, M=None, w=None, D=None, ds=None, dh=None, workspace=None, workspace_bytes=0)
    for dtype in (F32, BF16, F32X):
        assert _call(lib, "sgf_attn_h_fwd", n=0, dtype=dtype, h=None, M=None, m_vec=None, w=None, beta=None, out=None,
                     den=None) == SGF_OK
        assert _call(lib, "sgf_attn_h_bwd_apply", n=0, dtype=dtype, **nulls) == SGF_OK
    assert _call(lib, "sgf_attn_h_bwd_pre", n=0, g=None, o=None, den=None, M=None, w=None, rowscal=None, workspace=None,
                 workspace_bytes=0) == SGF_OK
    assert _call(lib, "sgf_attn_h_bwd_post", n=0, h=None, D=None, ds=None, dh=None, addend=None, workspace=None,
                 workspace_bytes=0) == SGF_OK


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_empty_apply_stages_are_ok_without_operands(lib, dtype):
    """n == 0: the statistics are still required, the row operands are not (aligned: null)."""
    assert _call(lib, "sgf_attn_fwd_apply", n=0, dtype=dtype, heads=2, q=None, v=None, out=None, den=None, o_heads=None) == SGF_OK
    for entry in ("sgf_attn_bwd_apply", "sgf_attn_bwd_apply_heads"):
        assert _call(lib, entry, n=0, dtype=dtype, heads=2, q=None, k=None, v=None, g=None, o=None, den=None, dq=None, dk=None,
                     dv=None, ldg=4) == SGF_OK
        _rejected(lib, entry, SGF_E_INVALID, n=0, dtype=dtype, bstats=None)
