"""Argument checks of the SpMM entry points (sgf_spmm, sgf_spmm_split, sgf_spmm_stream, sgf_spmm_blocked,
sgf_spmm_tile), the long-row workspace formula and the dispatch queries (sgf_spmm_arm, sgf_spmm_blocked_arm: which kernel
a launch would run), through ctypes on the CPU.

Every call here is rejected (or returns SGF_OK for an empty product) on the host BEFORE any HIP call, so the file runs
without a GPU.  Pointer arguments are dummy, suitably aligned host addresses that are never dereferenced.
"""
import os

import pytest

SGF_OK, SGF_E_INVALID, SGF_E_WORKSPACE = 0, -1, -2
F32, BF16 = 0, 1
A = 0x10000              # a 64 KiB-aligned dummy address
LONG = 1024
ROW_ENTRIES = ["sgf_spmm", "sgf_spmm_split", "sgf_spmm_stream", "sgf_spmm_blocked"]
QUEUE_ENTRIES = ["sgf_spmm_split", "sgf_spmm_stream", "sgf_spmm_blocked", "sgf_spmm_tile"]


@pytest.fixture(scope="module")
def lib():
    from sgformer_amd import _lib
    if not _lib.available():
        pytest.skip("libsgf.so not built (run `make`)")
    return _lib.load()


def _call(lib, entry, *, x=A, ldx=256, y=A, ldy=256, n_rows=10, d=256, dtype=BF16, long_len=LONG, long_segments=0,
          ws=None, ws_bytes=0, ptr=A):
    """One call of `entry` with plausible arguments; `ptr` stands for every pointer other than x, y and the workspace."""
    if entry == "sgf_spmm":
        return lib.sgf_spmm(ptr, ptr, ptr, x, ldx, 10, y, ldy, n_rows, d, dtype, None)
    if entry in ("sgf_spmm_split", "sgf_spmm_stream"):
        return getattr(lib, entry)(ptr, ptr, ptr, x, ldx, 10, y, ldy, n_rows, d, dtype, long_len, long_segments, ws,
                                   ws_bytes, None)
    if entry == "sgf_spmm_blocked":
        return lib.sgf_spmm_blocked(ptr, ptr, ptr, ptr, ptr, ptr, x, ldx, y, ldy, n_rows, d, dtype, 64, 16, long_len,
                                    long_segments, ws, ws_bytes, None)
    assert entry == "sgf_spmm_tile"
    return lib.sgf_spmm_tile(ptr, 1, 128, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, x, ldx, 10, y, ldy, n_rows, d, dtype,
                             long_len, long_segments, ws, ws_bytes, None)


def _rejected(lib, entry, code, **kw):
    assert _call(lib, entry, **kw) == code
    assert lib.sgf_last_error().startswith(entry.encode() + b":"), lib.sgf_last_error()


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("entry", ROW_ENTRIES)
def test_operand_checks(lib, entry, dtype):
    esz = 2 if dtype == BF16 else 4
    _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, d=6)                       # d not a multiple of 4
    _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, d=64, ldx=60)              # ldx < d
    _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, x=A + esz)                 # x misaligned by one element
    _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, x=None)                    # null x


@pytest.mark.parametrize("entry", ROW_ENTRIES)
def test_unknown_dtype(lib, entry):
    _rejected(lib, entry, SGF_E_INVALID, dtype=7)
    assert b"unknown dtype 7" in lib.sgf_last_error()


@pytest.mark.parametrize("entry", QUEUE_ENTRIES)
def test_long_row_queue_checks(lib, entry):
    d = 256
    need = lib.sgf_spmm_split_workspace_bytes(3, d)
    _rejected(lib, entry, SGF_E_INVALID, long_len=0)
    _rejected(lib, entry, SGF_E_INVALID, long_segments=-1)
    _rejected(lib, entry, SGF_E_WORKSPACE, long_segments=3, ws=None, ws_bytes=need)
    _rejected(lib, entry, SGF_E_WORKSPACE, long_segments=3, ws=A, ws_bytes=need - 1)


@pytest.mark.parametrize("s,d", [(0, 256), (1, 4), (3, 256), (17, 128)])
def test_split_workspace_bytes(lib, s, d):
    """256 bytes for the counter, the 16-byte entries rounded up to 256 bytes, one fp32 partial row per segment."""
    assert lib.sgf_spmm_split_workspace_bytes(s, d) == 256 + (16 * s + 255) // 256 * 256 + 4 * s * d


def test_split_workspace_bytes_of_a_negative_argument(lib):
    assert lib.sgf_spmm_split_workspace_bytes(-1, 256) == 0
    assert lib.sgf_spmm_split_workspace_bytes(3, -4) == 0


@pytest.mark.parametrize("entry", ROW_ENTRIES)
def test_empty_product_is_ok_with_null_pointers(lib, entry):
    assert _call(lib, entry, x=None, y=None, ptr=None, n_rows=0) == SGF_OK
    assert _call(lib, entry, x=None, y=None, ptr=None, d=0) == SGF_OK


# ---- which kernel a launch runs (csrc/spmm.hip: choose_kernel / choose_blocked behind the launchers AND these queries) ----
PAIRS, SEG, ROW, WAVE, SUB = 0, 1, 2, 3, 4                 # sgf_spmm_arm: arm | lanes_per_row << 8


def sub(lanes):
    return SUB | lanes << 8


@pytest.fixture
def switch(lib):
    """Set one of the library's cached switches; the teardown removes both and makes the library read its defaults again."""
    def set_(name, value):
        os.environ[name] = value
        lib.sgf_reload_env()

    yield set_
    os.environ.pop("SGF_SPMM_KERNEL", None)
    os.environ.pop("SGF_SPMM_BLK2", None)
    lib.sgf_reload_env()


FORCED = ["", "wave", "row", "seg", "seg2", "sub"]
# operands: (d, dtype, ldx, ldy, aligned16);  expectation per forced word: {word: (stream off, stream on)}
SAME = lambda arm: {f: (arm, arm) for f in FORCED}          # noqa: E731
F32_WIDE = {"": (ROW, ROW), "row": (ROW, ROW), "seg2": (ROW, ROW), "sub": (ROW, ROW), "seg": (SEG, SEG), "wave": (WAVE, WAVE)}
PAIRS_WIDE = {"": (ROW, PAIRS), "row": (ROW, PAIRS), "sub": (ROW, PAIRS), "seg": (SEG, PAIRS), "wave": (WAVE, PAIRS),
              "seg2": (PAIRS, PAIRS)}
PAIRS_NARROW = {"": (PAIRS, PAIRS), "seg2": (PAIRS, PAIRS), "sub": (sub(32), sub(32)), "seg": (SEG, PAIRS), "row": (ROW, PAIRS),
                "wave": (WAVE, PAIRS)}
ARM_TABLE = [
    # d > 256: wave, whatever is forced
    ((260, F32, 260, 260, 1), SAME(WAVE)), ((512, BF16, 512, 512, 1), SAME(WAVE)), ((264, BF16, 264, 264, 1), SAME(WAVE)),
    # d <= 64: sub, lanes by width
    ((4, F32, 4, 4, 1), SAME(sub(1))), ((8, BF16, 8, 8, 1), SAME(sub(2))), ((12, F32, 12, 12, 1), SAME(sub(4))),
    ((16, BF16, 16, 16, 1), SAME(sub(4))), ((20, F32, 20, 20, 1), SAME(sub(8))), ((32, BF16, 32, 32, 1), SAME(sub(8))),
    ((36, F32, 36, 36, 1), SAME(sub(16))), ((64, BF16, 64, 64, 1), SAME(sub(16))), ((64, F32, 72, 64, 0), SAME(sub(16))),
    # fp32, 128 < d <= 256
    ((132, F32, 132, 132, 1), F32_WIDE), ((200, F32, 200, 208, 1), F32_WIDE), ((256, F32, 256, 256, 1), F32_WIDE),
    ((256, F32, 256, 256, 0), F32_WIDE),
    # fp32, 64 < d <= 128: sub<32>
    ((68, F32, 68, 68, 1), SAME(sub(32))), ((100, F32, 100, 100, 1), SAME(sub(32))), ((128, F32, 128, 128, 1), SAME(sub(32))),
    # bf16 with pairs, 128 < d <= 256
    ((136, BF16, 136, 136, 1), PAIRS_WIDE), ((200, BF16, 208, 200, 1), PAIRS_WIDE), ((256, BF16, 256, 256, 1), PAIRS_WIDE),
    ((256, BF16, 264, 512, 1), PAIRS_WIDE),
    # bf16 with pairs, 64 < d <= 128
    ((72, BF16, 72, 72, 1), PAIRS_NARROW), ((128, BF16, 128, 128, 1), PAIRS_NARROW), ((104, BF16, 104, 112, 1), PAIRS_NARROW),
    # bf16 without pairs: the fp32 rows
    ((100, BF16, 100, 100, 1), SAME(sub(32))), ((100, BF16, 104, 104, 1), SAME(sub(32))), ((128, BF16, 132, 128, 1), SAME(sub(32))),
    ((128, BF16, 128, 132, 1), SAME(sub(32))), ((128, BF16, 128, 128, 0), SAME(sub(32))),
    ((132, BF16, 132, 132, 1), F32_WIDE), ((132, BF16, 136, 136, 1), F32_WIDE), ((256, BF16, 260, 256, 1), F32_WIDE),
    ((256, BF16, 256, 260, 1), F32_WIDE), ((256, BF16, 256, 256, 0), F32_WIDE), ((200, BF16, 204, 204, 1), F32_WIDE),
]


@pytest.mark.parametrize("forced", FORCED)
def test_spmm_arm_table(lib, switch, forced):
    switch("SGF_SPMM_KERNEL", forced)
    for (d, dtype, ldx, ldy, aligned), want in ARM_TABLE:
        for stream in (0, 1):
            got = lib.sgf_spmm_arm(d, dtype, ldx, ldy, 97, aligned, stream)
            assert got == want[forced][stream], (d, dtype, ldx, ldy, aligned, forced, stream, got)
            if got & 255 != SUB:
                assert got >> 8 == 0


@pytest.mark.parametrize("forced", FORCED)
def test_spmm_arm_beyond_32_bit_offsets(lib, switch, forced):
    """n_cols * ldx * element size >= 2^32: no buffer addressing, so wave for d > 128 (and sub below, as ever)."""
    switch("SGF_SPMM_KERNEL", forced)
    for dtype, esz in ((F32, 4), (BF16, 2)):
        n_cols = (1 << 32) // (256 * esz)
        for stream in (0, 1):
            assert lib.sgf_spmm_arm(256, dtype, 256, 256, n_cols, 1, stream) == WAVE
            assert lib.sgf_spmm_arm(136, dtype, 256, 256, n_cols, 1, stream) == WAVE
            assert lib.sgf_spmm_arm(128, dtype, 256, 256, n_cols, 1, stream) == sub(32)
            assert lib.sgf_spmm_arm(256, dtype, 256, 256, n_cols - 1, 1, stream) != WAVE or forced == "wave"
    assert lib.sgf_spmm_arm(256, F32, 256, 256, 0, 1, 0) == WAVE          # an empty x: nothing to describe by a buffer


def test_spmm_arm_follows_the_switch_only_after_a_reload(lib, switch):
    switch("SGF_SPMM_KERNEL", "")
    assert lib.sgf_spmm_arm(256, F32, 256, 256, 97, 1, 0) == ROW
    os.environ["SGF_SPMM_KERNEL"] = "seg"                                 # cached: the launcher would not see it either
    assert lib.sgf_spmm_arm(256, F32, 256, 256, 97, 1, 0) == ROW
    lib.sgf_reload_env()
    assert lib.sgf_spmm_arm(256, F32, 256, 256, 97, 1, 0) == SEG
    switch("SGF_SPMM_KERNEL", "no such kernel")
    assert lib.sgf_spmm_arm(256, F32, 256, 256, 97, 1, 0) == ROW


def test_arm_queries_reject_what_the_entries_reject(lib):
    assert lib.sgf_spmm_arm(256, 7, 256, 256, 97, 1, 0) == -1
    assert lib.sgf_spmm_blocked_arm(256, 7, 256, 256, 1000, 64, 16, 1) == -1
    for rpb, lds_rows, dtype in ((0, 16, BF16), (12, 16, BF16), (136, 16, BF16), (64, 0, BF16), (64, 289, BF16), (64, 145, F32)):
        assert lib.sgf_spmm_blocked_arm(256, dtype, 256, 256, 1000, rpb, lds_rows, 1) == -1, (rpb, lds_rows, dtype)


BLK2, LEAN, DEEP = 0, 1, 2
# k_spmm_blk's register budget by the LDS a block takes: lds_rows * (512 B bf16 | 1 KiB fp32) + 1 KiB per wave of 8 rows; lean
# when floor(160 KiB / that) blocks of rows_per_block / 8 waves are more than 16 waves per CU
BLOCKED_TABLE = [
    # (d, dtype, ldx, ldy, n_rows, rows_per_block, lds_rows, aligned16) -> (SGF_SPMM_BLK2 = 1, = 0)
    ((256, BF16, 256, 256, 1000, 64, 144, 1), (BLK2, DEEP)),       # 80 KiB: 2 blocks x 8 waves = 16: deep
    ((256, BF16, 256, 256, 1000, 64, 64, 1), (BLK2, LEAN)),        # 40 KiB: 4 x 8 = 32: lean
    ((256, BF16, 256, 256, 1000, 8, 3, 1), (BLK2, LEAN)),          # 2.5 KiB: 64 x 1
    ((256, BF16, 256, 256, 1000, 8, 288, 1), (BLK2, DEEP)),        # 145 KiB: 1 x 1
    ((64, BF16, 64, 72, 1000, 32, 16, 1), (BLK2, LEAN)),
    ((200, BF16, 200, 200, 1000, 64, 64, 1), (BLK2, LEAN)),
    ((200, BF16, 208, 264, 1000, 64, 64, 1), (BLK2, LEAN)),
    # each condition of blk2 in turn
    ((256, F32, 256, 256, 1000, 64, 64, 1), (DEEP, DEEP)),         # fp32 storage; 72 KiB: 2 x 8 = 16
    ((256, F32, 256, 256, 1000, 64, 32, 1), (LEAN, LEAN)),         # 40 KiB
    ((36, BF16, 40, 40, 1000, 64, 64, 1), (LEAN, LEAN)),           # d % 8
    ((100, BF16, 104, 104, 1000, 64, 64, 1), (LEAN, LEAN)),
    ((256, BF16, 260, 256, 1000, 64, 64, 1), (LEAN, LEAN)),        # ldx % 8
    ((256, BF16, 256, 260, 1000, 64, 64, 1), (LEAN, LEAN)),        # ldy % 8
    ((256, BF16, 256, 256, 1000, 64, 64, 0), (LEAN, LEAN)),        # alignment
    ((256, BF16, 256, 256, 1000, 72, 64, 1), (LEAN, LEAN)),        # more than 64 rows per block; 41 KiB: 3 x 9
    ((256, BF16, 256, 256, 1000, 128, 288, 1), (DEEP, DEEP)),      # 160 KiB: 1 x 16
    ((256, BF16, 256, 256, 1000, 128, 64, 1), (LEAN, LEAN)),       # 48 KiB: 3 x 16
    ((256, BF16, 256, 256, 1 << 23, 64, 64, 1), (LEAN, LEAN)),     # x beyond 32-bit offsets
    ((256, BF16, 256, 256, (1 << 23) - 1, 64, 64, 1), (BLK2, LEAN)),
    ((256, F32, 256, 256, 1000, 128, 144, 1), (DEEP, DEEP)),
    ((256, F32, 256, 256, 1000, 8, 3, 1), (LEAN, LEAN)),
]


@pytest.mark.parametrize("blk2", ["1", "0", ""])
def test_spmm_blocked_arm_table(lib, switch, blk2):
    switch("SGF_SPMM_BLK2", blk2)
    for args, want in BLOCKED_TABLE:
        assert lib.sgf_spmm_blocked_arm(*args) == want[blk2 == "0"], (args, blk2)
