"""Argument checks of the SpMM entry points (sgf_spmm, sgf_spmm_split, sgf_spmm_stream, sgf_spmm_blocked,
sgf_spmm_tile) and the long-row workspace formula, through ctypes on the CPU.

Every call here is rejected (or returns SGF_OK for an empty product) on the host BEFORE any HIP call, so the file runs
without a GPU.  Pointer arguments are dummy, suitably aligned host addresses that are never dereferenced.
"""
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
