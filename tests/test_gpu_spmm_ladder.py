"""Every SpMM kernel arm, bit for bit, on a ladder of row lengths (csrc/spmm.hip: k_spmm_wave, k_spmm_row, k_spmm_seg,
k_spmm_seg_bf16x2, k_spmm_sub<1..32>, k_spmm_long_seg / _fin, k_spmm_blk lean and deep, k_spmm_blk2).

torch_sparse.matmul(adj, x) of large/ours.py:34 with operands for which the product is EXACT in fp32 in any summation order
(tests/spmm_ladder.py: values multiples of 0.5, X integers in [-3, 3], 2 * sum|terms| < 2^24, asserted on the CPU by
tests/test_spmm_ladder_host.py).  Every arm is therefore compared for EQUALITY with one integer reference; bf16 storage with
that number rounded once to nearest even.  One stored entry dropped, doubled or given to the neighbouring row changes an
output by at least 0.5; no tolerance is involved.

The CSR is the ladder itself (no CSRGraph, no normalisation): 175 rows whose lengths cover 0..34, the 64-entry piece, the
unrolled batches, LONG_ROW - 1 / LONG_ROW / LONG_ROW + 1 and long rows of 2, 3 and 4 segments, each length at three stream
offsets, with one empty 4-row wave and a ragged last one; column 0 and column n_cols - 1 occur in most rows.

Which arm a case runs is part of its id (`arm_name` / `blocked_arm_name` restate the dispatch table in Python) and is
asserted against the library's own answer, sgf_spmm_arm / sgf_spmm_blocked_arm, for the case's actual operands and switch.
y lives inside a wider buffer filled with a sentinel no result can equal, with sentinel rows behind it; x's padding columns
hold a poison value.
"""
import os

import pytest
import torch

from tests import spmm_ladder as L

pytestmark = pytest.mark.gpu

N_COLS = 97
SEED = 5
SENTINEL = 32768.0        # bf16-exact, larger than any |result| (<= 3077 * 2 * 3)
POISON = 1024.0           # in x's padding columns
GUARD_ROWS = 4
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
WIDTHS = [4, 8, 16, 20, 36, 64, 100, 128, 132, 200, 256, 260, 512]
FORCED = ["", "wave", "row", "seg", "seg2", "sub"]
ENTRIES = ["spmm", "split", "stream"]          # sgf_spmm (no queue) / sgf_spmm_split / sgf_spmm_stream (exact long_segments)
LAYOUTS = ["tight", "pad4", "pad8", "yoff4"]
ARM_CODES = {"pairs": 0, "seg": 1, "row": 2, "wave": 3, "sub": 4}
BLK_CODES = {"blk2": 0, "lean": 1, "deep": 2}
SWITCHES = ("SGF_SPMM_KERNEL", "SGF_SPMM_BLK2", "SGF_SPMM_CHUNK_ROWS")


# ---- the dispatch table, restated -----------------------------------------------------------------------------------
def layout_dims(layout, d):
    """(ldx, ldy, column offset of y in its buffer)"""
    return {"tight": (d, d, 0), "pad4": (d + 4, d + 4, 0), "pad8": (d + 8, d + 8, 0), "yoff4": (d, d + 8, 4)}[layout]


def has_pairs(dt, d, layout):
    """bf16 rows the stream kernel may fetch two per load: d, ldx, ldy multiples of 8, x and y 16-byte aligned."""
    ldx, ldy, off = layout_dims(layout, d)
    return dt == "bf16" and d % 8 == 0 and ldx % 8 == 0 and ldy % 8 == 0 and (off * 2) % 16 == 0


def arm_name(dt, d, layout, forced, stream):
    if d > 256:
        return "wave"
    if d <= 64:
        return "sub%d" % (1 if d <= 4 else 2 if d <= 8 else 4 if d <= 16 else 8 if d <= 32 else 16)
    pairs = has_pairs(dt, d, layout)
    if d <= 128:
        if not pairs or forced == "sub":
            return "sub32"
        if stream or forced in ("", "seg2"):
            return "pairs"
        return forced
    if pairs and (stream or forced == "seg2"):
        return "pairs"
    return forced if forced in ("seg", "wave") else "row"


def arm_code(name):
    return ARM_CODES["sub"] | int(name[3:]) << 8 if name.startswith("sub") else ARM_CODES[name]


def blocked_arm_name(dt, d, layout, rpb, lds_rows, blk2):
    ldx, ldy, off = layout_dims(layout, d)
    if (dt == "bf16" and d % 8 == 0 and d <= 256 and ldx % 8 == 0 and ldy % 8 == 0 and (off * 2) % 16 == 0 and rpb <= 64
            and blk2 != 0):
        return "blk2"
    waves = rpb // 8
    lds_bytes = lds_rows * 64 * (8 if dt == "bf16" else 16) + waves * 1024
    return "lean" if (160 * 1024 // lds_bytes) * waves > 16 else "deep"


# ---- the cases --------------------------------------------------------------------------------------------------------
def row_cases():
    out = []
    for dt in DTYPES:
        for d in WIDTHS:
            for forced in (FORCED if 64 < d <= 256 else [""]):
                for entry in ENTRIES:
                    for layout in LAYOUTS:
                        out.append((dt, d, forced, entry, layout, arm_name(dt, d, layout, forced, entry == "stream")))
    return out


ROW_CASES = row_cases()
# (dtype, d, forced, entry, n_rows, arm): past the row count at which xcd_remap stops being the identity for that kernel
LARGE_CASES = ([(dt, 256, f, "spmm", 40003, f) for dt in DTYPES for f in ("wave", "row", "seg")] +
               [("bf16", 256, "", "stream", 40003, "pairs")] +
               [(dt, 512, "", "spmm", 40003, "wave") for dt in DTYPES] +
               [("f32", 128, "", "spmm", 70001, "sub32")])
# both stream kernels (16-row blocks) under SGF_SPMM_CHUNK_ROWS: (dtype, d, forced, entry, csr, chunk rows, arm).
# 16 rows = one block per chunk on the ladder: xcd_remap with chunk 1 is the IDENTITY (((j / 1) * 8 + xcd) * 1 + 0 = b), the
# case covers the smallest chunk the switch can ask for and nothing of the permutation.  32 rows = two blocks per chunk, a
# stripe of 16 blocks, on 3001 rows of lengths (7 i) mod 40 (row ends at every place of a group): 188 blocks, 176 of them
# permuted, a 12-block identity tail.  tests/test_spmm_ladder_host.py works both facts out from xcd_remap restated below.
CHUNKED = ("cyclic40", 3001, N_COLS)
CHUNK_CASES = [(dt, 256, forced, entry, csr, rows, arm)
               for csr, rows in ((("ladder", 175, N_COLS), 16), (CHUNKED, 32))
               for dt, forced, entry, arm in (("f32", "seg", "split", "seg"), ("bf16", "seg", "split", "seg"),
                                              ("bf16", "", "stream", "pairs"))]
STREAM_BLOCK_ROWS = 16        # kWavesPerBlock * kSegRows of csrc/spmm.hip


def xcd_remap(b, nblocks, chunk):
    """csrc/spmm_shared.h: the virtual block of hardware block b (8 XCDs walk chunks of `chunk` blocks round-robin)."""
    stripe = 8 * chunk
    if b >= nblocks // stripe * stripe:
        return b
    xcd, j = b % 8, b // 8
    return ((j // chunk) * 8 + xcd) * chunk + j % chunk
LDS_ROWS = {"f32": [3, 64, 144], "bf16": [3, 64, 288]}        # 3, 64, the type's maximum (sgf_spmm_lds_rows_len)
BLOCKED_LAYOUTS = ["pad8", "yoff4"]


def blocked_cases():
    out = []
    for dt in DTYPES:
        for rpb in (8, 64, 128):
            for lds_rows in LDS_ROWS[dt]:
                for d in (36, 64, 200, 256):
                    for blk2 in (1, 0):
                        for layout in BLOCKED_LAYOUTS:
                            out.append((dt, rpb, lds_rows, d, blk2, layout, blocked_arm_name(dt, d, layout, rpb, lds_rows, blk2)))
    return out


BLOCKED_CASES = blocked_cases()
BLOCKED_LARGE = [("bf16", 64, 64, 64, 1, "pad8", "blk2"), ("f32", 64, 64, 64, 1, "pad8", "deep")]
BLOCKED_LARGE_ROWS = 40003


def _id(case):
    return "-".join("auto" if v == "" else "%s%d" % v[:2] if isinstance(v, tuple) else str(v) for v in case)


# every (csr, d) whose reference is built; tests/test_spmm_ladder_host.py checks the exactness bound for each of them
def csr_of(key):
    kind, n_rows, n_cols = key
    return L.ladder(n_cols, SEED) if kind == "ladder" else L.cyclic(n_rows, int(kind[6:] or 6), n_cols, SEED)


LADDER = ("ladder", 175, N_COLS)
SQUARE = ("ladder", 175, 175)
OPERANDS = sorted({(LADDER, d) for d in WIDTHS} | {(("cyclic", c[4], N_COLS), c[1]) for c in LARGE_CASES} |
                  {(c[4], c[1]) for c in CHUNK_CASES} | {(SQUARE, c[3]) for c in BLOCKED_CASES} |
                  {(("cyclic", BLOCKED_LARGE_ROWS, BLOCKED_LARGE_ROWS), c[3]) for c in BLOCKED_LARGE})

_csr_cache, _ref_cache, _dev_cache = {}, {}, {}


def get_csr(key):
    if key not in _csr_cache:
        _csr_cache[key] = csr_of(key)
    return _csr_cache[key]


def get_operand(key, d):
    """(x int64 [n_cols, d], exact reference float64 [n_rows, d], worst sum of |terms|), built once per (csr, d)."""
    if (key, d) not in _ref_cache:
        _, rowptr, colind, val = get_csr(key)
        x = L.operand(key[2], d, 100 + d)
        _ref_cache[(key, d)] = (x,) + L.reference(rowptr, colind, val, x)
    return _ref_cache[(key, d)]


def _device_csr(key, dev):
    if ("csr", key) not in _dev_cache:
        _dev_cache[("csr", key)] = tuple(t.to(dev) for t in get_csr(key)[1:])
    return _dev_cache[("csr", key)]


def _device_expected(key, d, dtype, dev):
    if ("exp", key, d, dtype) not in _dev_cache:
        _dev_cache[("exp", key, d, dtype)] = L.expected(get_operand(key, d)[1], dtype).to(dev)
    return _dev_cache[("exp", key, d, dtype)]


# ---- running one case ---------------------------------------------------------------------------------------------------
@pytest.fixture
def switches():
    """Set library switches for one case; the teardown removes them and makes the library read its defaults again."""
    from sgformer_amd import _lib

    def set_(**kw):
        for name, value in kw.items():
            os.environ[name] = str(value)
        _lib.load().sgf_reload_env()

    yield set_
    for name in SWITCHES:
        os.environ.pop(name, None)
    _lib.load().sgf_reload_env()


def _buffers(key, d, dtype, layout, dev):
    """x as the first d columns of an ldx-wide buffer (padding poisoned), y inside a sentinel-filled buffer with guard rows."""
    n_rows, n_cols = key[1], key[2]
    ldx, ldy, off = layout_dims(layout, d)
    xbuf = torch.full((n_cols, ldx), POISON, dtype=dtype, device=dev)
    xbuf[:, :d] = get_operand(key, d)[0].to(dev).to(dtype)
    ybuf = torch.full((n_rows + GUARD_ROWS, ldy), SENTINEL, dtype=dtype, device=dev)
    return xbuf[:, :d], ybuf, ybuf[:n_rows, off:off + d]


def _aligned16(x, y):
    return int(x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0)


def _check(key, d, dtype, ybuf, y, off, what):
    want = _device_expected(key, d, dtype, y.device)
    if not torch.equal(y, want):
        lens = get_csr(key)[0]
        bad = (y != want).nonzero()
        rows = sorted({int(r) for r in bad[:, 0].tolist()})
        r, c = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} wrong outputs in {len(rows)} rows; rows (length) "
                             f"{[(q, int(lens[q])) for q in rows[:12]]}; first at [{r}, {c}]: got {float(y[r, c])}, "
                             f"want {float(want[r, c])}")
    mask = torch.ones_like(ybuf, dtype=torch.bool)
    mask[:y.shape[0], off:off + d] = False
    assert bool((ybuf[mask] == SENTINEL).all()), f"{what}: wrote outside y"


def _run_rows(cuda, switches, key, dt, d, forced, entry, layout, arm, **extra):
    from sgformer_amd import _lib, ops
    dtype = DTYPES[dt]
    switches(SGF_SPMM_KERNEL=forced, **extra)
    lens = get_csr(key)[0]
    rowptr, colind, val = _device_csr(key, cuda)
    x, ybuf, y = _buffers(key, d, dtype, layout, cuda)
    got = _lib.load().sgf_spmm_arm(d, _lib.SGF_BF16 if dt == "bf16" else _lib.SGF_F32, x.stride(0), y.stride(0), key[2],
                                   _aligned16(x, y), int(entry == "stream"))
    assert got == arm_code(arm), f"the library would run arm {got & 255} (lanes {got >> 8}), the case is named {arm}"
    segs = 0 if entry == "spmm" else L.long_segments(lens)
    out = ops.K.spmm(rowptr, colind, val, x, key[1], out=y, long_segments=segs, stream_hint=entry == "stream")
    assert out.data_ptr() == y.data_ptr()
    _check(key, d, dtype, ybuf, y, layout_dims(layout, d)[2], f"{arm} {dt} d={d} {entry} {layout}")


@pytest.mark.parametrize("dt,d,forced,entry,layout,arm", ROW_CASES, ids=[_id(c) for c in ROW_CASES])
def test_row_kernels_on_the_ladder(cuda, switches, dt, d, forced, entry, layout, arm):
    """sgf_spmm: the 1025..3077-entry rows at full length in the row kernel; _split / _stream: the same rows through the
    long-row queue (k_spmm_long_seg / _fin), which every arm feeds."""
    _run_rows(cuda, switches, LADDER, dt, d, forced, entry, layout, arm)


@pytest.mark.parametrize("dt,d,forced,entry,csr,chunk_rows,arm", CHUNK_CASES, ids=[_id(c) for c in CHUNK_CASES])
def test_stream_kernels_under_the_chunk_switch(cuda, switches, dt, d, forced, entry, csr, chunk_rows, arm):
    """The chunk_blocks argument of k_spmm_seg / k_spmm_seg_bf16x2: one block per chunk on the ladder (an identity mapping)
    and two blocks per chunk on 3001 rows, where 176 of the 188 blocks are dealt over the XCDs."""
    _run_rows(cuda, switches, csr, dt, d, forced, entry, "tight", arm, SGF_SPMM_CHUNK_ROWS=chunk_rows)


@pytest.mark.parametrize("dt,d,forced,entry,n_rows,arm", LARGE_CASES, ids=[_id(c) for c in LARGE_CASES])
def test_row_kernels_past_the_remap_threshold(cuda, switches, dt, d, forced, entry, n_rows, arm):
    """More than one full stripe of blocks (8 XCDs x 1024 blocks of the wave-per-row kernels = 32 768 rows; 65 536 rows for
    k_spmm_sub<32>; 8 x 256 blocks of 16 rows for the stream kernels), plus a ragged tail."""
    _run_rows(cuda, switches, ("cyclic", n_rows, N_COLS), dt, d, forced, entry, "tight", arm)


_plans = {}


def _run_blocked(cuda, switches, key, dt, rpb, lds_rows, d, blk2, layout, arm):
    from sgformer_amd import _lib, ops
    dtype = DTYPES[dt]
    switches(SGF_SPMM_BLK2=blk2)
    lens = get_csr(key)[0]
    rowptr, colind, val = _device_csr(key, cuda)
    if (key, dt, rpb, lds_rows) not in _plans:
        _plans[(key, dt, rpb, lds_rows)] = ops.BlockedPlan(rowptr, colind, val, key[1], dtype, rows_per_block=rpb,
                                                           lds_rows=lds_rows)
    plan = _plans[(key, dt, rpb, lds_rows)]
    x, ybuf, y = _buffers(key, d, dtype, layout, cuda)
    got = _lib.load().sgf_spmm_blocked_arm(d, _lib.SGF_BF16 if dt == "bf16" else _lib.SGF_F32, x.stride(0), y.stride(0),
                                           key[1], rpb, lds_rows, _aligned16(x, y))
    assert got == BLK_CODES[arm], f"the library would run arm {got}, the case is named {arm}"
    ops.K.spmm_blocked(rowptr, plan, x, key[1], out=y, long_segments=L.long_segments(lens))
    _check(key, d, dtype, ybuf, y, layout_dims(layout, d)[2], f"{arm} {dt} d={d} rpb={rpb} lds_rows={lds_rows} {layout}")
    return plan


@pytest.mark.parametrize("dt,rpb,lds_rows,d,blk2,layout,arm", BLOCKED_CASES, ids=[_id(c) for c in BLOCKED_CASES])
def test_row_block_kernels_on_the_ladder(cuda, switches, dt, rpb, lds_rows, d, blk2, layout, arm):
    """The square ladder (n_cols = n_rows = 175: sgf_spmm_blocked bounds x by n_rows) through sgf_spmm_plan: rows mix LDS
    and gathered entries, the long rows keep plain ids and go through the queue."""
    plan = _run_blocked(cuda, switches, SQUARE, dt, rpb, lds_rows, d, blk2, layout, arm)
    assert 0 < plan.lds_entries < plan.nnz                  # both kinds of entries are exercised


@pytest.mark.parametrize("dt,rpb,lds_rows,d,blk2,layout,arm", BLOCKED_LARGE, ids=[_id(c) for c in BLOCKED_LARGE])
def test_row_block_kernels_past_the_remap_threshold(cuda, switches, dt, rpb, lds_rows, d, blk2, layout, arm):
    """40 003 rows in 64-row blocks: 626 blocks, one stripe is 8 x 64."""
    _run_blocked(cuda, switches, ("cyclic", BLOCKED_LARGE_ROWS, BLOCKED_LARGE_ROWS), dt, rpb, lds_rows, d, blk2, layout, arm)
