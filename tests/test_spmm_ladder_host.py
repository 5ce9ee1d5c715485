"""GPU-free guards of tests/test_gpu_spmm_ladder.py: the ladder holds the row lengths the kernels' paths turn on, its
operands meet the exactness bound the bit-exact comparisons rest on (so that a mismatch on the GPU can only be a kernel's),
the store's bf16 rounding is really exercised, and the case grid runs every arm the dispatch table allows."""
import numpy as np
import pytest
import torch

from tests import spmm_ladder as L
from tests import test_gpu_spmm_ladder as G


def test_constants_match_the_library():
    from sgformer_amd import _lib, kernels
    assert L.LONG_ROW == kernels.LONG_ROW
    if not _lib.available():
        pytest.skip("libsgf.so not built (run `make`)")
    lib = _lib.load()
    assert lib.sgf_spmm_segment_len() == L.SEGMENT
    assert [lib.sgf_spmm_lds_rows_len(_lib.SGF_F32), lib.sgf_spmm_lds_rows_len(_lib.SGF_BF16)] == \
        [G.LDS_ROWS["f32"][-1], G.LDS_ROWS["bf16"][-1]]


def test_ladder_shape():
    lens, rowptr, colind, val = L.ladder(G.N_COLS, G.SEED)
    lens = lens.tolist()
    assert len(lens) == 175 and int(rowptr[-1]) == 43131 == sum(lens) and colind.numel() == val.numel() == 43131
    assert len(lens) % 4 == 3                                            # the last 4-row wave is ragged
    assert lens[:4] == [0, 0, 0, 0]                                      # wave 0 of the stream kernels owns only empty rows
    need = set(range(35)) | {47, 48, 49, 63, 64, 65, 127, 128, 129, 255, 256, 257, L.LONG_ROW - 1, L.LONG_ROW, L.LONG_ROW + 1,
                             2 * L.SEGMENT - 1, 2 * L.SEGMENT, 2 * L.SEGMENT + 1, 3 * L.SEGMENT + 5}
    assert need == set(L.B)
    starts = rowptr[:-1].tolist()
    for b in L.B:
        at = [i for i, n in enumerate(lens) if n == b]
        assert len(at) >= 3, b
        if b > 1:                # three different places in a wave's stream: both parities of the start, different rows of the wave
            assert len({starts[i] % 2 for i in at}) == 2 or len({i % 4 for i in at}) >= 2, b
    assert len({starts[i] % 2 for i, n in enumerate(lens) if n > 1}) == 2
    # long rows: 2, 3 and 4 segments, last segments that are full and that hold one entry
    long_rows = [n for n in lens if n > L.LONG_ROW]
    assert {-(-n // L.SEGMENT) for n in long_rows} == {2, 3, 4}
    assert {n % L.SEGMENT for n in long_rows} >= {0, 1}
    assert L.long_segments(lens) == 3 * (2 + 2 + 2 + 3 + 4)
    # columns: sorted inside each row, inside [0, n_cols), both ends of x in most rows
    col = colind.numpy()
    rp = rowptr.numpy()
    assert col.min() == 0 and col.max() == G.N_COLS - 1
    ends = [(col[rp[i]] == 0, col[rp[i + 1] - 1] == G.N_COLS - 1) for i in range(175) if lens[i] >= 16]
    assert all(a and b for a, b in ends)
    assert all(np.all(np.diff(col[rp[i]:rp[i + 1]]) >= 0) for i in range(175))
    assert any(np.any(np.diff(col[rp[i]:rp[i + 1]]) == 0) for i in range(175))     # duplicates are kept
    assert set(val.tolist()) == set(L.VALUES)


def test_the_chunk_cases_permute_the_blocks_where_they_say_so():
    """xcd_remap (restated in the GPU file) for the block counts and chunks of the cases that turn on it: a bijection every
    time; the identity for one-block chunks; a real permutation for the two-block chunks of the 3001-row case and for the
    default chunks of the cases past the stripe."""
    def mapping(n_rows, rows_per_block, chunk):
        nb = -(-n_rows // rows_per_block)
        m = [G.xcd_remap(b, nb, chunk) for b in range(nb)]
        assert sorted(m) == list(range(nb))
        return m, sum(1 for b, v in enumerate(m) if v != b)

    for c in G.CHUNK_CASES:
        chunk = max(c[5] // G.STREAM_BLOCK_ROWS, 1)
        m, moved = mapping(c[4][1], G.STREAM_BLOCK_ROWS, chunk)
        if c[5] == 16:
            assert chunk == 1 and moved == 0
        else:
            assert chunk == 2 and len(m) == 188 and moved >= 150 and m[176:] == list(range(176, 188))
            assert m[:4] == [0, 2, 4, 6] and m[8:10] == [1, 3]           # XCD x walks blocks 2 x, 2 x + 1 of a stripe
    assert {c[5] for c in G.CHUNK_CASES} == {16, 32} and {(c[0], c[-1]) for c in G.CHUNK_CASES if c[5] == 32} == \
        {("f32", "seg"), ("bf16", "seg"), ("bf16", "pairs")}
    lens = G.get_csr(G.CHUNKED)[0].tolist()
    assert set(lens) == set(range(40))
    # default chunks: (rows per block, blocks per chunk) of each kernel the large cases run - kChunkBlocks = 1024 for the
    # wave-per-row and sub kernels, 4096 rows for the stream kernels
    geometry = {"wave": (4, 1024), "row": (4, 1024), "sub32": (8, 1024), "seg": (16, 256), "pairs": (16, 256)}
    for c in G.LARGE_CASES:
        _, moved = mapping(c[4], *geometry[c[5]])
        assert moved > 1000, c
    for c in G.BLOCKED_LARGE:
        _, moved = mapping(G.BLOCKED_LARGE_ROWS, c[1], 4096 // c[1])
        assert moved > 100, c


def test_cyclic_shape():
    lens, rowptr, colind, _ = L.cyclic(40003, 6, G.N_COLS, G.SEED)
    assert lens.tolist()[:8] == [0, 1, 2, 3, 4, 5, 0, 1] and int(rowptr[-1]) == colind.numel()
    assert int(colind.min()) == 0 and int(colind.max()) == G.N_COLS - 1


@pytest.mark.parametrize("key,d", G.OPERANDS, ids=[f"{k[0]}{k[1]}x{k[2]}-d{d}" for k, d in G.OPERANDS])
def test_every_operand_is_exact_in_fp32(key, d):
    """2 * max sum|terms| < 2^24: all partial sums, in any order, are multiples of 0.5 below 2^23 in magnitude."""
    x, ref, worst = G.get_operand(key, d)
    assert int(x.min()) == -3 and int(x.max()) == 3
    assert 0 < 2 * worst < L.EXACT, worst
    assert torch.equal(x.to(torch.bfloat16).to(torch.int64), x)          # bf16 storage holds X exactly
    assert torch.equal(ref.float().double(), ref)
    lens = G.get_csr(key)[0]
    assert bool((ref[lens == 0] == 0).all()) and float(ref.abs().max()) < G.SENTINEL


def _orders(rowptr, colind, val, x):
    """fp32 accumulation of every row in three orders the kernels use."""
    rp, col, v = rowptr.numpy(), colind.numpy().astype(np.int64), val.numpy()
    xf = x.numpy().astype(np.float32)
    n, d = rp.size - 1, xf.shape[1]
    seq, halves, seg = (np.zeros((n, d), dtype=np.float32) for _ in range(3))

    def chain(t):                                            # sequential fp32 sum into an accumulator that starts at +0
        return np.add.accumulate(np.concatenate([np.zeros((1, d), dtype=np.float32), t]), axis=0, dtype=np.float32)[-1]

    for i in range(n):
        t = v[rp[i]:rp[i + 1], None] * xf[col[rp[i]:rp[i + 1]]]
        assert t.dtype == np.float32
        seq[i] = chain(t)
        odd = rp[i] % 2                                      # even / odd STREAM positions, the halves added when the row ends
        halves[i] = chain(t[odd::2]) + chain(t[1 - odd::2])
        total = np.zeros(d, dtype=np.float32)
        for s in range(0, t.shape[0], L.SEGMENT):            # k_spmm_long_seg: wave w takes the 64-entry pieces w, w + 4, ...
            piece = t[s:s + L.SEGMENT]
            waves = [chain(np.concatenate([piece[p:p + 64] for p in range(64 * w, piece.shape[0], 256)] or [piece[:0]]))
                     for w in range(4)]
            part = waves[0]
            for w in range(1, 4):
                part = part + waves[w]
            total = total + part                             # k_spmm_long_fin: partials in segment order
        seg[i] = total
    return seq, halves, seg


def test_three_summation_orders_reproduce_the_reference_bit_for_bit():
    _, rowptr, colind, val = L.ladder(G.N_COLS, G.SEED)
    x = L.operand(G.N_COLS, 16, 116)
    ref, worst = L.reference(rowptr, colind, val, x)
    assert 2 * worst < L.EXACT
    want = L.expected(ref, torch.float32).numpy()
    for got in _orders(rowptr, colind, val, x):
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_reference_agrees_with_a_dense_product():
    _, rowptr, colind, val = L.ladder(G.N_COLS, G.SEED)
    x = L.operand(G.N_COLS, 8, 3)
    a = torch.zeros(175, G.N_COLS, dtype=torch.float64)
    rows = torch.repeat_interleave(torch.arange(175), rowptr[1:] - rowptr[:-1])
    a.index_put_((rows, colind.long()), val.double(), accumulate=True)
    ref, worst = L.reference(rowptr, colind, val, x)
    assert torch.equal(ref, a @ x.double())
    small, worst2 = L.reference(rowptr, colind, val, x, budget_bytes=4096)        # many chunks: the same numbers
    assert torch.equal(small, ref) and worst2 == worst


def test_bf16_rounding_is_exercised():
    """At least 1 % of the bf16 outputs are not bf16 numbers before the store rounds them."""
    for d in (16, 256):
        _, ref, _ = G.get_operand(G.LADDER, d)
        y = ref.float()
        frac = float((y.to(torch.bfloat16).float() != y).float().mean())
        assert frac >= 0.01, (d, frac)


def test_the_grid_runs_every_arm_the_table_allows():
    """Every (arm, dtype, entry) the dispatch table can produce at the ladder's widths runs at least once on tight rows and
    once on padded ones (pairs needs 8-element pitches: its padded layout is pad8)."""
    ran = {}
    for dt, d, forced, entry, layout, arm in G.ROW_CASES:
        ran.setdefault((arm, dt, entry), set()).add(layout)
    arms = {"wave", "row", "seg", "sub1", "sub2", "sub4", "sub8", "sub16", "sub32"}
    want = {(a, dt, e) for a in arms for dt in G.DTYPES for e in G.ENTRIES} | {("pairs", "bf16", e) for e in G.ENTRIES}
    assert set(ran) == want, set(ran) ^ want
    for k, layouts in ran.items():
        assert "tight" in layouts and layouts & {"pad4", "pad8", "yoff4"}, (k, layouts)
    assert {c[-1] for c in G.BLOCKED_CASES} == {"blk2", "lean", "deep"}
    assert {(c[0], c[-1]) for c in G.BLOCKED_CASES} >= {("bf16", "blk2"), ("bf16", "lean"), ("bf16", "deep"), ("f32", "lean"),
                                                       ("f32", "deep")}
    assert {(c[0], c[-1]) for c in G.BLOCKED_LARGE} == {("bf16", "blk2"), ("f32", "deep")}
    assert len({G._id(c) for c in G.ROW_CASES}) == len(G.ROW_CASES)


def test_case_names_agree_with_the_library():
    """arm_name / blocked_arm_name of the GPU file against sgf_spmm_arm / sgf_spmm_blocked_arm, for every case (16-byte aligned
    buffers, as torch allocates them)."""
    import os
    from sgformer_amd import _lib
    if not _lib.available():
        pytest.skip("libsgf.so not built (run `make`)")
    lib = _lib.load()
    code = {"f32": _lib.SGF_F32, "bf16": _lib.SGF_BF16}
    try:
        for dt, d, forced, entry, layout, arm in G.ROW_CASES:
            if os.environ.get("SGF_SPMM_KERNEL") != forced:
                os.environ["SGF_SPMM_KERNEL"] = forced
                lib.sgf_reload_env()
            ldx, ldy, off = G.layout_dims(layout, d)
            aligned = int(off * (2 if dt == "bf16" else 4) % 16 == 0)
            assert lib.sgf_spmm_arm(d, code[dt], ldx, ldy, G.N_COLS, aligned, int(entry == "stream")) == G.arm_code(arm), \
                (dt, d, forced, entry, layout, arm)
        for n_rows, (dt, rpb, lds_rows, d, blk2, layout, arm) in ([(175, c) for c in G.BLOCKED_CASES] +
                                                                  [(G.BLOCKED_LARGE_ROWS, c) for c in G.BLOCKED_LARGE]):
            os.environ["SGF_SPMM_BLK2"] = str(blk2)
            lib.sgf_reload_env()
            ldx, ldy, off = G.layout_dims(layout, d)
            aligned = int(off * (2 if dt == "bf16" else 4) % 16 == 0)
            assert lib.sgf_spmm_blocked_arm(d, code[dt], ldx, ldy, n_rows, rpb, lds_rows, aligned) == G.BLK_CODES[arm], \
                (dt, rpb, lds_rows, d, blk2, layout, arm)
    finally:
        os.environ.pop("SGF_SPMM_KERNEL", None)
        os.environ.pop("SGF_SPMM_BLK2", None)
        lib.sgf_reload_env()
