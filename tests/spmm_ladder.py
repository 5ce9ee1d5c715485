"""Inputs and the exact reference of the SpMM ladder tests (tests/test_gpu_spmm_ladder.py, tests/test_spmm_ladder_host.py).
CPU only, plain torch / numpy.

The operands are chosen so that Y = A X is EXACT in fp32 whatever the summation order: the values of A are multiples of
0.5 out of {0.5, 1, -1, 2, -0.5, 1.5}, X holds integers in [-3, 3] (bf16-exact), so every product and every partial sum is a
multiple of 0.5 whose magnitude is at most the row's sum of |terms|; while twice that sum stays below 2^24 all of them are
fp32 numbers, every fma is exact, and sequential sums, even / odd half sums, LDS-first / gather-second sums and 4 x 64-strided
segment sums all give the same bits.  For bf16 storage the expected value is that exact number rounded once to nearest even
(f32_to_bf16 of csrc/common.h = torch's float32 -> bfloat16 cast).
"""
import numpy as np
import torch

LONG_ROW = 1024          # = sgformer_amd.kernels.LONG_ROW (asserted by the host test)
SEGMENT = 1024           # = sgf_spmm_segment_len()
EXACT = 2 ** 24

# the row lengths every part of the ladder holds: every length up to 2 * 16 + 2 (a 16-entry group, its double-buffer switch at
# 2 G and the < G tail, for G = 8 and 16, at both parities), then the 64-entry piece of the row-block kernels, the unrolled
# batches, LONG_ROW from both sides, and long rows of 2, 3 and 4 segments with full and 1-entry last segments
B = list(range(35)) + [47, 48, 49, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3077]
VALUES = (0.5, 1.0, -1.0, 2.0, -0.5, 1.5)


def _fill(lens, n_cols, seed):
    """The CSR of rows with these lengths: random columns with every 7th stored entry forced to n_cols - 1 and every 11th to
    0 (a short buffer bound or a wrong row pitch then shows in the result), sorted inside each row, duplicates kept."""
    lens = np.asarray(lens, dtype=np.int64)
    rowptr = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    nnz = int(rowptr[-1])
    rng = np.random.RandomState(seed)
    col = rng.randint(0, n_cols, size=nnz).astype(np.int64)
    e = np.arange(nnz)
    col[e % 7 == 6] = n_cols - 1
    col[e % 11 == 10] = 0
    rows = np.repeat(np.arange(lens.size), lens)
    col = col[np.lexsort((col, rows))]                       # by row, then by column: rows keep their places
    val = np.asarray(VALUES, dtype=np.float32)[rng.randint(0, len(VALUES), size=nnz)]
    return (torch.from_numpy(lens), torch.from_numpy(rowptr), torch.from_numpy(col.astype(np.int32)),
            torch.from_numpy(val))


def ladder_lens(seed):
    rng = np.random.RandomState(seed + 1000)
    shuffled = [B[i] for i in rng.permutation(len(B))]
    lens = [0, 0, 0, 0] + B + [0, 0] + B[::-1] + [0] + shuffled + [0, 0, 0]
    while len(lens) % 4 != 3:
        lens.append(1)
    return lens


def ladder(n_cols, seed):
    """(lens, rowptr, colind, val): 175 rows, 43 131 stored entries.  Every length of B at three stream offsets and wave
    parities, rows 0-3 (one 4-row wave) empty, the last 4-row wave ragged."""
    return _fill(ladder_lens(seed), n_cols, seed)


def cyclic(n_rows, period, n_cols, seed):
    """The same kind of CSR with row lengths (7 i) mod period: the large-n cases."""
    return _fill((7 * np.arange(n_rows, dtype=np.int64)) % period, n_cols, seed)


def long_segments(lens):
    """The `long_segments` argument of sgf_spmm_split for these rows, exactly."""
    lens = torch.as_tensor(lens)
    return int(((lens[lens > LONG_ROW] + SEGMENT - 1) // SEGMENT).sum())


def operand(n_cols, d, seed):
    """X: int64 [n_cols, d], integers in [-3, 3]."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, (n_cols, d), generator=g, dtype=torch.int64)


def reference(rowptr, colind, val, x, budget_bytes=64 << 20):
    """(Y, worst): Y = A X exactly, as float64 [n_rows, d], computed in int64 on 2 val and x and halved; worst = the largest
    sum of |terms| over the outputs.  Rows are taken in chunks so that no temporary exceeds about `budget_bytes`."""
    n, d = rowptr.numel() - 1, x.shape[1]
    v2 = (2.0 * val.double()).round().to(torch.int64)
    assert torch.equal(v2.double(), 2.0 * val.double()), "values must be multiples of 0.5"
    col = colind.to(torch.int64)
    out = torch.zeros((n, d), dtype=torch.int64)
    worst = 0
    per_chunk = max(budget_bytes // (8 * max(d, 1)), 1)
    rp = rowptr.numpy()
    r0 = 0
    while r0 < n:
        r1 = int(np.searchsorted(rp, rp[r0] + per_chunk, side="right")) - 1
        r1 = min(max(r1, r0 + 1), n)
        e0, e1 = int(rp[r0]), int(rp[r1])
        if e1 > e0:
            terms = v2[e0:e1, None] * x[col[e0:e1]]
            rows = torch.repeat_interleave(torch.arange(r1 - r0), rowptr[r0 + 1:r1 + 1] - rowptr[r0:r1])
            out[r0:r1].index_add_(0, rows, terms)
            worst = max(worst, int(torch.zeros((r1 - r0, d), dtype=torch.int64).index_add_(0, rows, terms.abs()).max()))
        r0 = r1
    return out.double() / 2.0, worst / 2.0


def expected(ref, dtype):
    """What a kernel must store: the exact result as fp32 (no rounding while 2 * worst < 2^24), rounded once for bf16."""
    y = ref.to(torch.float32)
    assert torch.equal(y.double(), ref)
    return y if dtype == torch.float32 else y.to(torch.bfloat16)
