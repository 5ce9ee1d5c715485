"""The forward GCN SpMM on zero-elided operand rows (csrc/spmm.hip: k_spmm_row_packed; csrc/fused.hip:
k_bn_apply_bf16x8_packed), bit for bit against the dense kernels: sgf_spmm_packed == sgf_spmm on the same operand for both slot
sizes, with the slots from the numpy encoder (tests/packed_rows.py) and from the producer; one overflowing row sends the whole
launch to the dense rows; sgf_bn_apply_packed writes sgf_bn_apply's output, slots that decode to it, and the exact count of
overflowing rows.  (large/ours.py:34 on the operand of :77-80 / :87-93.)"""
import numpy as np
import pytest
import torch

from tests import packed_rows as P

pytestmark = pytest.mark.gpu

N = 3001                                    # not a multiple of the producer's 32-row block pass nor of the 4-row SpMM block
DEGREES = (0, 1, 7, 8, 9, 16, 17, 65)       # around the 8-entry batches of the row kernel and its 4 / 2 / 1 tail


@pytest.fixture(scope="module")
def csr(cuda):
    """Rows of every degree in DEGREES in turn; sources ascending inside a row, with a duplicate source in every row of
    two or more entries, a self loop in every row, and the crafted operand rows 0-5 among the sources of every long row."""
    rng = np.random.default_rng(5)
    rowptr, colind = [0], []
    for i in range(N):
        k = DEGREES[i % len(DEGREES)]
        c = rng.integers(0, N, size=k)
        if k >= 1:
            c[0] = i                                            # self loop
        if k >= 2:
            c[1] = c[-1]                                        # duplicate source
        if k >= 16:
            c[2:8] = np.arange(6)                               # the crafted operand rows
        colind.extend(np.sort(c).tolist())
        rowptr.append(len(colind))
    val = rng.uniform(0.01, 1.0, size=len(colind)).astype(np.float32)
    return (torch.tensor(rowptr, dtype=torch.int64, device=cuda), torch.tensor(colind, dtype=torch.int32, device=cuda),
            torch.from_numpy(val).to(cuda))


def _bf16(rows_u16: np.ndarray, cuda) -> torch.Tensor:
    return torch.from_numpy(rows_u16.view(np.int16).copy()).to(cuda).view(torch.bfloat16)


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _packed_from_numpy(rows_u16, slot_bytes, cuda):
    from sgformer_amd import _lib
    from sgformer_amd.kernels import PackedRows
    slots, over = P.encode(rows_u16, slot_bytes)
    n = rows_u16.shape[0]
    buf = torch.zeros(_lib.load().sgf_spmm_packed_bytes(n, slot_bytes), dtype=torch.uint8, device=cuda)
    buf[:n * slot_bytes] = torch.from_numpy(slots.reshape(-1)).to(cuda)
    return PackedRows(buf, slot_bytes, n, torch.tensor([over], dtype=torch.int32, device=cuda)), over


@pytest.mark.parametrize("slot_bytes", [384, 448])
@pytest.mark.parametrize("overflow_row", [False, True])
def test_spmm_packed_equals_spmm(cuda, csr, slot_bytes, overflow_row):
    from sgformer_amd import ops
    K = ops.K
    rowptr, colind, val = csr
    rows = P.crafted_rows(slot_bytes, N, seed=11, overflow_row=overflow_row)
    x = _bf16(rows, cuda)
    assert K.spmm_packed_supported(x.shape, x.dtype, slot_bytes)
    packed, over = _packed_from_numpy(rows, slot_bytes, cuda)
    assert over == int(overflow_row)
    want = K.spmm(rowptr, colind, val, x, N)
    got = K.spmm_packed(rowptr, colind, val, x, packed, N)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    if not overflow_row:
        # the launch really gathered the slots: with the dense operand poisoned it still gives the same rows, and with
        # the overflow count raised it reads the (poisoned) dense rows instead
        poison = torch.full_like(x, 3.0)
        assert torch.equal(K.spmm_packed(rowptr, colind, val, poison, packed, N).view(torch.int16), want.view(torch.int16))
        packed.overflow.fill_(1)
        assert torch.equal(K.spmm_packed(rowptr, colind, val, poison, packed, N).view(torch.int16),
                           K.spmm(rowptr, colind, val, poison, N).view(torch.int16))


@pytest.mark.parametrize("slot_bytes", [384, 448])
def test_long_rows_take_the_queue(cuda, slot_bytes):
    """A launch with a long-row queue gathers the slots for its short rows; the queued row (1500 entries > 1024) is reduced
    from the dense operand by the long-row kernels, as in sgf_spmm_split."""
    from sgformer_amd import ops
    K = ops.K
    rng = np.random.default_rng(9)
    lens = [9, 1500, 17, 0, 65] + [8] * 60
    colind = np.concatenate([np.sort(rng.integers(0, N, size=k)) for k in lens]).astype(np.int32)
    rowptr = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device=cuda)
    val = torch.from_numpy(rng.uniform(0.01, 1.0, size=colind.size).astype(np.float32)).to(cuda)
    colind = torch.from_numpy(colind).to(cuda)
    segs = ops.long_row_segments(rowptr)
    assert segs == 2
    rows = P.crafted_rows(slot_bytes, N, seed=13)
    x = _bf16(rows, cuda)
    packed, over = _packed_from_numpy(rows, slot_bytes, cuda)
    assert over == 0
    want = K.spmm(rowptr, colind, val, x, len(lens), long_segments=segs)
    got = K.spmm_packed(rowptr, colind, val, x, packed, len(lens), long_segments=segs)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def _bn_inputs(cuda, n, seed, scale):
    g = torch.Generator(device=cuda).manual_seed(seed)
    z = (torch.randn(n, 256, device=cuda, generator=g) * 1.5).to(torch.bfloat16)
    res = torch.relu(torch.randn(n, 256, device=cuda, generator=g)).to(torch.bfloat16)
    mean = torch.randn(256, device=cuda, generator=g) * 0.2 + scale
    rstd = torch.rand(256, device=cuda, generator=g) + 0.5
    gamma = torch.rand(256, device=cuda, generator=g) + 0.5
    beta = torch.randn(256, device=cuda, generator=g) * 0.1
    return z, res, mean, rstd, gamma, beta


@pytest.mark.parametrize("slot_bytes", [384, 448])
@pytest.mark.parametrize("use_res,relu", [(False, True), (True, True), (False, False)])
@pytest.mark.parametrize("n", [1, 3001])
def test_bn_apply_packed(cuda, slot_bytes, use_res, relu, n):
    """relu without residual: about half of every row is zero and no row overflows; with the residual about a quarter is
    (rows overflow a 384-byte slot, most fit 448); without relu nothing is zero and every row overflows."""
    from sgformer_amd import ops
    K = ops.K
    z, res, mean, rstd, gamma, beta = _bn_inputs(cuda, n, 17 + n, 0.0)
    if not relu:
        z[0, 5] = -1e-30                    # -> -1e-30 * 1e-12: below half of bf16's smallest subnormal, rounds to -0.0
        rstd[5], gamma[5], beta[5], mean[5] = 1e-12, 1.0, 0.0, 0.0
    r = res if use_res else None
    want = K.bn_apply(z, mean, rstd, gamma, beta, r, relu)
    got, packed = K.bn_apply_packed(z, mean, rstd, gamma, beta, r, relu, slot_bytes)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    rows = _bits(want)
    if not relu:
        assert rows[0, 5] == 0x8000
    nz = (rows != 0).sum(1)
    fits = nz <= P.capacity(slot_bytes)
    assert int(packed.overflow.item()) == int((~fits).sum())
    if relu and not use_res:
        assert fits.all()
    if not relu:
        assert not fits[1:].any()
    slots = packed.slots[:n * slot_bytes].cpu().numpy().reshape(n, slot_bytes)
    assert np.array_equal(P.counts(slots), nz)
    assert np.array_equal(P.decode(slots)[fits], rows[fits])
    ref_slots, _ = P.encode(rows, slot_bytes)
    assert np.array_equal(slots, ref_slots)                      # truncated rows and the zero tails included


@pytest.mark.parametrize("slot_bytes", [384, 448])
def test_producer_feeds_consumer(cuda, csr, slot_bytes):
    """The chain of the model: BatchNorm + relu writes the operand and its packed copy, the SpMM gathers the copy."""
    from sgformer_amd import ops
    K = ops.K
    rowptr, colind, val = csr
    z, _, mean, rstd, gamma, beta = _bn_inputs(cuda, N, 23, 0.0)
    x, packed = K.bn_apply_packed(z, mean, rstd, gamma, beta, None, True, slot_bytes)
    assert int(packed.overflow.item()) == 0
    want = K.spmm(rowptr, colind, val, x, N)
    before = ops._kernels.counters["spmm_packed"]
    got = K.spmm_packed(rowptr, colind, val, torch.full_like(x, 3.0), packed, N)     # (dense operand poisoned)
    assert ops._kernels.counters["spmm_packed"] == before + 1
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
