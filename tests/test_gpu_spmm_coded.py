"""The SpMM on 12-bit coded operand rows (csrc/spmm.hip: k_spmm_row_coded; csrc/spmm_coded.hip: k_code_rows, k_code_values),
bit for bit against the dense kernel: sgf_spmm_coded == sgf_spmm on a row-length ladder with a long row, for Gaussian,
row-scaled and relu + relu operands, with escaped rows planted among the sources (mixed batches), with every row escaped, with
a negative stored value (whole launch falls back) and with stored zeros; the two preparation kernels against the numpy codec
of tests/coded_rows.py byte for byte.  Apart from the all-escape and negative-value cases at most 15 % of the source rows are
escaped (asserted from the device count), so parity is not proved on the dense path alone."""
import numpy as np
import pytest
import torch

from tests import coded_rows as C

pytestmark = pytest.mark.gpu

N = 6000
LONG = (37, 1500)                           # one row longer than LONG_ROW = sgf_spmm_segment_len() = 1024: two segments
OPERANDS = {"gaussian": C.gaussian, "scaled": C.gaussian_scaled, "relu_relu": C.relu_relu,
            "scaled12": lambda n, seed: C.gaussian_scaled(n, seed, span=12)}
# The largest share of the stored entries that may carry the escape tag (and so read the dense row) in a parity case.  An entry
# is tagged when its source row escaped or when val * 2^(E - 15) is not a normal float.  Escaped sources: at most 15 % of the
# rows (asserted), met uniformly by the random sources, plus rows 0 and n - 1, which the ladder forces into every row of 16
# or more entries (2 of at least 16: under 5 % of all entries): 0.15 + 0.05 = 0.20.  Overflow: val in [0.01, 1) has an
# exponent field of 120-126, so val * 2^(E - 15) leaves the floats when E >= 143-149, a row maximum of 2^16-2^22: never for
# unit Gaussians and relu sums (E = 127-130) nor for scales up to 2^12 (E <= 142); for scales drawn from 2^-30 .. 2^30 it takes
# the rows scaled by 2^14 or more at the most, 17 of 61 = 0.28 of them — that case proves the tag rule, "scaled12" the coded
# path under a row scale.
TAGGED_CAP = {"gaussian": 0.20, "relu_relu": 0.20, "scaled12": 0.20, "scaled": 0.20 + 0.28}


def _bf16(rows_u16: np.ndarray, cuda) -> torch.Tensor:
    return torch.from_numpy(rows_u16.view(np.int16).copy()).to(cuda).view(torch.bfloat16)


def _planted(n):
    return sorted({0, n - 1} | set(range(5, n, 10)))


@pytest.fixture(scope="module")
def csr(cuda):
    from sgformer_amd import kernels, ops
    assert kernels.LONG_ROW == 1024 < LONG[1]
    lens, rowptr, colind, val = C.ladder_csr(N, seed=5, long_row=LONG)
    assert set(C.LENGTHS) <= set(lens) and max(lens) == LONG[1]
    rowptr, colind, val = rowptr.to(cuda), colind.to(cuda), val.to(cuda)
    segs = ops.long_row_segments(rowptr)
    assert segs == 2
    return rowptr, colind, val, segs


def _coded(K, csr, x, val=None):
    """(y of sgf_spmm_coded, escaped rows, unsupported values) with everything prepared on the device."""
    rowptr, colind, v, segs = csr
    v = v if val is None else val
    slots, scale, n_escaped = K.spmm_code_rows(x)
    vc, n_unsupported = K.spmm_code_values(colind, v, scale)
    y = K.spmm_coded(rowptr, colind, v, vc, x, slots, n_unsupported, N, long_segments=segs)
    _coded.tagged_share = float((vc[:v.numel()].view(torch.int32) < 0).float().mean())
    return y, int(n_escaped.item()), int(n_unsupported.item())


def _same(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("planted", [False, True])
@pytest.mark.parametrize("operand", sorted(OPERANDS))
def test_spmm_coded_equals_spmm(cuda, csr, operand, planted):
    from sgformer_amd import kernels, ops
    K = ops.K
    rowptr, colind, val, segs = csr
    rows = OPERANDS[operand](N, seed=11)
    if planted:
        rows = C.plant_escapes(rows, _planted(N))
    x = _bf16(rows, cuda)
    assert K.spmm_coded_supported(x.shape, x.dtype)
    want = K.spmm(rowptr, colind, val, x, N, long_segments=segs)
    before = kernels.counters["spmm_coded"]
    got, escaped, unsupported = _coded(K, csr, x)
    assert kernels.counters["spmm_coded"] == before + 1
    assert unsupported == 0
    assert escaped == C.encode(rows)[2] and escaped <= 0.15 * N
    assert escaped >= (len(_planted(N)) if planted else 0)
    print(f"{operand} planted={planted}: escaped rows {escaped / N:.4f}, tagged entries {_coded.tagged_share:.4f}")
    assert _coded.tagged_share <= TAGGED_CAP[operand]
    assert _same(got, want)


def test_the_launch_gathers_the_slots(cuda):
    """With the dense rows of every coded source poisoned the result is unchanged (no long row here: those are reduced from
    the dense operand); with the unsupported count raised the launch reads the (poisoned) dense rows and original values."""
    from sgformer_amd import ops
    K = ops.K
    _, rowptr, colind, val = C.ladder_csr(N, seed=6)
    rowptr, colind, val = rowptr.to(cuda), colind.to(cuda), val.to(cuda)
    rows = C.plant_escapes(C.gaussian(N, seed=12), _planted(N))
    x = _bf16(rows, cuda)
    want = K.spmm(rowptr, colind, val, x, N)
    slots, scale, n_escaped = K.spmm_code_rows(x)
    vc, n_unsupported = K.spmm_code_values(colind, val, scale)
    assert 0 < int(n_escaped.item()) <= 0.15 * N
    poison = x.clone()
    poison[(scale != C.ESCAPED)] = 3.0
    assert _same(K.spmm_coded(rowptr, colind, val, vc, poison, slots, n_unsupported, N), want)
    n_unsupported.fill_(1)
    assert _same(K.spmm_coded(rowptr, colind, val, vc, poison, slots, n_unsupported, N), K.spmm(rowptr, colind, val, poison, N))


def test_every_row_escapes(cuda, csr):
    from sgformer_amd import ops
    K = ops.K
    rowptr, colind, val, segs = csr
    rows = C.gaussian(N, seed=13)
    rows[np.arange(N), np.arange(N) % C.D] = 0x0001               # a subnormal in every row
    x = _bf16(rows, cuda)
    got, escaped, unsupported = _coded(K, csr, x)
    assert escaped == N and unsupported == 0
    assert _same(got, K.spmm(rowptr, colind, val, x, N, long_segments=segs))


def test_negative_stored_value_falls_back(cuda, csr):
    from sgformer_amd import ops
    K = ops.K
    rowptr, colind, val, segs = csr
    val = val.clone()
    val[123] = -0.5
    x = _bf16(C.relu_relu(N, seed=14), cuda)
    got, escaped, unsupported = _coded(K, csr, x, val)
    assert unsupported == 1
    assert _same(got, K.spmm(rowptr, colind, val, x, N, long_segments=segs))


def test_negative_zero_stored_value_falls_back(cuda, csr):
    """-0.0 has the tag's bit set already: it counts as unsupported, and the launch reads the dense rows — a NaN in the source
    row reaches y as it does through sgf_spmm (0 x NaN), where the zeroed slot of the escaped row would have given 0."""
    from sgformer_amd import ops
    K = ops.K
    rowptr, colind, val, segs = csr
    val = val.clone()
    e = int(rowptr[9])                                            # first entry of row 9 (16 entries)
    val[e] = -0.0
    rows = C.gaussian(N, seed=16)
    rows[int(colind[e]), 3] = 0x7FC0                              # NaN in its source row
    x = _bf16(rows, cuda)
    got, escaped, unsupported = _coded(K, csr, x, val)
    assert unsupported == 1 and escaped >= 1
    want = K.spmm(rowptr, colind, val, x, N, long_segments=segs)
    assert bool(torch.isnan(want[9, 3])) and _same(got, want)


def test_stored_zeros(cuda, csr):
    from sgformer_amd import ops
    K = ops.K
    rowptr, colind, val, segs = csr
    val = val.clone()
    val[::7] = 0.0
    x = _bf16(C.gaussian(N, seed=15), cuda)
    got, escaped, unsupported = _coded(K, csr, x, val)
    assert unsupported == 0 and escaped <= 0.15 * N
    assert _same(got, K.spmm(rowptr, colind, val, x, N, long_segments=segs))


@pytest.mark.parametrize("n", [1, 17, N + 1])               # one row, one row past a 16-row block, a ragged last wave
def test_code_rows_against_the_cpu_encoder(cuda, n):
    from sgformer_amd import ops
    rows = np.concatenate([C.gaussian(n, 21), C.gaussian_scaled(n, 22), C.relu_relu(n, 23)])[np.random.default_rng(1).permutation(3 * n)[:n]]
    rows = C.plant_escapes(rows, range(0, n, 9))
    if n > 40:
        rows[3] = 0
        rows[4] = 0x8000
        rows[6] = 0x0080                                          # E = 1
        rows[7] = 0x7F7F                                          # E = 254
    slots, scale, n_escaped = ops.K.spmm_code_rows(_bf16(rows, cuda))
    want_slots, want_scale, want_escaped = C.encode(rows)
    assert int(n_escaped.item()) == want_escaped > 0
    assert np.array_equal(scale.cpu().numpy()[:n], want_scale)
    assert slots.numel() == n * C.SLOT
    assert np.array_equal(slots.cpu().numpy().reshape(n, C.SLOT), want_slots)


@pytest.mark.parametrize("nnz", [1, 3, 1023, 1025, 40001])    # under one thread's four, around a 1024-entry block, many blocks
def test_code_values_against_the_cpu_restatement(cuda, nnz):
    from sgformer_amd import ops
    rng = np.random.default_rng(nnz)
    scale = rng.integers(1, 255, size=N).astype(np.uint8)
    scale[::5] = C.ESCAPED
    scale[1::5] = 128
    colind = rng.integers(0, N, size=nnz).astype(np.int32)
    val = rng.uniform(0.01, 1.0, size=nnz).astype(np.float32)
    val[::11] = 0.0
    val[5::13] = np.float32(2.0 ** -120)
    val[6::17] = np.float32(2.0 ** 100)
    if nnz > 100:
        val[[7, 70]] = -0.25
        val[80] = -0.0                                            # counted: the sign bit is set
    vc, n_unsupported = ops.K.spmm_code_values(torch.from_numpy(colind).to(cuda), torch.from_numpy(val).to(cuda),
                                               torch.from_numpy(scale).to(cuda))
    want, want_neg = C.code_values(colind, val, scale)
    assert int(n_unsupported.item()) == want_neg
    assert np.array_equal(vc.cpu().numpy()[:nnz].view(np.uint32), want.view(np.uint32))
