"""The evaluation metrics on the MI355X: sgf_rocauc_counts / sgf_argmax_count (csrc/metrics.hip, include/sgf.h block N5)
through the kernel table against the numpy table of tests/cpu_kernels_metrics.py — INTEGER equality, the contract is exact —
and sgformer_amd.metrics' drop-ins against the values the live reference returned (tests/golden/metrics/metrics_eval.npz), 1e-12
absolute (exact counts, one float64 division per column, a sum of a few terms in [0, 1]).

The one-column softmax form: the device's softmax may differ from the CPU's by an ulp, which can make or break ties, so
that case is asserted against the numpy table fed with the device's own softmax column; its difference to the recorded
value (reference, CPU softmax) is printed here and written into profiles/metrics_probe.md by scripts/metrics_probe.py,
not asserted."""
import os

import numpy as np
import pytest
import torch

from tests.cpu_kernels_metrics import CpuKernelsMetrics

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "metrics", "metrics_eval.npz")
TOL = 1e-12


def _scores(n, c, seed, quantum=None, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, generator=g) * 3
    if quantum:
        x = torch.round(x / quantum) * quantum
    flat = x.view(-1)
    flat[::97], flat[1::97] = 0.0, -0.0
    flat[5::211], flat[6::211] = float("inf"), float("-inf")
    return x.to(dtype)


def _labels(n, c, seed, kind):
    g = torch.Generator().manual_seed(seed + 1000)
    t = (torch.rand(n, c, generator=g) < 0.3).long()
    if kind == "i64":
        return t
    t = t.float()
    t[torch.rand(n, c, generator=g) < 0.1] = float("nan")
    return t


def _idx(n, m, how, seed):
    if how == "dense":
        assert m == n
        return None
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:m]
    return perm if how == "permuted" else perm.sort().values


def _auc_counts(cuda, logits, target, idx):
    from sgformer_amd import ops
    got = ops.K.rocauc_counts(logits.to(cuda), target.to(cuda), None if idx is None else idx.to(cuda))
    torch.cuda.synchronize()
    return got.cpu()


CASES = [
    # n, m, c, label kind, dtype, quantum, idx form
    (30000, 20000, 112, "i64", torch.float32, None, "permuted"),
    (30000, 20000, 112, "f32", torch.float32, None, "indexed"),
    (9000, 9000, 112, "f32", torch.bfloat16, None, "dense"),
    (1000003, 1000003, 1, "i64", torch.float32, None, "dense"),       # one column across ~490 blocks
    (1200000, 1000003, 1, "f32", torch.float32, 0.5, "permuted"),     # ~20 score values: tie groups of ~50 000 rows
    (50000, 50000, 3, "i64", torch.float32, 4.0, "dense"),            # tie groups longer than a block's 2048-key chunk
    (4100, 4100, 7, "i64", torch.bfloat16, 1.0, "dense"),
    (1, 1, 1, "i64", torch.float32, None, "dense"),
    (1, 1, 5, "f32", torch.float32, None, "dense"),
    (2049, 2048, 2, "i64", torch.float32, None, "indexed"),
]


@pytest.mark.parametrize("n,m,c,kind,dtype,quantum,how", CASES)
def test_rocauc_counts_equal_the_numpy_table(cuda, n, m, c, kind, dtype, quantum, how):
    logits, target, idx = _scores(n, c, n + c, quantum, dtype), _labels(n, c, n + c, kind), _idx(n, m, how, m)
    got = _auc_counts(cuda, logits, target, idx)
    want = CpuKernelsMetrics.rocauc_counts(logits, target, idx)
    assert got.dtype == torch.int64 and got.shape == (c, 6)
    bad = (got != want).any(dim=1).nonzero().view(-1).tolist()
    print(f"n={n} m={m} c={c} {kind} {dtype} q={quantum} {how}: {len(bad)} of {c} columns differ; column 0 {got[0].tolist()}")
    assert torch.equal(got, want), (bad[:5], got[bad[:2]].tolist(), want[bad[:2]].tolist())


def test_all_scores_equal_and_other_and_nan(cuda):
    n, c = 5000, 4
    logits = torch.full((n, c), 1.5)
    target = _labels(n, c, 3, "f32")
    target[::50, 1] = 0.5
    logits[7::40, 2] = float("nan")
    got = _auc_counts(cuda, logits, target, None)
    assert torch.equal(got, CpuKernelsMetrics.rocauc_counts(logits, target, None))
    p, nn, u2 = got[0, :3].tolist()
    assert u2 == p * nn and u2 / (2 * p * nn) == 0.5
    assert int(got[1, 3]) > 0 and int(got[2, 4]) > 0 and int(got[:, 5].min()) > 0


def test_strided_logits_view(cuda):
    n, c = 6000, 24
    wide = _scores(n, 40, 5).to(cuda)
    view = wide[:, 8:8 + c]                                   # ldl = 40 > c, rows start off the 16-byte grid
    target = _labels(n, c, 5, "i64")
    idx = _idx(n, 3500, "permuted", 9)
    from sgformer_amd import ops
    got = ops.K.rocauc_counts(view, target.to(cuda), idx.to(cuda)).cpu()
    assert torch.equal(got, CpuKernelsMetrics.rocauc_counts(view.cpu(), target, idx))
    labels = torch.randint(0, c, (n, 1))
    got = ops.K.argmax_count(view, labels.to(cuda), idx.to(cuda)).cpu()
    assert torch.equal(got, CpuKernelsMetrics.argmax_count(view.cpu(), labels, idx))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n,c,m,kind", [(200000, 47, 120000, "i64"), (50000, 2, 50000, "f32"), (30000, 112, 9000, "i64"),
                                         (3000, 1, 3000, "i64"), (5000, 5, 1, "f32"), (7000, 200, 4000, "f32")])
def test_argmax_count_matches_torch_argmax_on_the_cpu(cuda, n, c, m, kind, dtype):
    """First-index ties, NaN rows (a NaN is the maximum, the first NaN wins), -0.0 / +0.0, strided [N, 1] labels."""
    from sgformer_amd import ops
    g = torch.Generator().manual_seed(n + c)
    logits = torch.randn(n, c, generator=g)
    if c > 1:
        logits[::3, 0] = logits[::3, c - 1] = 9.0              # the maximum twice: the first index wins
        logits[1::7, c // 2] = float("nan")
        logits[1::14, c - 1] = float("nan")
        logits[2::11] = -0.0
        logits[2::11, c - 1] = 0.0                             # -0.0 == +0.0: column 0 wins
        logits[4::13] = float("-inf")
    logits = logits.to(dtype)
    labels = torch.randint(0, c, (n, 1), generator=g)
    pair = torch.stack([labels, labels + 1], dim=2)           # [n, 1, 2]: its [:, :, 0] is an [n, 1] view with row stride 2
    if kind == "f32":
        pair = pair.float()
        pair[::9] = float("nan")
    both, both_dev = pair[:, :, 0], pair.to(cuda)[:, :, 0]
    assert both_dev.stride(0) == 2
    idx = None if m == n else _idx(n, m, "permuted", m)
    got = ops.K.argmax_count(logits.to(cuda), both_dev, None if idx is None else idx.to(cuda))
    torch.cuda.synchronize()
    want = CpuKernelsMetrics.argmax_count(logits, both, idx)
    rows = torch.arange(n) if idx is None else idx
    pred = torch.argmax(logits.float()[rows], dim=-1)          # (the table's own prediction IS torch.argmax on the CPU copy)
    y = both[rows, 0]
    lab = ~torch.isnan(y) if kind == "f32" else torch.ones_like(y, dtype=torch.bool)
    assert want.tolist() == [int(lab.sum()), int((y[lab] == pred[lab]).sum())]
    print(f"n={n} c={c} m={m} {kind} {dtype}: got {got.tolist()} want {want.tolist()}")
    assert torch.equal(got.cpu(), want)


def test_two_runs_give_identical_bytes(cuda):
    from sgformer_amd import ops
    logits, target = _scores(40000, 16, 21, 0.25).to(cuda), _labels(40000, 16, 21, "f32").to(cuda)
    idx = _idx(40000, 33000, "permuted", 4).to(cuda)
    labels = torch.randint(0, 16, (40000,), device=cuda)
    a = [ops.K.rocauc_counts(logits, target, idx).cpu().numpy().tobytes() for _ in range(2)]
    b = [ops.K.argmax_count(logits, labels, idx).cpu().numpy().tobytes() for _ in range(2)]
    assert a[0] == a[1] and b[0] == b[1]


def test_side_stream(cuda):
    """Inputs produced on a side stream just before the call on that stream: same counts (no hidden default-stream use)."""
    from sgformer_amd import ops
    base, target = _scores(60000, 20, 31), _labels(60000, 20, 31, "i64")
    labels = torch.randint(0, 20, (60000,))
    want_auc = CpuKernelsMetrics.rocauc_counts(base * 2 + 1, target, None)
    want_arg = CpuKernelsMetrics.argmax_count(base * 2 + 1, labels, None)
    bd, td, ld = base.to(cuda), target.to(cuda), labels.to(cuda)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        x = bd * 2 + 1
        t = td.clone()
        auc = ops.K.rocauc_counts(x, t, None)
        arg = ops.K.argmax_count(x, ld.clone(), None)
    side.synchronize()
    assert torch.equal(auc.cpu(), want_auc) and torch.equal(arg.cpu(), want_arg)


def test_invalid_arguments_are_rejected_on_the_host(cuda):
    from sgformer_amd import ops
    x, t = torch.zeros(8, 3, device=cuda), torch.zeros(8, 3, dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError):
        ops.K.rocauc_counts(x, t[:, :2], None)
    with pytest.raises(ValueError):
        ops.K.rocauc_counts(x, t.int(), None)
    with pytest.raises(ValueError):
        ops.K.rocauc_counts(x, t, torch.zeros(2, dtype=torch.int32, device=cuda))
    with pytest.raises(ValueError):
        ops.K.argmax_count(x, t, None)
    with pytest.raises(TypeError):
        ops.K.argmax_count(x.double(), t[:, :1], None)
    with pytest.raises(RuntimeError):
        ops.rocauc_counts(x.cpu(), t.cpu())


@pytest.mark.parametrize("where", ["device", "host"])
def test_drop_ins_equal_the_recorded_reference_values(cuda, where):
    from sgformer_amd import metrics
    z = np.load(GOLDEN)
    fn = {"rocauc": metrics.eval_rocauc, "acc": metrics.eval_acc, "f1": metrics.eval_f1}
    lines = []
    for name in sorted({k.split(".")[0] for k in z.files}):
        kind = str(z[f"{name}.kind"])
        y_true, y_pred = torch.from_numpy(z[f"{name}.y_true"]), torch.from_numpy(z[f"{name}.y_pred"])
        if where == "device":
            y_true, y_pred = y_true.to(cuda), y_pred.to(cuda)
        got = fn[kind](y_true, y_pred)
        want = float(z[f"{name}.value"])
        assert isinstance(got, float)
        if kind == "rocauc" and y_true.shape[1] == 1:
            col = torch.softmax(y_pred.to(cuda), dim=-1)[:, 1:2].cpu()          # the device's own softmax column
            counts = CpuKernelsMetrics.rocauc_counts(col, y_true.cpu(), None)
            own = metrics.auc_from_counts(counts)[0]
            own = sum(own) / len(own)
            lines.append(f"{name} [{where}]: got {got!r}, numpy table on the device softmax {own!r} (|d|={abs(got - own):.2e}), "
                         f"recorded with the CPU softmax {want!r} (|d|={abs(got - want):.2e}, not asserted)")
            print(lines[-1])
            assert abs(got - own) <= TOL
            continue
        print(f"{name} [{where}]: got {got!r} recorded {want!r} |d|={abs(got - want):.2e}")
        assert abs(got - want) <= TOL


def test_rows_surface_on_the_device(cuda):
    """rocauc_rows / accuracy_rows / f1_micro_rows with int64 rows, a bool mask and None; a host label with device logits."""
    from sgformer_amd import metrics, ops
    from tests.test_metrics_host import midrank_mean
    n, c = 20000, 10
    out, label = _scores(n, c, 41, 0.25), _labels(n, c, 41, "f32")
    out[torch.isinf(out)] = 1.0
    perm = _idx(n, 12000, "permuted", 6)
    mask = torch.zeros(n, dtype=torch.bool).index_fill_(0, perm, True)
    for idx, rows in ((perm, perm), (mask, mask.nonzero().view(-1)), (None, torch.arange(n))):
        got = metrics.rocauc_rows(out.to(cuda), label, None if idx is None else idx.to(cuda))
        assert abs(got - midrank_mean(out[rows], label[rows])) <= TOL
    y = torch.randint(0, c, (n, 1))
    hits = (out.argmax(-1)[perm] == y[perm, 0]).sum().item()
    assert metrics.accuracy_rows(out.to(cuda), y.to(cuda), perm.to(cuda)) == hits / 12000
    assert metrics.f1_micro_rows(out.to(cuda), y.to(cuda), mask.to(cuda)) == hits / 12000
    assert ops.K.name == "hip"
