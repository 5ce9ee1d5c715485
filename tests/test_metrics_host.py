"""The evaluation metrics (include/sgf.h block N5) above the C ABI, on the CPU: sgformer_amd.metrics driven by the numpy
kernel table of tests/cpu_kernels_metrics.py, and launch.patch_eval_metrics on a fake data_utils module.

References: (1) a mid-rank restatement of the AUC in numpy float64 (scipy-free: average 1-based rank of each tie group,
U = sum of the positives' ranks - P (P + 1) / 2, AUC = U / (P Nn)); (2) scikit-learn's roc_auc_score / f1_score and the
numpy accuracy loop; (3) the values the live reference returned, stored in tests/golden/metrics/metrics_eval.npz by
scripts/make_metrics_golden.py.  Bound 1e-12 absolute: the counts are exact integers, what remains is one float64 division
per column and a sum of at most a few hundred terms in [0, 1] (each rounding <= 2^-53 relative)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "metrics", "metrics_eval.npz")
TOL = 1e-12


@pytest.fixture
def cpu_table():
    from sgformer_amd import ops
    from tests.cpu_kernels_metrics import CpuKernelsMetrics
    prev = ops.set_kernels(CpuKernelsMetrics())
    yield
    ops.set_kernels(prev)


def midrank_auc(score, label):
    """float64 AUC of one column from average ranks; rows whose label is NaN are dropped."""
    score, label = np.asarray(score, dtype=np.float64), np.asarray(label, dtype=np.float64)
    keep = ~np.isnan(label)
    score, label = score[keep], label[keep]
    order = np.argsort(score, kind="stable")
    s = score[order]
    starts = np.flatnonzero(np.concatenate(([True], s[1:] != s[:-1])))
    ends = np.concatenate((starts[1:], [s.size]))
    rank_sorted = np.repeat((starts + 1 + ends) / 2.0, ends - starts)
    rank = np.empty(s.size)
    rank[order] = rank_sorted
    p, nn = float((label == 1).sum()), float((label == 0).sum())
    return (rank[label == 1].sum() - p * (p + 1) / 2) / (p * nn)


def midrank_mean(pred, true):
    pred, true = pred.float().numpy(), true.double().numpy()
    cols = [k for k in range(true.shape[1]) if (true[:, k] == 1).any() and (true[:, k] == 0).any()]
    return sum(midrank_auc(pred[:, k], true[:, k]) for k in cols) / len(cols)


def sklearn_eval_rocauc(y_true, y_pred):
    """The reference's loop (large/data_utils.py:223-246), restated for the test with scikit-learn."""
    metrics = pytest.importorskip("sklearn.metrics")
    y_true = y_true.numpy()
    if y_true.shape[1] == 1:
        y_pred = torch.softmax(y_pred, dim=-1)[:, 1:2].numpy()
    else:
        y_pred = y_pred.numpy()
    vals = []
    for k in range(y_true.shape[1]):
        if (y_true[:, k] == 1).sum() > 0 and (y_true[:, k] == 0).sum() > 0:
            ok = y_true[:, k] == y_true[:, k]
            vals.append(metrics.roc_auc_score(y_true[ok, k], y_pred[ok, k]))
    return sum(vals) / len(vals)


def _case(seed, m=600, c=9, quantum=None, float_labels=False):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(m, c, generator=g) * 2
    if quantum:
        pred = torch.round(pred / quantum) * quantum
    true = (torch.rand(m, c, generator=g) < 0.35).long()
    if float_labels:
        true = true.float()
        true[torch.rand(m, c, generator=g) < 0.15] = float("nan")
    return true, pred


@pytest.mark.parametrize("quantum,float_labels", [(None, False), (0.25, False), (0.25, True), (None, True)])
def test_eval_rocauc_matches_midrank_and_sklearn(cpu_table, quantum, float_labels):
    from sgformer_amd import metrics
    true, pred = _case(3, quantum=quantum, float_labels=float_labels)
    got = metrics.eval_rocauc(true, pred)
    assert isinstance(got, float)
    ref = midrank_mean(pred, true)
    print(f"quantum={quantum} float_labels={float_labels}: got {got!r} midrank {ref!r} |d|={abs(got - ref):.2e}")
    assert abs(got - ref) <= TOL
    sk = sklearn_eval_rocauc(true, pred)
    print(f"  scikit-learn {sk!r} |d|={abs(got - sk):.2e}")
    assert abs(got - sk) <= TOL


def test_rocauc_special_scores(cpu_table):
    """All scores equal: exactly 0.5.  -0.0 == +0.0 (one tie group).  +-inf are ordinary values for rocauc_rows; the
    drop-in hands infinite scores to the original (scikit-learn rejects them)."""
    from sgformer_amd import metrics
    true, pred = _case(5, m=400, c=4, quantum=0.5)
    pred[:, 0] = 1.25
    pred[::3, 1], pred[1::3, 1], pred[2::3, 1] = 0.0, -0.0, 1.0
    assert metrics.rocauc_rows(pred[:, :1], true[:, :1]) == 0.5
    got = metrics.rocauc_rows(pred, true)
    assert abs(got - midrank_mean(pred, true)) <= TOL
    z = pred[:, 1:2].clone()
    z[z == 0] = 0.0                                    # every zero positive: the same value
    assert metrics.rocauc_rows(pred[:, 1:2], true[:, 1:2]) == metrics.rocauc_rows(z, true[:, 1:2])
    pred[::5, 2], pred[1::5, 2] = float("inf"), float("-inf")
    got = metrics.rocauc_rows(pred, true)
    assert abs(got - midrank_mean(pred, true)) <= TOL
    seen = []
    fn = metrics.make_eval_rocauc(lambda a, b: seen.append("original") or -1.0)
    assert fn(true, pred) == -1.0 and seen == ["original"]


def test_undefined_columns(cpu_table):
    from sgformer_amd import metrics
    true, pred = _case(7, m=300, c=5)
    true[:, 1], true[:, 3] = 0, 1                      # no positives / no negatives: skipped
    got = metrics.eval_rocauc(true, pred)
    assert abs(got - midrank_mean(pred, true)) <= TOL
    assert abs(got - sklearn_eval_rocauc(true, pred)) <= TOL
    true[:] = 0
    with pytest.raises(RuntimeError, match="No positively labeled data available. Cannot compute ROC-AUC."):
        metrics.eval_rocauc(true, pred)
    with pytest.raises(RuntimeError, match="No positively labeled data available"):
        metrics.rocauc_rows(pred, true)


def test_other_labels_and_nan_scores_go_to_the_original(cpu_table):
    from sgformer_amd import metrics, ops
    true, pred = _case(9, m=200, c=3)
    calls = []
    fn = metrics.make_eval_rocauc(lambda a, b: calls.append((a, b)) or 0.125)
    assert fn(true, pred) != 0.125 and not calls
    bad = true.clone()
    bad[5, 1] = 2
    assert fn(bad, pred) == 0.125 and calls[-1][0] is bad and calls[-1][1] is pred
    nan = pred.clone()
    nan[7, 2] = float("nan")
    assert fn(true, nan) == 0.125 and len(calls) == 2
    counts = ops.rocauc_counts(nan, bad)
    assert counts[:, 3].tolist() == [0, 1, 0] and counts[:, 4].tolist() == [0, 0, 1]
    with pytest.raises(ValueError):
        metrics.rocauc_rows(nan, true)
    with pytest.raises(NotImplementedError):
        metrics.eval_rocauc(bad, pred)                 # the module-level drop-in has no original bound
    assert fn(true.double(), pred) == 0.125 and fn(true, pred.double()) == 0.125      # dtypes outside the fast path


def test_one_column_softmax_form(cpu_table):
    from sgformer_amd import metrics
    g = torch.Generator().manual_seed(11)
    true = (torch.rand(500, 1, generator=g) < 0.4).long()
    pred = torch.round(torch.randn(500, 2, generator=g) * 2) / 2
    got = metrics.eval_rocauc(true, pred)
    score = torch.softmax(pred, dim=-1)[:, 1:2]
    assert abs(got - midrank_mean(score, true)) <= TOL
    assert abs(got - sklearn_eval_rocauc(true, pred)) <= TOL


@pytest.mark.parametrize("how", ["int64", "mask", "none"])
def test_rows_forms(cpu_table, how):
    """idx as int64 rows, as a bool mask, as None; labels indexed by node id; host inputs."""
    from sgformer_amd import metrics
    true, pred = _case(13, m=500, c=6, quantum=0.25, float_labels=True)
    g = torch.Generator().manual_seed(14)
    perm = torch.randperm(500, generator=g)[:320]
    idx = {"int64": perm, "mask": torch.zeros(500, dtype=torch.bool).index_fill_(0, perm, True), "none": None}[how]
    rows = torch.arange(500) if idx is None else (perm if how == "int64" else idx.nonzero().view(-1))
    got = metrics.rocauc_rows(pred, true, idx)
    assert abs(got - midrank_mean(pred[rows], true[rows])) <= TOL
    logits = torch.randn(500, 7, generator=g)
    logits[::4, 1] = logits[::4, 5] = 8.0
    logits[3::50, 2] = float("nan")
    labels = torch.randint(0, 7, (500, 1), generator=g).float()
    labels[::9] = float("nan")
    p, y = logits[rows].argmax(-1).numpy(), labels[rows, 0].numpy()
    ok = ~np.isnan(y)
    assert metrics.accuracy_rows(logits, labels, idx) == float((y[ok] == p[ok]).sum()) / ok.sum()
    assert metrics.f1_micro_rows(logits, labels, idx) == float((y == p).sum()) / len(y)
    assert metrics.accuracy_rows(logits.bfloat16(), labels[:, 0], idx) == \
        float((y[ok] == logits.bfloat16().float()[rows].argmax(-1).numpy()[ok]).sum()) / ok.sum()


def test_eval_acc_and_f1_match_the_loop_and_sklearn(cpu_table):
    from sgformer_amd import metrics
    skm = pytest.importorskip("sklearn.metrics")
    g = torch.Generator().manual_seed(17)
    logits = torch.randn(700, 6, generator=g)
    logits[::5, 0] = logits[::5, 3] = 7.0
    for labels in (torch.randint(0, 6, (700, 1), generator=g), torch.randint(0, 3, (700, 1), generator=g),
                   torch.full((700, 1), 2)):
        pred = logits.argmax(dim=-1, keepdim=True).numpy()
        y = labels.numpy()
        acc = float(np.sum(y[:, 0] == pred[:, 0])) / len(y)
        assert abs(metrics.eval_acc(labels, logits) - acc) <= TOL
        assert abs(metrics.eval_f1(labels, logits) - skm.f1_score(y, pred, average="micro")) <= TOL
    one = torch.zeros(700, 1)                                            # one predicted class, float labels with NaN
    one[::7] = float("nan")
    only0 = torch.zeros(700, 6)
    only0[:, 0] = 1.0
    assert metrics.eval_acc(one, only0) == 1.0
    fn = metrics.make_eval_f1(lambda a, b: "original")
    assert fn(one, only0) == "original"                                  # floating / unlabelled: the original decides
    assert metrics.make_eval_acc(lambda a, b: "original")(torch.zeros(5, 2), torch.zeros(5, 3)) == "original"
    assert metrics.make_eval_acc(lambda a, b: "original", min_rows=701)(torch.zeros(700, 1).long(), logits) == "original"


def test_no_autograd(cpu_table):
    from sgformer_amd import ops
    true, pred = _case(19, m=50, c=2)
    pred.requires_grad_(True)
    with pytest.raises(RuntimeError, match="not differentiable"):
        ops.rocauc_counts(pred, true)
    with pytest.raises(RuntimeError, match="not differentiable"):
        ops.argmax_count(pred, true[:, :1])
    with torch.no_grad():
        assert ops.rocauc_counts(pred, true).shape == (2, 6)


def test_fixture_of_the_live_reference(cpu_table):
    from sgformer_amd import metrics
    z = np.load(GOLDEN)
    names = sorted({k.split(".")[0] for k in z.files})
    assert len(names) == 6
    fn = {"rocauc": metrics.eval_rocauc, "acc": metrics.eval_acc, "f1": metrics.eval_f1}
    for name in names:
        got = fn[str(z[f"{name}.kind"])](torch.from_numpy(z[f"{name}.y_true"]), torch.from_numpy(z[f"{name}.y_pred"]))
        want = float(z[f"{name}.value"])
        print(f"{name}: got {got!r} recorded {want!r} |d|={abs(got - want):.2e}")
        assert isinstance(got, float) and abs(got - want) <= TOL


@pytest.mark.parametrize("mode", ["all", "device", "minimal", "host_metrics"])
def test_launcher_replaces_and_restores_the_trainers_names(cpu_table, tmp_path, monkeypatch, mode):
    from sgformer_amd import launch
    tdir = tmp_path / "large"
    tdir.mkdir()
    (tdir / "data_utils.py").write_text(
        "def eval_acc(y_true, y_pred):\n    return 'acc'\n"
        "def eval_rocauc(y_true, y_pred):\n    return 'rocauc'\n"
        "def eval_f1(y_true, y_pred):\n    return 'f1'\n")
    (tdir / "main.py").write_text(
        "import sys, torch\n"
        "from data_utils import eval_acc, eval_rocauc, eval_f1\n"
        "import data_utils\n"
        "data_utils.seen = [getattr(f, '_sgf_orig', None) is not None for f in (eval_acc, eval_rocauc, eval_f1)]\n"
        "y, p = torch.tensor([[0], [1], [1]]), torch.tensor([[2., 1.], [0., 3.], [5., 4.]])\n"
        "data_utils.values = [eval_acc(y, p), eval_f1(y, p), eval_rocauc(torch.tensor([[0, 1], [1, 0], [1, 1]]), p),\n"
        "                     eval_acc(y.double(), p)]\n")
    tg, tgu = types.ModuleType("torch_geometric"), types.ModuleType("torch_geometric.utils")
    tgu.subgraph, tgu.to_undirected, tgu.remove_self_loops, tgu.add_self_loops = "pyg-subgraph", "pyg-und", "pyg-rsl", "pyg-asl"
    tg.utils = tgu
    monkeypatch.setitem(sys.modules, "torch_geometric", tg)
    monkeypatch.setitem(sys.modules, "torch_geometric.utils", tgu)
    monkeypatch.setitem(sys.modules, "ours", None)
    monkeypatch.delitem(sys.modules, "data_utils", raising=False)
    monkeypatch.setattr(sys, "argv", list(sys.argv))
    monkeypatch.setattr(sys, "path", list(sys.path))
    adam0, adam_flag = torch.optim.Adam.__init__, getattr(torch.optim.Adam, "_sgf_patched", False)
    extra = {"all": [], "device": ["--sgf-device-metrics", "1"], "minimal": ["--sgf-patches", "minimal"],
             "host_metrics": ["--sgf-host-metrics", "1"]}[mode]
    monkeypatch.setattr(launch, "EVAL_PATCH_MIN_ROWS", {"eval_acc": 3, "eval_rocauc": 4, "eval_f1": None})
    try:
        launch.main(extra + [str(tdir / "main.py")])
        du = sys.modules["data_utils"]
        assert isinstance(du, types.ModuleType)
        if mode in ("all", "device"):
            assert du.seen == [True, True, True]
            # (float64 labels: the trainer's own function; under the size gates: 3 rows reach eval_acc's 3, not
            # eval_rocauc's 4, and eval_f1 has no measured crossover — the original)
            assert du.values == ([2.0 / 3.0, 2.0 / 3.0, 0.5, "acc"] if mode == "device" else [2.0 / 3.0, "f1", "rocauc", "acc"])
            launch.patch_eval_metrics()                                 # idempotent: the original stays the trainer's
            assert du.eval_acc._sgf_orig(None, None) == "acc"
            launch.unpatch_eval_metrics()
            assert [du.eval_acc(0, 0), du.eval_rocauc(0, 0), du.eval_f1(0, 0)] == ["acc", "rocauc", "f1"]
        else:
            assert du.seen == [False, False, False] and du.values == ["acc", "f1", "rocauc", "acc"]
    finally:
        launch.unpatch_eval_metrics()
        launch.unpatch_nll_loss()
        launch.unpatch_bce_loss()
        torch.optim.Adam.__init__ = adam0
        torch.optim.Adam._sgf_patched = adam_flag
        sys.modules.pop("data_utils", None)
