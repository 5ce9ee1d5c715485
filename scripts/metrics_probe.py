"""Time the evaluation metrics against the functions they replace, on one GPU box in one run -> profiles/metrics_probe.md.

    python scripts/metrics_probe.py [--reps 20] [--out profiles/metrics_probe.md] [--only NAME]

Per shape: (a) the ORIGINAL function — the reference's loop restated here with scikit-learn (scipy.stats.rankdata when
scikit-learn is missing) on host tensors, as evaluate_large calls it; (b) the drop-in on the same host tensors, staging
included; (c) the drop-in on device tensors; (d) the device time of the kernel-table call alone, between two HIP events,
and for sgf_rocauc_counts its three stages — key pass, radix sort, rank pass — by difference of the same call stopped
after the first and after the second stage (SGF_ROCAUC_STAGES, csrc/metrics.hip).  Warm-up first, then `--reps` repetitions; median and the min .. max spread.  The comparison is (a) against
(b) / (c) in this same run.  Next to the key pass the box's own copy rate is printed (torch's device-to-device copy of a
buffer of the size the key pass moves)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [  # name, kind, rows, logits columns
    ("proteins train", "rocauc", 86619, 112), ("proteins valid", "rocauc", 21236, 112), ("proteins test", "rocauc", 24679, 112),
    ("binary 168114", "rocauc1", 168114, 2), ("products accuracy", "acc", 2449029, 47),
    ("arxiv accuracy", "acc", 90941, 40), ("small accuracy", "acc", 1000, 7), ("small auc", "rocauc", 2000, 112),
    ("arxiv micro-F1", "f1", 90941, 40), ("small micro-F1", "f1", 1000, 7),
]


def original_rocauc(y_true, y_pred):
    try:
        from sklearn.metrics import roc_auc_score as auc
    except ImportError:
        from scipy.stats import rankdata

        def auc(t, s):
            r, p = rankdata(s), float((t == 1).sum())
            return (r[t == 1].sum() - p * (p + 1) / 2) / (p * (len(t) - p))
    y_true = y_true.detach().cpu().numpy()
    if y_true.shape[1] == 1:
        y_pred = torch.softmax(y_pred, dim=-1)[:, 1].unsqueeze(1).cpu().numpy()
    else:
        y_pred = y_pred.detach().cpu().numpy()
    vals = []
    for i in range(y_true.shape[1]):
        if np.sum(y_true[:, i] == 1) > 0 and np.sum(y_true[:, i] == 0) > 0:
            ok = y_true[:, i] == y_true[:, i]
            vals.append(auc(y_true[ok, i], y_pred[ok, i]))
    return sum(vals) / len(vals)


def original_acc(y_true, y_pred):
    y_true = y_true.detach().cpu().numpy()
    y_pred = y_pred.argmax(dim=-1, keepdim=True).detach().cpu().numpy()
    ok = y_true[:, 0] == y_true[:, 0]
    correct = y_true[ok, 0] == y_pred[ok, 0]
    return float(np.sum(correct)) / len(correct)


def original_f1(y_true, y_pred):
    from sklearn.metrics import f1_score
    y_true = y_true.detach().cpu().numpy()
    y_pred = y_pred.argmax(dim=-1, keepdim=True).detach().cpu().numpy()
    vals = [f1_score(y_true, y_pred, average="micro") for _ in range(y_true.shape[1])]
    return sum(vals) / len(vals)


def timed(fn, reps, warm=2):
    for _ in range(warm):
        value = fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        value = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return value, ts


def events(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def fmt(ts):
    return f"{statistics.median(ts):.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--orig-reps", type=int, default=0, help="repetitions of the original (default: --reps)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_probe.md"))
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_probe: no GPU visible; timings are taken on the device only")
    from sgformer_amd import _lib, metrics, ops
    dev = torch.device("cuda", 0)
    rows = ["| shape | original, host tensors (ms) | drop-in, host tensors (ms) | drop-in, device tensors (ms) | "
            "kernels, HIP events (ms) | original / drop-in (host) | value: original, drop-in |", "|---|---|---|---|---|---|---|"]
    notes, ratios = [], {}
    lib = _lib.load()
    for name, kind, m, c in SHAPES:
        if args.only and args.only != name:
            continue
        g = torch.Generator().manual_seed(m)
        pred = torch.randn(m, c, generator=g)
        if kind == "rocauc":
            true = (torch.rand(m, c, generator=g) < 0.3).long()
            orig, new = original_rocauc, metrics.eval_rocauc
            kern = lambda p, t: ops.K.rocauc_counts(p, t, None)                      # noqa: E731
        elif kind == "rocauc1":
            true = (torch.rand(m, 1, generator=g) < 0.4).long()
            orig, new = original_rocauc, metrics.eval_rocauc
            kern = lambda p, t: ops.K.rocauc_counts(p[:, 1:2].contiguous(), t, None)  # noqa: E731
        else:
            true = torch.randint(0, c, (m, 1), generator=g)
            orig, new = (original_acc, metrics.eval_acc) if kind == "acc" else (original_f1, metrics.eval_f1)
            kern = lambda p, t: ops.K.argmax_count(p, t, None)                       # noqa: E731
        pd, td = pred.to(dev), true.to(dev)
        v0, t_orig = timed(lambda: orig(true, pred), args.orig_reps or args.reps, warm=1)
        v1, t_host = timed(lambda: new(true, pred), args.reps)
        v2, t_dev = timed(lambda: new(td, pd), args.reps)
        t_k = events(lambda: kern(pd, td), args.reps)
        cell = fmt(t_k)
        if kind in ("rocauc", "rocauc1"):
            stage = {}
            for st in (1, 2):
                os.environ["SGF_ROCAUC_STAGES"] = str(st)
                lib.sgf_reload_env()
                stage[st] = events(lambda: kern(pd, td), args.reps)
            os.environ.pop("SGF_ROCAUC_STAGES")
            lib.sgf_reload_env()
            k1, k2, k3 = (statistics.median(stage[1]), statistics.median(stage[2]), statistics.median(t_k))
            cell += f"; keys {k1:.3f}, sort {k2 - k1:.3f}, rank {k3 - k2:.3f}"
        ratio = statistics.median(t_orig) / statistics.median(t_host)
        ratios[(kind, m)] = (statistics.median(t_orig), min(t_orig), max(t_orig), statistics.median(t_host))
        rows.append(f"| {name} [{m} x {c}] | {fmt(t_orig)} | {fmt(t_host)} | {fmt(t_dev)} | {cell} | {ratio:.2f} x | "
                    f"{v0!r}, {v1!r} |")
        print(rows[-1], flush=True)
        if abs(v0 - v1) > 1e-12 or abs(v0 - v2) > 1e-12:
            notes.append(f"- {name}: original {v0!r}, drop-in on host tensors {v1!r}, on device tensors {v2!r}")
        if kind == "rocauc":
            # the key pass reads m c (4 + 8) bytes and writes m c 8: time a device copy that moves as many bytes
            nbytes = m * c * 20
            buf = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(buf)
            t_c = events(lambda: dst.copy_(buf), args.reps)
            notes.append(f"- {name}: the key pass moves {nbytes / 1e6:.1f} MB (reads fp32 logits and int64 labels, writes 64-bit "
                         f"keys) in {k1:.3f} ms = {nbytes / k1 / 1e6:.0f} GB/s; this box copies as many bytes device-to-device "
                         f"in {fmt(t_c)} ms = {nbytes / statistics.median(t_c) / 1e6:.0f} GB/s.")
    gold = os.path.join(ROOT, "tests", "golden", "metrics", "metrics_eval.npz")
    if not args.only and os.path.exists(gold):
        z = np.load(gold)
        yt, yp = torch.from_numpy(z["auc_binary_softmax.y_true"]), torch.from_numpy(z["auc_binary_softmax.y_pred"])
        got, want = metrics.eval_rocauc(yt.to(dev), yp.to(dev)), float(z["auc_binary_softmax.value"])
        notes.append(f"- one-column softmax form, fixture `auc_binary_softmax` (900 rows): the drop-in with the device's softmax "
                     f"gives {got!r}, the reference recorded {want!r} with the CPU softmax: |d| = {abs(got - want):.3e}.")
    text = ["# Evaluation metrics: the original functions against the device drop-ins", "",
            f"`python scripts/metrics_probe.py --reps {args.reps}` on {torch.cuda.get_device_name(0)}, torch "
            f"{torch.__version__}, {torch.get_num_threads()} host threads.  Random fp32 scores; labels int64.  Times in ms: median "
            "(min .. max).  The original is the reference's loop with scikit-learn on host tensors; every column is timed in "
            "the same process, one after the other.", ""] + rows + [""] + notes + [""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
