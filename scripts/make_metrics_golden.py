"""Write tests/golden/metrics/metrics_eval.npz: seeded inputs and the values the LIVE reference's eval_rocauc / eval_acc / eval_f1
(large/data_utils.py) return for them.  Run where the reference is mounted (SGF_REFERENCE_ROOT, oracle/ref_shim.py):

    python scripts/make_metrics_golden.py

The reference's data_utils is imported unchanged over the stand-ins the other fixtures use (a subdirectory: the model tests take every tests/golden/*.npz for a model fixture; tests/standins for
google_drive_downloader, oracle.ref_shim for torch_sparse); scikit-learn must be installed.  Tests read only the fixture.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests", "standins"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "metrics", "metrics_eval.npz")


def reference_data_utils():
    ref_shim.install_stand_ins()
    path = os.path.join(ref_shim.REFERENCE_ROOT, "large", "data_utils.py")
    spec = importlib.util.spec_from_file_location("_sgf_reference_large_data_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    """name -> (kind, y_true, y_pred): multi-label AUC (int64 and float labels with NaN, heavy ties, a column without
    positives), the one-column softmax form, accuracy with NaN labels, micro-F1 with differing class sets."""
    g = torch.Generator().manual_seed(20240611)
    out = {}
    m, c = 700, 12
    pred = torch.randn(m, c, generator=g) * 2
    true = (torch.rand(m, c, generator=g) < 0.3).long()
    true[:, 5] = 0                                           # a column without positives: skipped
    out["auc_i64"] = ("rocauc", true, pred)
    tied = torch.round(torch.randn(m, c, generator=g) * 4) / 4    # scores on a 0.25 grid: long tie groups
    tied[::7, 0], tied[1::7, 0] = 0.0, -0.0
    tied[::11, 1], tied[1::11, 1] = 3.0e38, -3.0e38          # (scikit-learn rejects +-inf scores: the largest finite ones)
    tied[:, 2] = 1.5                                         # all scores equal: AUC exactly 0.5
    ftrue = true.float()
    ftrue[torch.rand(m, c, generator=g) < 0.1] = float("nan")
    out["auc_f32_nan_ties"] = ("rocauc", ftrue, tied)
    out["auc_binary_softmax"] = ("rocauc", (torch.rand(900, 1, generator=g) < 0.4).long(), torch.randn(900, 2, generator=g))
    logits = torch.randn(800, 7, generator=g)
    logits[::9, 2] = logits[::9, 4] = 9.0                    # first-index ties
    labels = torch.randint(0, 7, (800, 1), generator=g)
    out["acc_i64"] = ("acc", labels, logits)
    flabels = labels.float()
    flabels[::13] = float("nan")
    out["acc_f32_nan"] = ("acc", flabels, logits)
    out["f1_i64"] = ("f1", torch.randint(0, 5, (800, 1), generator=g), logits)     # true classes 0..4, predicted 0..6
    return out


def main():
    du = reference_data_utils()
    fn = {"rocauc": du.eval_rocauc, "acc": du.eval_acc, "f1": du.eval_f1}
    blob = {}
    for name, (kind, y_true, y_pred) in cases().items():
        value = float(fn[kind](y_true, y_pred))
        blob[f"{name}.kind"] = np.array(kind)
        blob[f"{name}.y_true"] = y_true.numpy()
        blob[f"{name}.y_pred"] = y_pred.numpy()
        blob[f"{name}.value"] = np.float64(value)
        print(f"{name}: {kind} = {value!r}")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **blob)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
