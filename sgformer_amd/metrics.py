"""The trainers' evaluation metrics on the device (include/sgf.h block N5; large/data_utils.py:199-246 and the same
functions in medium/ and 100M/).

    from sgformer_amd.metrics import rocauc_rows, accuracy_rows, f1_micro_rows
    auc = rocauc_rows(out, dataset.label, split_idx['valid'])

`label` is indexed by NODE id; `idx` is int64 rows, a bool mask over N or None for every row, as
loss.bce_with_logits_rows takes them.  The kernels return integer counts (sgf_rocauc_counts: per column P, Nn and the
Mann-Whitney count U2; sgf_argmax_count: labelled rows and hits); one device->host read per call brings them over and the
metric is finished here in float64: AUC_k = U2 / (2 P Nn), the mean over the columns that have a positive and a negative,
in column order.

`eval_rocauc`, `eval_acc` and `eval_f1` are drop-ins with the reference's signatures and return values for the unchanged
trainers (sgformer_amd.launch.patch_eval_metrics binds each to the trainer's own function).  Host tensors are accepted and
staged to the current GPU: evaluate_large hands over host logits.  The house rule of loss.py holds: whatever the fast path
does not cover goes to the original — other dtypes and shapes, a label that is neither 0, 1 nor NaN, a NaN or infinite
score (scikit-learn raises or handles those), unlabelled rows in eval_f1, an empty selection.
"""
from __future__ import annotations

import torch

from . import ops

NO_POSITIVE = "No positively labeled data available. Cannot compute ROC-AUC."


def _device_table() -> bool:
    return ops.K.name == "hip"


def _usable() -> bool:
    """Can the current kernel table serve the metrics?  libsgf needs a GPU; a CPU table (tests) needs the two entries."""
    if _device_table():
        return torch.cuda.is_available()
    return hasattr(ops.K, "rocauc_counts") and hasattr(ops.K, "argmax_count")


def _stage(*tensors):
    """Host tensors -> the current GPU when the kernel table is libsgf's (a CPU table takes them as they are); device
    tensors decide the device for the rest."""
    if not _device_table():
        return tensors
    dev = next((t.device for t in tensors if t is not None and t.is_cuda), None)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return tuple(None if t is None else (t if t.device == dev else t.to(dev, non_blocking=False)) for t in tensors)


def _scores(out, what):
    if not torch.is_tensor(out) or out.dim() != 2:
        raise ValueError(f"{what}: `out` must be a [N, C] tensor")
    if out.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{what}: `out` must be float32 or bfloat16, got {out.dtype}")
    return out.detach()


def _labels(label, what):
    """float32 and int64 are read as stored; bool / other integers become int64, half / bfloat16 become float32 (exact)."""
    label = label.detach()
    if label.dtype in (torch.float32, torch.int64):
        return label
    if label.dtype in (torch.float16, torch.bfloat16):
        return label.to(torch.float32)
    if not label.is_floating_point() and not label.is_complex():
        return label.to(torch.int64)
    raise TypeError(f"{what}: labels must be float32 / float16 / bfloat16, bool or integer, got {label.dtype}")


def auc_from_counts(counts):
    """counts: [C, 6] integers on the host -> (list of the defined columns' AUCs in column order, other, nan_scores)."""
    rows = counts.tolist()
    aucs = [u2 / (2 * p * nn) for p, nn, u2, _o, _s, _u in rows if p > 0 and nn > 0]    # (exact integers, one division)
    return aucs, sum(r[3] for r in rows), sum(r[4] for r in rows)


def rocauc_rows(out, label, idx=None) -> float:
    """Mean over the label columns of the ROC-AUC of `out[idx, k]` against `label[idx, k]` (0 / 1; NaN = unlabelled, those
    rows are dropped per column), ties counted half — scikit-learn's roc_auc_score per column, ogb's evaluator for
    ogbn-proteins.  Columns without a positive or without a negative are skipped; RuntimeError if none is left; ValueError
    for a label that is neither 0, 1 nor NaN, or a NaN score."""
    out, label = _scores(out, "rocauc_rows"), _labels(label, "rocauc_rows")
    if label.dim() == 1:
        label = label.unsqueeze(1)
    out, label, idx = _stage(out, label, idx)
    aucs, other, nans = auc_from_counts(ops.rocauc_counts(out, label, idx).cpu())
    if other or nans:
        raise ValueError(f"rocauc_rows: {other} label(s) that are neither 0, 1 nor NaN and {nans} NaN score(s) in the "
                         "selected rows")
    if not aucs:
        raise RuntimeError(NO_POSITIVE)
    return sum(aucs) / len(aucs)


def _hits(out, label, idx, what):
    out, label = _scores(out, what), _labels(label, what)
    out, label, idx = _stage(out, label, idx)
    if idx is not None and idx.dtype == torch.bool:
        idx = idx.nonzero().view(-1)                  # (once, here: its length is the row count)
    labelled, correct = ops.argmax_count(out, label, idx).cpu().tolist()
    return (out.shape[0] if idx is None else idx.numel()), labelled, correct


def accuracy_rows(out, label, idx=None) -> float:
    """Share of the labelled rows of `idx` whose argmax equals the label (`label`: [N] or [N, 1], NaN = unlabelled)."""
    _m, labelled, correct = _hits(out, label, idx, "accuracy_rows")
    if labelled == 0:
        raise ZeroDivisionError("accuracy_rows: no labelled row selected")
    return float(correct) / labelled


def f1_micro_rows(out, label, idx=None) -> float:
    """Micro-averaged F1 of the argmax predictions: for one prediction per row it equals the share of ALL selected rows
    whose argmax equals the label, whatever the class sets are (a NaN label counts as a miss)."""
    m, _labelled, correct = _hits(out, label, idx, "f1_micro_rows")
    if m == 0:
        raise ZeroDivisionError("f1_micro_rows: no row selected")
    return float(correct) / m


# ------------------------------------------------------------------------------------------------
# drop-ins for the trainers' eval_func (large/data_utils.py:199-246)
# ------------------------------------------------------------------------------------------------
def _pair_ok(y_true, y_pred, min_rows):
    return (_usable() and type(y_true) is torch.Tensor and type(y_pred) is torch.Tensor and y_true.dim() == 2
            and y_pred.dim() == 2 and y_pred.dtype == torch.float32 and y_true.shape[0] == y_pred.shape[0]
            and min_rows <= y_true.shape[0] < 2 ** 31 and y_pred.shape[1] >= 1
            and (y_true.dtype in (torch.float32, torch.float16, torch.bfloat16) or
                 not (y_true.is_floating_point() or y_true.is_complex())))


def _missing(name):
    def original(y_true, y_pred):
        raise NotImplementedError(f"sgformer_amd.metrics.{name}: this call is outside the device path and no original "
                                  "function is bound (sgformer_amd.launch.patch_eval_metrics binds the trainer's own)")
    return original


def make_eval_rocauc(original=None, min_rows: int = 0):
    original = original or _missing("eval_rocauc")

    def eval_rocauc(y_true, y_pred):
        if not _pair_ok(y_true, y_pred, min_rows) or not (
                (y_true.shape[1] == 1 and y_pred.shape[1] >= 2) or (y_true.shape[1] > 1 and y_true.shape == y_pred.shape)):
            return original(y_true, y_pred)
        true, pred = _stage(_labels(y_true, "eval_rocauc"), y_pred.detach())
        if true.shape[1] == 1:
            # the reference's binary form: the score is the softmax probability of class 1 (ATen, on the device)
            pred = torch.nn.functional.softmax(pred, dim=-1)[:, 1].unsqueeze(1).contiguous()
        counts = ops.rocauc_counts(pred, true, None)
        # scikit-learn rejects infinite scores, which the kernel ranks as ordinary values: the flag rides along with
        # the counts in the one host read
        inf = torch.isinf(pred).any().to(counts.dtype).reshape(1)
        host = torch.cat([counts.reshape(-1), inf]).cpu()
        aucs, other, nans = auc_from_counts(host[:-1].reshape(-1, 6))
        if other or nans or int(host[-1]):
            return original(y_true, y_pred)
        if not aucs:
            raise RuntimeError(NO_POSITIVE)
        return sum(aucs) / len(aucs)

    return eval_rocauc


def _argmax_counts(y_true, y_pred):
    true, pred = _stage(_labels(y_true, "eval"), y_pred.detach())
    return ops.argmax_count(pred, true, None).cpu().tolist()


def make_eval_acc(original=None, min_rows: int = 0):
    original = original or _missing("eval_acc")

    def eval_acc(y_true, y_pred):
        if not _pair_ok(y_true, y_pred, min_rows) or y_true.shape[1] != 1:
            return original(y_true, y_pred)
        labelled, correct = _argmax_counts(y_true, y_pred)
        if labelled == 0:
            return original(y_true, y_pred)
        return float(correct) / labelled

    return eval_acc


def make_eval_f1(original=None, min_rows: int = 0):
    original = original or _missing("eval_f1")

    def eval_f1(y_true, y_pred):
        # (floating labels: scikit-learn first decides whether they are classes at all — the original's business)
        if not _pair_ok(y_true, y_pred, min_rows) or y_true.shape[1] != 1 or y_true.is_floating_point():
            return original(y_true, y_pred)
        labelled, correct = _argmax_counts(y_true, y_pred)
        m = y_true.shape[0]
        if labelled != m or m == 0:           # (unlabelled rows: the reference does not filter them, scikit-learn decides)
            return original(y_true, y_pred)
        return float(correct) / m

    return eval_f1


eval_rocauc = make_eval_rocauc()
eval_acc = make_eval_acc()
eval_f1 = make_eval_f1()

MAKERS = {"eval_rocauc": make_eval_rocauc, "eval_acc": make_eval_acc, "eval_f1": make_eval_f1}
