"""The output head on the rows a trainer actually reads (include/sgf.h block N6, csrc/head_rows.hip).

The neighbour-sampled trainer (100M/nb-sample.py:29 and :41) does, in every step,

    output = model(graph.x, graph.edge_index)[:batch_size]
    loss   = nn.CrossEntropyLoss()(output, graph.y[:batch_size])

on a batch of some 756 000 nodes with 1 000 seeds: 0.13 % of the logits are read, all of them are computed, stored,
zero-filled by the slice's backward and reduced into the weight gradient.  Here the head, the loss and their gradient run on
the selected rows only:

    logits(x1, x2, w, bias, a, b, rows)                 fp32 [m, C] = round(a x1[rows] + b x2[rows]) W^T + bias
    cross_entropy(x1, x2, w, bias, a, b, rows, labels)  mean cross-entropy of those rows, one forward launch

`rows`: an int k (the prefix 0..k-1), an int64 index tensor, or a bool mask over the n rows.  Whatever the kernels do not
take — aggregate='cat' (w is [C, 2 d]), d > 256, C > 256, other dtypes, an index with repeated rows — runs the same
arithmetic with the existing operators on x1[rows], x2[rows]: correct by construction, no kernel of its own.

`LazyHead` is the same for the UNCHANGED trainer: with SGF_SEED_HEAD=1 and a sampled batch, SGFormer.forward returns it in
place of the [n, C] logits; `lazy[:k]` and F.cross_entropy on that (launch.patch_ce_loss) reach the two functions above,
every other use computes what the existing path computes.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib, ops
from .kernels import _code, _launch, _scratch
from .linear import _f32c, _switch
from .ops import _rows16

_F32 = torch.float32
_BF16 = torch.bfloat16


def seed_head_enabled() -> bool:
    """SGF_SEED_HEAD: 1 = SGFormer.forward answers a sampled batch with a LazyHead; 0 (the default, see
    profiles/seed_head_probe.md) = today's head, bit for bit."""
    return _switch("SGF_SEED_HEAD", False)


# ------------------------------------------------------------------------------------------------
# the two entries on the current stream (private: the kernel table of kernels.py is not extended)
# ------------------------------------------------------------------------------------------------
class _Hip:
    @staticmethod
    def head_rows_supported(d: int, classes: int, dtype) -> bool:
        if dtype not in (_F32, _BF16):
            return False
        return bool(_lib.load().sgf_head_rows_supported(int(d), int(classes), _lib.SGF_BF16 if dtype == _BF16 else _lib.SGF_F32))

    @staticmethod
    def head_rows_fwd(x1, a: float, x2, b: float, w, bias, idx, m: int, labels=None):
        """(logits fp32 [m, C], lse fp32 [m], loss_sum fp32 [1], counts int64 [2]); the last three None without labels."""
        dev, n, d = x1.device, x1.shape[0], x1.shape[1]
        c = w.shape[0]
        logits = torch.empty((m, c), dtype=_F32, device=dev)
        lse = loss_sum = counts = None
        ws = (None, 0)
        if m == 0:          # (no rows: an empty tensor has no address to tell "no labels" from "no rows" by; nothing to launch)
            if labels is None:
                return logits, None, None, None
            return logits, torch.empty(0, dtype=_F32, device=dev), torch.zeros(1, dtype=_F32, device=dev), torch.zeros(
                2, dtype=torch.int64, device=dev)
        if labels is not None:
            lse = torch.empty(m, dtype=_F32, device=dev)
            loss_sum = torch.empty(1, dtype=_F32, device=dev)
            counts = torch.empty(2, dtype=torch.int64, device=dev)
            ws = _scratch(dev, "head_rows_fwd", _lib.load().sgf_head_rows_fwd_workspace_bytes(m))
        _launch(dev, "sgf_head_rows_fwd", x1, x1.stride(0), float(a), x2, 0 if x2 is None else x2.stride(0), float(b), w, bias,
                n, d, c, _code(x1), idx, m, logits, c, labels, lse, loss_sum, counts, *ws)
        return logits, lse, loss_sum, counts

    @staticmethod
    def head_rows_bwd(x1, a: float, x2, b: float, w, idx, m: int, dlogits=None, logits=None, lse=None, labels=None,
                      gout=None, inv_denom: float = 1.0):
        """(dx1 [n, d], dx2 [n, d] or None, dw fp32 [C, d], db fp32 [C]); dlogits, or logits + lse + labels + gout."""
        dev, n, d = x1.device, x1.shape[0], x1.shape[1]
        c = w.shape[0]
        dx1 = torch.empty((n, d), dtype=x1.dtype, device=dev)
        dx2 = None if x2 is None else torch.empty((n, d), dtype=x1.dtype, device=dev)
        dw = torch.empty((c, d), dtype=_F32, device=dev)
        db = torch.empty(c, dtype=_F32, device=dev)
        ws = _scratch(dev, "head_rows_bwd", _lib.load().sgf_head_rows_bwd_workspace_bytes(m, d, c))
        _launch(dev, "sgf_head_rows_bwd", x1, x1.stride(0), float(a), x2, 0 if x2 is None else x2.stride(0), float(b), w,
                n, d, c, _code(x1), idx, m, dlogits, 0 if dlogits is None else dlogits.stride(0), logits,
                0 if logits is None else logits.stride(0), lse, labels, gout, float(inv_denom), dx1, d, dx2,
                0 if dx2 is None else d, dw, db, *ws)
        return dx1, dx2, dw, db


def _table():
    """Where head_rows_supported / _fwd / _bwd live: a test's CPU table that has them, the entries above on the HIP table,
    nothing otherwise (every call then takes the fallback)."""
    k = ops.K
    if hasattr(k, "head_rows_fwd"):
        return k
    return _Hip if k.name == "hip" else None


# ------------------------------------------------------------------------------------------------
# rows, shapes
# ------------------------------------------------------------------------------------------------
def _select(rows, n: int, device):
    """(idx or None for a prefix, m, distinct) of the three forms of `rows`."""
    if isinstance(rows, bool) or (not torch.is_tensor(rows) and not isinstance(rows, int)):
        raise TypeError(f"head_rows: rows must be an int, an int64 index tensor or a bool mask, got {type(rows).__name__}")
    if isinstance(rows, int):
        if not 0 <= rows <= n:
            raise IndexError(f"head_rows: a prefix of {rows} rows of {n}")
        return None, rows, True
    if rows.dtype == torch.bool:
        if rows.dim() != 1 or rows.shape[0] != n:
            raise IndexError(f"head_rows: a bool mask must have shape [{n}], got {tuple(rows.shape)}")
        idx = rows.nonzero().view(-1).to(device)             # ascending, each row once
        return idx, int(idx.numel()), True
    if rows.dtype != torch.int64 or rows.dim() != 1:
        raise TypeError(f"head_rows: an index must be a 1-D int64 tensor, got {rows.dtype} {tuple(rows.shape)}")
    from .loss import _idx_is_unique
    idx = rows.to(device).contiguous()
    if idx.numel() and int(idx.max()) >= n:       # (negative entries wrap as in torch: not distinct rows, the fallback)
        raise IndexError(f"head_rows: index out of range for {n} rows")
    return idx, int(idx.numel()), _idx_is_unique(idx)


def _kernel_ok(x1, x2, w, distinct: bool):
    t = _table()
    if t is None or not distinct or x1.dim() != 2 or w.dim() != 2 or w.shape[1] != x1.shape[1]:
        return None
    if x2 is not None and (x2.shape != x1.shape or x2.dtype != x1.dtype):
        return None
    return t if t.head_rows_supported(x1.shape[1], w.shape[0], x1.dtype) else None


def _fallback_logits(x1, x2, w, bias, a: float, b: float, idx, m: int):
    """The same arithmetic with the existing operators on the selected rows (autograd accumulates repeated rows)."""
    s1 = x1[:m] if idx is None else x1[idx]
    s2 = None if x2 is None else (x2[:m] if idx is None else x2[idx])
    if m == 0:                               # (no rows: nothing for a kernel to do, the graph still reaches every operand)
        z = s1.float() if s2 is None else torch.cat([s1, s2], 1).float()[:, :w.shape[1]]
        return z @ w.float().t() + bias.float()
    if s2 is not None and w.shape[1] == s1.shape[1] + s2.shape[1]:          # aggregate='cat'
        out = ops.out_linear_cat((s1, s2), w, bias)
    elif s2 is None:
        out = ops.out_linear(s1 if a == 1.0 else (s1 * a).to(s1.dtype), w, bias)
    elif m > 0 and ops.combine_fc_supported(s1, w.shape[0]):
        out = ops.combine_fc(s1, s2, w, bias, a, b)
    else:
        out = ops.out_linear(ops.axpby(s1, s2, a, b), w, bias)
    return out.float()


def _once(what: str):
    if torch.is_grad_enabled():          # (only under create_graph=True)
        raise RuntimeError(f"sgformer_amd: {what} is once differentiable; backward with create_graph=True is not "
                           "implemented (SGF_SEED_HEAD=0 and --sgf-aten-loss 1 keep ATen's twice differentiable path)")


class _Logits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x1, x2, w, bias, a: float, b: float, idx, m: int):
        ops.K.check(x1, x2, idx)
        t = _table()
        x1, x2 = _rows16(x1), (None if x2 is None else _rows16(x2))
        w32, b32 = _f32c(w), _f32c(bias)
        ctx.save_for_backward(x1, x2, w32, idx)
        ctx.meta = (t, float(a), float(b), m, w.dtype, bias.dtype)
        return t.head_rows_fwd(x1, a, x2, b, w32, b32, idx, m)[0]

    @staticmethod
    def backward(ctx, g):
        _once("head_rows.logits")
        x1, x2, w32, idx = ctx.saved_tensors
        t, a, b, m, wdt, bdt = ctx.meta
        if g.dtype != _F32 or not g.is_contiguous():
            g = g.float().contiguous()
        dx1, dx2, dw, db = t.head_rows_bwd(x1, a, x2, b, w32, idx, m, dlogits=g)
        return dx1, dx2, dw.to(wdt), db.to(bdt), None, None, None, None


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x1, x2, w, bias, a: float, b: float, idx, m: int, labels):
        ops.K.check(x1, x2, idx, labels)
        t = _table()
        x1, x2 = _rows16(x1), (None if x2 is None else _rows16(x2))
        w32, b32 = _f32c(w), _f32c(bias)
        logits, lse, loss_sum, counts = t.head_rows_fwd(x1, a, x2, b, w32, b32, idx, m, labels)
        denom = counts[0].to(_F32)               # stays on the device; every label ignored: 0 / 0 = nan, as ATen
        ctx.save_for_backward(x1, x2, w32, idx, logits, lse, labels, denom)
        ctx.meta = (t, float(a), float(b), m, w.dtype, bias.dtype)
        return (loss_sum[0] / denom).reshape(())

    @staticmethod
    def backward(ctx, g):
        _once("head_rows.cross_entropy")
        x1, x2, w32, idx, logits, lse, labels, denom = ctx.saved_tensors
        t, a, b, m, wdt, bdt = ctx.meta
        gout = (g.float() / denom).reshape(1).contiguous()
        dx1, dx2, dw, db = t.head_rows_bwd(x1, a, x2, b, w32, idx, m, logits=logits, lse=lse, labels=labels, gout=gout,
                                           inv_denom=1.0)
        return dx1, dx2, dw.to(wdt), db.to(bdt), None, None, None, None, None


def logits(x1, x2, w, bias, a: float, b: float, rows) -> torch.Tensor:
    """fp32 [m, C] logits of the rows `rows`: round(a x1[rows] + b x2[rows]) W^T + bias (x2 may be None: round(a x1[rows])).
    Differentiable once in x1, x2, w and bias; the gradients of x1 / x2 are [n, d] with exact zeros off the rows."""
    idx, m, distinct = _select(rows, x1.shape[0], x1.device)
    if _kernel_ok(x1, x2, w, distinct) is None:
        return _fallback_logits(x1, x2, w, bias, a, b, idx, m)
    return _Logits.apply(x1, x2, w, bias, a, b, idx, m)


def cross_entropy(x1, x2, w, bias, a: float, b: float, rows, labels) -> torch.Tensor:
    """F.cross_entropy(logits(...), labels) — class-index labels int64 [m], one per SELECTED row, mean over the labels in
    [0, C) (ignore_index = -100 and every other label outside the range add nothing; all ignored: nan, as ATen) — in one
    forward launch and one backward call that forms softmax - onehot in registers."""
    idx, m, distinct = _select(rows, x1.shape[0], x1.device)
    labels = labels.reshape(-1)
    if labels.dtype != torch.int64 or labels.numel() != m:
        raise ValueError(f"head_rows.cross_entropy: labels must be int64 [{m}] (one per selected row), got {labels.dtype} "
                         f"{tuple(labels.shape)}")
    if _kernel_ok(x1, x2, w, distinct) is None:
        lg = _fallback_logits(x1, x2, w, bias, a, b, idx, m)
        c = lg.shape[1]
        return F.cross_entropy(lg, torch.where((labels >= 0) & (labels < c), labels, torch.full_like(labels, -100)))
    return _CrossEntropy.apply(x1, x2, w, bias, a, b, idx, m, labels.to(x1.device).contiguous())


# ------------------------------------------------------------------------------------------------
# The trainer's two lines AS WRITTEN (100M/nb-sample.py:29, :41) — the LazyLogSoftmax pattern of loss.py
# ------------------------------------------------------------------------------------------------
def _materialise(x):
    if isinstance(x, LazyHead):
        return x._sgf_value()
    if isinstance(x, (list, tuple)):
        return type(x)(_materialise(v) for v in x)
    if isinstance(x, dict):
        return {k: _materialise(v) for k, v in x.items()}
    return x


def _meta_funcs():
    from .loss import _META
    return _META


class LazyHead(torch.Tensor):
    """The [n, C] logits of SGFormer.forward that have not been computed yet (rows is None), or their first k rows (rows = k,
    from `lazy[:k]` with k <= the batch's seed count).  `full` computes the [n, C] logits with the existing head path."""

    @staticmethod
    def __new__(cls, x1, x2, fc, a, b, full, out_dtype, seeds, rows=None, parent=None):
        n, c = x1.shape[0], fc.weight.shape[0]
        shape = (n, c) if rows is None else (rows, c)
        grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x1, x2, fc.weight, fc.bias))
        r = torch.Tensor._make_wrapper_subclass(cls, shape, dtype=out_dtype, device=x1.device, requires_grad=bool(grad))
        r._sgf = (x1, x2, fc, float(a), float(b), full, out_dtype, int(seeds))
        r._sgf_rows, r._sgf_parent, r._sgf_cache = rows, parent, None
        return r

    def _sgf_value(self):
        if self._sgf_cache is None:
            x1, x2, fc, a, b, full, out_dtype, _ = self._sgf
            if self._sgf_rows is None:
                self._sgf_cache = full()
            elif self._sgf_parent is not None and self._sgf_parent._sgf_cache is not None:
                self._sgf_cache = self._sgf_parent._sgf_cache[:self._sgf_rows]
            else:
                self._sgf_cache = logits(x1, x2, fc.weight, fc.bias, a, b, self._sgf_rows).to(out_dtype)
        return self._sgf_cache

    def _sgf_cross_entropy(self, target):
        x1, x2, fc, a, b, _, out_dtype, _ = self._sgf
        loss = cross_entropy(x1, x2, fc.weight, fc.bias, a, b, self._sgf_rows, target)
        return loss if out_dtype == loss.dtype else loss.to(out_dtype)

    def __deepcopy__(self, memo):
        return self._sgf_value().detach().clone()

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if (func is torch.Tensor.__getitem__ and len(args) == 2 and isinstance(args[0], LazyHead)
                and args[0]._sgf_rows is None and args[0]._sgf_cache is None and isinstance(args[1], slice)
                and args[1].start in (None, 0) and args[1].step in (None, 1) and isinstance(args[1].stop, int)
                and not isinstance(args[1].stop, bool) and 0 <= args[1].stop <= min(args[0]._sgf[7], args[0].shape[0])):
            s = args[0]
            return LazyHead(*s._sgf, rows=args[1].stop, parent=s)
        with torch._C.DisableTorchFunctionSubclass():
            if func in _meta_funcs():          # shape / dtype / device ... live on the wrapper: nothing is computed for them
                return func(*args, **kwargs)
            return func(*_materialise(args), **_materialise(kwargs))

    @classmethod
    def __torch_dispatch__(cls, func, types, args=(), kwargs=None):        # (whatever reaches the dispatcher: real values)
        return func(*_materialise(args), **_materialise(kwargs or {}))


def lazy_cross_entropy_ok(input, target, weight, size_average, ignore_index, reduce, reduction, label_smoothing) -> bool:
    """Is this F.cross_entropy call the trainer's (lazy rows, int64 class indices, no weights, no smoothing, mean,
    ignore_index -100)?  Everything else goes to the original with the real logits."""
    return (isinstance(input, LazyHead) and input._sgf_rows is not None and input._sgf_cache is None
            and torch.is_tensor(target) and not isinstance(target, LazyHead) and target.dtype == torch.int64
            and target.dim() == 1 and target.shape[0] == input.shape[0] and target.device == input.device
            and weight is None and size_average is None and reduce is None and reduction == "mean"
            and ignore_index == -100 and label_smoothing == 0.0)
