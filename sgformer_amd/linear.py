"""The Linear layers of the path as autograd operators (split out of ops.py in r06): T4 — every y = x W^T + b of
large/ours.py (:123-126, :36-40, :77, :198, :275), the two input stems with their BatchNorm / LayerNorm, and T6 — the GraphConv
layer's Linear + BatchNorm + relu + residual with its chained input gradients.  `ops` re-exports every name."""
from __future__ import annotations

import os
from functools import partial
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from .kernels import _pair_gram, _rows, _rows16

_F32 = torch.float32
_BF16 = torch.bfloat16

from .graph import K, _has  # noqa: E402,F401  (ONE kernel table, rebound in every module by ops.set_kernels; one probe)


def _f32c(t):
    """A parameter (or None) as the kernels read it: fp32, contiguous, outside autograd."""
    return None if t is None else t.detach().float().contiguous()


def _switch(name: str, default: bool) -> bool:
    """The environment switch `name`: on by default and turned off with 0, or off by default and turned on with 1.  Read on
    every call — the tests flip switches at run time."""
    v = os.environ.get(name)
    return default if v is None else (v != "0" if default else v == "1")


# BatchNorm's batch statistics of a tensor (large/ours.py:77-81, :87-88): shifted one-pass column sums
_BN_SAMPLE_ROWS = 1024


class BNSums(NamedTuple):
    """What the statistics pass leaves of a [n, d] tensor: sums = [sum (x - shift) | sum (x - shift)^2] over all rows (all
    ranks when sharded) in fp32, the shift they were taken about, and the row count."""
    sums: torch.Tensor
    shift: Optional[torch.Tensor]
    count: float

    def moments(self):
        """(mean, biased variance, count): mean = shift + m1, var = m2 - m1^2 with m1 ~ sigma / sqrt(sample) — no
        cancellation, unlike the unshifted E[x^2] - E[x]^2."""
        d = self.sums.numel() // 2
        m1 = self.sums[:d] / max(self.count, 1.0)
        mean = m1 if self.shift is None else self.shift + m1
        return mean, (self.sums[d:] / max(self.count, 1.0) - m1 * m1).clamp_min_(0.0), self.count


def _shifted_sums(launch, d: int, n: int, device, shard):
    """(out, BNSums) of a producer of n rows of width d in ONE pass over its operand.  `launch(rows, shift, want_stats)` runs
    the producer on the first `rows` rows (None: all) and returns (its output, the sums about `shift`).

    The shift is the column mean of a small leading sample of rows (a ~10 us launch), then the full launch accumulates the
    shifted sums — half the HBM traffic of the two-pass form.  Node-sharded runs all-reduce the sample sums with their count
    (so that every rank uses the same shift) and then the two sums."""
    ns = min(n, _BN_SAMPLE_ROWS)
    _, st_s = launch(ns, None, True)
    count = float(n)
    if shard is None:
        shift = st_s[:d] * (1.0 / float(max(ns, 1)))          # one launch; the sharded form needs the global sample count
    else:
        samp = torch.cat([st_s[:d], torch.full((1,), float(ns), dtype=_F32, device=device)])
        shard.all_reduce(samp)
        count = float(shard.n_global)
        shift = (samp[:d] / samp[d].clamp_min(1.0)).contiguous()
    out, st = launch(None, shift, True)
    if shard is not None:
        shard.all_reduce(st)
    return out, BNSums(st, shift, count)


def _column_sums(x: torch.Tensor, shard=None) -> BNSums:
    x = _rows(x.detach())
    return _shifted_sums(lambda rows, shift, _: (None, K.colstats(x if rows is None else x[:rows], shift)),
                         x.shape[1], x.shape[0], x.device, shard)[1]


def batch_stats(x: torch.Tensor, shard=None):
    """Column mean / biased variance over all rows (all ranks when sharded) in ONE pass over x (sgf_colstats)."""
    K.check(x)
    return _column_sums(x, shard).moments()


def _bn_param_grads(stats, d: int, g32, be32, dtype, shard):
    """(d gamma, d beta) out of BatchNorm backward's sums [sum dz | sum dz xhat].  Node-sharded: the sums are global already
    and ShardContext.sync_grads sums parameter gradients over the ranks again — pre-divide."""
    dgamma = stats[d:].to(dtype) if g32 is not None else None
    dbeta = stats[:d].to(dtype) if be32 is not None else None
    if shard is not None and g32 is not None:
        dgamma, dbeta = shard.unsum(dgamma), shard.unsum(dbeta)
    return dgamma, dbeta


# ------------------------------------------------------------------------------------------------
# T4: the Linear layers  y = x W^T + b  (large/ours.py:123-126, :36-40, :77, :198, :275).
# bf16 storage, square layers of width 64 / 128 / 256 (and pairs [x1 | x2] of them): forward, the BatchNorm column sums of
# the output and dX on the streaming row kernels (sgf_gcn_epilogue_*, csrc/rowgemm.hip); fp32 storage, widths % 4 up to 256:
# the exact-fp32 streaming kernel (csrc/linear_f32.hip); EVERY other shape: the general matrix-core kernel sgf_gemm
# (csrc/gemm.hip) — no Linear of the path is a library GEMM.  The weight / bias gradients
#     dW = dY^T X   (a d x d <- [N x d]^T [N x d] reduction over all nodes),   db = colsum(dY)
# always run on sgf_gram: hipBLASLt's kernels for that shape ran at 0.7 TB/s (3.6 ms per call at
# ogbn-products scale, profiles/r01_products_bf16_kernel_stats.md) and ATen's column reduction for
# the bias gradient at 18.6 ms for C = 47.  Master weights may be fp32 while activations are bf16.
# ------------------------------------------------------------------------------------------------
class _Linear(torch.autograd.Function):
    """y = sum_i x_i W_i^T + b with W = [W_1 | W_2 | ...] split along its input dimension
    (one operand for nn.Linear; two for GraphConvLayer's W [A x | x0], large/ours.py:36-38,
    without materialising the concatenation)."""

    @staticmethod
    def forward(ctx, w, b, want_stats: bool, shard, *xs):
        """(y, BNSums of y for the BatchNorm that follows — None unless asked for)."""
        K.check(*xs)
        dt = xs[0].dtype
        wc = w if w.dtype == dt else w.to(dt)
        widths = [x.shape[1] for x in xs]
        if sum(widths) != w.shape[1]:
            raise RuntimeError(f"linear: input widths {widths} do not add up to {w.shape[1]}")
        offs = [sum(widths[:i]) for i in range(len(widths))]
        fused = (len(xs) <= 2 and all(_streaming_linear_ok(x, wc[:, o:o + k]) for x, o, k in zip(xs, offs, widths)))
        if fused:
            # streaming passes with W resident in LDS (sgf_gcn_epilogue_*); the BatchNorm that follows gets its
            # column sums from the same pass
            xr = [_rows16(x) for x in xs]
            y, stats = _linear_with_stats(xr, wc, _f32c(b), shard) if want_stats else _streaming_linear(xr, wc, _f32c(b))
        else:
            # any other shape (input widths beyond 256 or not multiples of 4, odd hidden widths, multi-head projections):
            # the general matrix-core kernel (sgf_gemm, csrc/gemm.hip) — first operand with the bias, the rest accumulated
            # IN PLACE; W's column blocks are passed as strided views (no copy, no transposition)
            y = K.gemm(xs[0], wc[:, :widths[0]].t(), bias=_f32c(b))
            off = widths[0]
            for x, k in zip(xs[1:], widths[1:]):
                K.gemm(x, wc[:, off:off + k].t(), out=y, beta=1.0, addend=y)
                off += k
            stats = _column_sums(y, shard) if want_stats else None
        ctx.save_for_backward(wc, *xs)
        ctx.meta = (w.dtype, None if b is None else b.dtype, widths)
        return y, stats

    @staticmethod
    def backward(ctx, g, _):
        wc, *xs = ctx.saved_tensors
        wdtype, bdtype, widths = ctx.meta
        g = g.contiguous()
        need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and bdtype is not None
        dxs, off = [], 0
        for i, k in enumerate(widths):
            if not ctx.needs_input_grad[4 + i]:
                dxs.append(None)
            elif _streaming_linear_ok(g, wc[:, off:off + k], dx=True):
                dxs.append(K.gcn_epilogue_dx(_rows16(g), wc[:, off:off + k]))
            else:
                dxs.append(K.gemm(g, wc[:, off:off + k]))
            off += k
        dw, db = _linear_param_grads(g, xs, widths, need_w, need_b, wdtype, bdtype)
        return (dw, db, None, None, *dxs)


def _linear_param_grads(g, xs, widths, need_w, need_b, wdtype, bdtype):
    """dW = g^T [x_1 | x_2 | ...], db = sum_n g on sgf_gram (one node reduction per operand)."""
    dw = db = None
    if need_w or need_b:
        # sgf_gram wants widths that are multiples of 4 elements: zero-pad the odd ones (e.g. the
        # C = 47 logits gradient: one extra [N, 48] pass) and slice the result
        m = g.shape[1]
        gp = _rows(g if m % 4 == 0 else F.pad(g, (0, 4 - m % 4)))
        dw = torch.empty((gp.shape[1], sum(widths)), dtype=_F32, device=g.device)
        off = 0
        if (len(xs) == 2 and widths[0] == widths[1] and widths[0] % 4 == 0 and _has(K, "gram2") and gp.dtype == _BF16
                and xs[0].dtype == _BF16 and xs[1].dtype == _BF16 and _pair_gram()):
            # both blocks of dW = g^T [x_1 | x_2] from ONE read of g out of HBM (paired launch, sgf_gram2)
            k = widths[0]
            db = K.gram2(gp, _rows(xs[0]), _rows(xs[1]), dw[:, :k], dw[:, k:], want_colsum=need_b)
            xs, widths = [], []
        for i, (x, k) in enumerate(zip(xs, widths)):
            if k % 4 == 0 and off % 4 == 0:   # sgf_gram stores float4s: the slice must stay 16-B aligned
                _, cs = K.gram(gp, _rows(x), out=dw[:, off:off + k], want_colsum=(i == 0 and need_b))
            elif k % 4 == 0:
                blk, cs = K.gram(gp, _rows(x), want_colsum=(i == 0 and need_b))
                dw[:, off:off + k] = blk
            else:
                xp = _rows(F.pad(x, (0, 4 - k % 4)))
                blk, cs = K.gram(gp, xp, want_colsum=(i == 0 and need_b))
                dw[:, off:off + k] = blk[:, :k]
            if i == 0:
                db = cs
            off += k
        dw = dw[:m].to(wdtype) if need_w else None
        db = db[:m].to(bdtype) if need_b else None
    return dw, db


def _batchnorm_of(book, launch, d: int, n: int, device, shard):
    """(the output of `launch`, mean, rstd, count, used batch statistics): a producer's output and the BatchNorm that `book`
    — the module's bookkeeping, ours._BNBook — decides for it: batch statistics out of the producer's own pass (the running
    ones updated on the way), or the running statistics."""
    if book.use_batch():
        out, stats = _shifted_sums(launch, d, n, device, shard)
        mean, rstd, count, used = book.from_sums(stats)
    else:
        out = launch(None, None, False)[0]
        mean, rstd, count, used = book.running()
    return out, _f32c(mean), _f32c(rstd), count, used


def _stem_launch(x, w0c, w1c, b32):
    """Both stems as a `launch` of _shifted_sums: ((y0, y1), sums of y0); the statistics sample computes y0 alone."""
    def launch(rows, shift, want_stats):
        if rows is not None:
            return None, K.stem_pair(x[:rows], w0c, b32[0], None, None, None, want_stats0=True)[2]
        y0, y1, st = K.stem_pair(x, w0c, b32[0], w1c, b32[1], shift, want_stats0=want_stats)
        return (y0, y1), st
    return launch


class _StemPair(torch.autograd.Function):
    """(y0, y1, BNSums of y0 or None) with (y0, y1) = (x W0^T + b0, x W1^T + b1) from ONE pass over x — the first Linear of
    GraphConv and of TransConv (large/ours.py:77, :198) read the same node features; the column sums y0's BatchNorm needs
    ride along when asked for."""

    @staticmethod
    def forward(ctx, x, w0, b0, w1, b1, want_stats: bool, shard):
        K.check(x)
        dt = x.dtype
        w0c, w1c = w0.to(dt), w1.to(dt)
        launch = _stem_launch(x, w0c, w1c, [_f32c(b0), _f32c(b1)])
        if want_stats:
            (y0, y1), stats = _shifted_sums(launch, w0.shape[0], x.shape[0], x.device, shard)
        else:
            (y0, y1), stats = launch(None, None, False)[0], None
        ctx.save_for_backward(x, w0c, w1c)
        ctx.meta = (w0.dtype, None if b0 is None else b0.dtype, w1.dtype, None if b1 is None else b1.dtype)
        return y0, y1, stats

    @staticmethod
    def backward(ctx, g0, g1, _):
        x, w0c, w1c = ctx.saved_tensors
        wd0, bd0, wd1, bd1 = ctx.meta
        k = [x.shape[1]]
        dw0, db0 = _linear_param_grads(g0.contiguous(), [x], k, ctx.needs_input_grad[1],
                                       ctx.needs_input_grad[2] and bd0 is not None, wd0, bd0)
        dw1, db1 = _linear_param_grads(g1.contiguous(), [x], k, ctx.needs_input_grad[3],
                                       ctx.needs_input_grad[4] and bd1 is not None, wd1, bd1)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = K.gemm(g0.contiguous(), w0c)
            K.gemm(g1.contiguous(), w1c, out=dx, beta=1.0, addend=dx)
        return dx, dw0, db0, dw1, db1, None, None


class _StemPairBN(torch.autograd.Function):
    """(x0, x0, y1): x0 = relu(BatchNorm(x W0^T + b0)) — GraphConv's stem, large/ours.py:77-80 — handed out TWICE (the first
    SpMM and the layers' Linear / residual consume it; their gradients come back separately instead of through an add),
    y1 = x W1^T + b1 (TransConv's stem, :198) from the same read of x.  Backward: the BatchNorm's two sums over both
    gradients (sgf_bn_bwd_stats2), then dW0 / db0 straight from them — dz is formed inside the Gram kernel and never written
    (sgf_gram_bn_bwd): x is data, nobody else needs dz."""

    @staticmethod
    def forward(ctx, x, w0, b0, w1, b1, gamma, beta, book, shard, ln_gamma=None, ln_beta=None, ln_cfg=None, pack=None):
        """ln_cfg = (eps, relu, affine) — not None: the third output is [relu](LayerNorm(y1)) (TransConv's stem, large/ours.py:
        198-201) instead of y1, and its backward takes dW1 / db1 / d ln_gamma / d ln_beta from sgf_gram_ln_bwd.
        pack = {"slot_bytes": S} — not None: the BatchNorm pass also writes x0 in packed form for the SpMM that gathers it
        (K.bn_apply_packed), left in pack["out"]."""
        K.check(x)
        dt = x.dtype
        w0c, w1c = w0.to(dt), w1.to(dt)
        (y0, y1), mean, rstd, n_tot, training = _batchnorm_of(book, _stem_launch(x, w0c, w1c, [_f32c(b0), _f32c(b1)]),
                                                              w0.shape[0], x.shape[0], x.device, shard)
        g32, be32 = _f32c(gamma), _f32c(beta)
        if pack is not None:
            x0, pack["out"] = K.bn_apply_packed(y0, mean, rstd, g32, be32, None, True, pack["slot_bytes"])
        else:
            x0 = K.bn_apply(y0, mean, rstd, g32, be32, None, True)
        out1, ln_saved = y1, (None, None, None, None, None)
        if ln_cfg is not None:
            eps, ln_relu, affine = ln_cfg
            lg32, lb32 = (_f32c(ln_gamma), _f32c(ln_beta)) if affine else (None, None)
            out1, lmean, lrstd = K.ln_fwd(_rows(y1), None, 1.0, 0.0, lg32, lb32, bool(ln_relu), float(eps))
            ln_saved = (y1, lmean, lrstd, lg32, lb32)
        ctx.save_for_backward(x, w0c, w1c, y0, g32, be32, mean, rstd, *ln_saved)
        ctx.meta = (w0.dtype, None if b0 is None else b0.dtype, w1.dtype, None if b1 is None else b1.dtype,
                    None if gamma is None else gamma.dtype, bool(training), float(n_tot), shard,
                    None if ln_cfg is None else (bool(ln_cfg[1]), None if ln_gamma is None else ln_gamma.dtype))
        return x0, x0.view_as(x0), out1

    @staticmethod
    def backward(ctx, ga, gb, g1):
        x, w0c, w1c, y0, g32, be32, mean, rstd, y1, lmean, lrstd, lg32, lb32 = ctx.saved_tensors
        wd0, bd0, wd1, bd1, gdt, training, n_tot, shard, ln_meta = ctx.meta
        d = y0.shape[1]
        if ga is None:
            ga, gb = gb, None
        if ga is None:
            ga = torch.zeros_like(y0)
        ga = _rows(ga.contiguous())
        gb = None if gb is None else _rows(gb.contiguous())
        stats = K.bn_bwd_stats2(ga, gb, y0, mean, rstd, g32, be32, True)
        if shard is not None:
            shard.all_reduce(stats)
        inv_n = 1.0 / max(n_tot, 1.0)
        dw0, db0 = K.gram_bn_bwd(ga, gb, y0, mean, rstd, g32, be32, True, stats, inv_n, training, _rows(x))
        dw0 = dw0.to(wd0) if ctx.needs_input_grad[1] else None
        db0 = db0.to(bd0) if (ctx.needs_input_grad[2] and bd0 is not None) else None
        dlg = dlb = None
        if ln_meta is not None:
            # TransConv's stem: LayerNorm backward inside the Gram (dl never written); row-local, no collective
            ln_relu, lgdt = ln_meta
            dw1, db1, dlg, dlb = K.gram_ln_bwd(_rows(g1.contiguous()), y1, lmean, lrstd, lg32, lb32, ln_relu, _rows(x))
            dw1 = dw1.to(wd1) if ctx.needs_input_grad[3] else None
            db1 = db1.to(bd1) if (ctx.needs_input_grad[4] and bd1 is not None) else None
            dlg, dlb = (dlg.to(lgdt), dlb.to(lgdt)) if lg32 is not None else (None, None)
        else:
            dw1, db1 = _linear_param_grads(g1.contiguous(), [x], [x.shape[1]], ctx.needs_input_grad[3],
                                           ctx.needs_input_grad[4] and bd1 is not None, wd1, bd1)
        dgamma, dbeta = _bn_param_grads(stats, d, g32, be32, gdt, shard)
        dx = None
        if ctx.needs_input_grad[0]:                      # features that require a gradient (not in any recipe): explicit dz
            g = ga if gb is None else ga + gb
            dz = K.bn_bwd_apply(g, y0, mean, rstd, g32, be32, True, stats, inv_n, training)
            gl = g1
            if ln_meta is not None:
                gl = K.ln_bwd(_rows(g1.contiguous()), None, y1, None, 1.0, 0.0, lg32, False, lmean, lrstd)[0] \
                    if not ln_meta[0] else None
                if gl is None:
                    raise NotImplementedError("features that require a gradient behind the fused LayerNorm stem: set "
                                              "SGF_STEM_LN_FUSED=0")
            dx = K.gemm(dz, w0c)
            K.gemm(gl.contiguous(), w1c, out=dx, beta=1.0, addend=dx)
        return dx, dw0, db0, dw1, db1, dgamma, dbeta, None, None, dlg, dlb, None, None


def stem_pair_bn_supported(x, w0, w1) -> bool:
    return stem_pair_supported(x, w0, w1) and _has(K, "gram_bn_bwd_supported", w0.shape[0], x.shape[1], x.dtype)


def stem_pair_bn(x, w0, b0, w1, b1, gamma, beta, book, shard=None, ln=None, pack=None):
    """(x0 for the layers, x0 for the first SpMM, y1): see _StemPairBN.  book: the BatchNorm's bookkeeping (ours._BNBook).
    ln = (LayerNorm weight, bias, eps, relu): the third output is [relu](LayerNorm(y1)) — TransConv's stem — when the shapes
    allow (stem_ln_supported).  pack: see _StemPairBN."""
    if ln is None:
        return _StemPairBN.apply(x, w0, b0, w1, b1, gamma, beta, book, shard, None, None, None, pack)
    lg, lb, eps, relu = ln
    return _StemPairBN.apply(x, w0, b0, w1, b1, gamma, beta, book, shard, lg, lb, (eps, relu, lg is not None), pack)


def stem_ln_supported(x, w1) -> bool:
    return (_has(K, "gram_ln_bwd_supported", w1.shape[0], x.shape[1], x.dtype) and not x.requires_grad
            and _switch("SGF_STEM_LN_FUSED", True))


def stem_pair_supported(x, w0, w1) -> bool:
    return (x.dim() == 2 and x.shape[0] > 0 and w0.shape == w1.shape and x.stride(-1) == 1
            and (x.stride(0) * x.element_size()) % 8 == 0 and x.data_ptr() % 8 == 0
            and K.stem_pair_supported(x.shape[1], w0.shape[0], x.dtype))


def stem_pair(x, w0, b0, w1, b1, want_stats0=False, shard=None):
    """((y0, y1), stats0): both input stems from one read of x; stats0 = (mean, var, count) of y0 for its BatchNorm
    when asked for, else None."""
    y0, y1, stats = _StemPair.apply(x, w0, b0, w1, b1, bool(want_stats0), shard)
    return (y0, y1), (None if stats is None else stats.moments())


def _streaming_linear_ok(x: torch.Tensor, wc: torch.Tensor, dx: bool = False) -> bool:
    """x wc^T (or, dx=True, x wc) on the streaming kernels: bf16 square layers, fp32 layers of widths % 4 up to 256."""
    return (x.dim() == 2 and x.shape[0] > 0 and wc.stride(-1) == 1 and (wc.stride(0) * wc.element_size()) % 16 == 0
            and wc.data_ptr() % 16 == 0 and x.shape[1] == (wc.shape[0] if dx else wc.shape[1])
            and K.gcn_epilogue_supported(wc.shape[1], wc.shape[0], x.dtype))


def _streaming_linear(xr, wc, b32, rows=None, shift=None, want_stats=False):
    """([x_1 | x_2] wc^T + b32 on the first `rows` rows (all by default), its sums about `shift` if wanted): one or two
    streaming passes — a `launch` of _shifted_sums once the operands are bound."""
    xs = xr if rows is None else [x[:rows] for x in xr]
    if len(xs) == 1:
        return K.gcn_epilogue_stats(xs[0], wc, b32, shift, want_stats=want_stats)
    return K.gcn_epilogue_cat(xs[0], xs[1], wc, b32, shift, want_stats=want_stats)


def _linear_with_stats(xr, wc, b32, shard):
    """(y, BNSums of y): y = [x_1 | x_2] wc^T + b32 and the sums BatchNorm needs of it, from the same pass."""
    return _shifted_sums(partial(_streaming_linear, xr, wc, b32), wc.shape[0], xr[0].shape[0], xr[0].device, shard)


# ------------------------------------------------------------------------------------------------
# T4 + T6 as ONE autograd node: out = [relu](BatchNorm(W [y | x0] + b)) [+ x0]   (large/ours.py:36-40, 87-93)
# ------------------------------------------------------------------------------------------------
class GradChain:
    """The gradient of x0 = layer_[0] of one GraphConv forward, collected across its layers' backward nodes (which run in
    reverse layer order: layer i's input is layer i-1's output) and returned to autograd ONCE, by the first layer's node —
    the last to run; the others return nothing for x0.  Two forms:
      * fused kernel (SGF_GCN_BWD_FUSED=1): every layer's sgf_gcn_bn_bwd_dx adds its two contributions (the residual's gy
        and dz W[:, d:]) to the running sum it is handed (`acc`, opaque);
      * default: the contributions are kept (`parts`) and summed in one pass (sgf_sum_n) by the first layer's node."""

    def __init__(self):
        self.acc = None
        self.parts = []


def _fused_bwd() -> bool:
    """sgf_gcn_bn_bwd_dx in the layers' backward.  Off by default: at d = 256 the four workgroups per row tile do not stay
    inside the L2's window on their own (gy / z leave HBM four times) and with the per-tile rendezvous the launch is bound
    by its own serial phases — 2.4-4.4 ms against 2.1 ms for the separate kernels (profiles/r04_bn_bwd_dx_*.md)."""
    return _switch("SGF_GCN_BWD_FUSED", False)


def _acc_in_place(d: int, dtype) -> bool:
    """sgf_gcn_epilogue_dx2_acc in the layers' backward (default on; SGF_GCN_DX_ACC=0: paired dx2 + one sgf_sum_n)."""
    return _has(K, "gcn_epilogue_dx2_acc_supported", d, dtype) and _switch("SGF_GCN_DX_ACC", True)


def gcn_layer_fused_ok(x0: torch.Tensor, w: torch.Tensor) -> bool:
    """bf16 storage, square blocks of 64 / 128 / 256, W = [W1 | W2] — what sgf_gcn_bn_bwd_dx / sgf_gcn_epilogue_cat take."""
    d = x0.shape[1] if x0.dim() == 2 else 0
    return (x0.dim() == 2 and x0.shape[0] > 0 and x0.dtype == _BF16 and tuple(w.shape) == (d, 2 * d)
            and _has(K, "gcn_bn_bwd_dx_supported", d, x0.dtype) and _switch("SGF_GCN_FUSED", True))


class _LinearBNActRes(torch.autograd.Function):
    """y = A x (already multiplied), x0 -> z = [y | x0] W^T + b -> out = [relu](BatchNorm(z)) [+ x0].

    Forward: one pass for the Linear and BatchNorm's batch sums (sgf_gcn_epilogue_cat), `book` — the module's own
    bookkeeping (ours._BNBook: batch vs running statistics, running-stat update) — then sgf_bn_apply.
    Backward: sgf_bn_bwd_stats (the one global reduction), then ONE launch for dz, d y and the running gradient of x0
    (sgf_gcn_bn_bwd_dx), then the weight / bias gradients on sgf_gram."""

    @staticmethod
    def forward(ctx, y, x0, w, b, gamma, beta, book, relu: bool, use_res: bool, shard, chain, first: bool, pack=None):
        # pack = {"slot_bytes": S}: the BatchNorm pass also writes `out` in packed form for the next SpMM (pack["out"])
        K.check(y, x0)
        dt = x0.dtype
        wc = w.detach().to(dt).contiguous()
        yr, xr = _rows16(y), _rows16(x0)
        z, mean, rstd, n_tot, training = _batchnorm_of(book, partial(_streaming_linear, [yr, xr], wc, _f32c(b)), wc.shape[0],
                                                       yr.shape[0], yr.device, shard)
        g32, be32 = _f32c(gamma), _f32c(beta)
        if pack is not None:
            out, pack["out"] = K.bn_apply_packed(z, mean, rstd, g32, be32, xr if use_res else None, relu, pack["slot_bytes"])
        else:
            out = K.bn_apply(z, mean, rstd, g32, be32, xr if use_res else None, relu)
        ctx.save_for_backward(yr, xr, z, wc, g32, be32, mean, rstd)
        ctx.meta = (bool(relu), bool(use_res), bool(training), float(n_tot), shard, chain, bool(first), w.dtype,
                    None if b is None else b.dtype, None if gamma is None else gamma.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        yr, xr, z, wc, g32, be32, mean, rstd = ctx.saved_tensors
        relu, use_res, training, n_tot, shard, chain, first, wdt, bdt, gdt = ctx.meta
        d = z.shape[1]
        gout = _rows16(gout.contiguous())
        stats = K.bn_bwd_stats(gout, z, mean, rstd, g32, be32, relu)
        if shard is not None:
            shard.all_reduce(stats)
        inv_n = 1.0 / max(n_tot, 1.0)
        if _fused_bwd():
            dz, dy, acc = K.gcn_bn_bwd_dx(gout, z, mean, rstd, g32, be32, relu, stats, inv_n, training, wc, chain.acc,
                                          last=first, add_gy=use_res)
            chain.acc = None if first else acc
            dx0 = acc if first else None
        else:
            # BatchNorm backward, then BOTH input gradients from one HBM read of dz (paired launch); x0's contributions wait
            # in the chain for the one summation pass
            fused_dw = None
            if ctx.needs_input_grad[2] and _pair_gram() and _has(K, "gram2_bn_bwd_supported", gout, z, yr, xr):
                # dz, dW = dz^T [y | x0] and db from ONE pass over (gout, z): sgf_gram2_bn_bwd (csrc/gramx.hip, k_gramb2)
                dwf = torch.empty((d, 2 * d), dtype=_F32, device=z.device)
                dz, dbf = K.gram2_bn_bwd(gout, z, mean, rstd, g32, be32, relu, stats, inv_n, training, yr, xr, dwf[:, :d], dwf[:, d:])
                fused_dw = (dwf.to(wdt), dbf.to(bdt) if (ctx.needs_input_grad[3] and bdt is not None) else None)
            else:
                dz = K.bn_bwd_apply(gout, z, mean, rstd, g32, be32, relu, stats, inv_n, training)
            if _acc_in_place(d, dz.dtype) and not chain.parts:
                # x0's gradient accumulated IN PLACE: this layer's dz W2 and residual gradient join the running sum inside
                # the launch that produces dy (balanced pair of workgroups at d = 256) — no k-operand summation pass at the end
                dy, chain.acc = K.gcn_epilogue_dx2_acc(dz, wc, _rows16(gout) if use_res else None, chain.acc)
                dx0 = None
                if first:
                    dx0, chain.acc = chain.acc, None
            else:
                dy, dxi = K.gcn_epilogue_dx2(dz, wc[:, :d], wc[:, d:], True)
                chain.parts.append(dxi)
                if use_res:
                    chain.parts.append(gout)
                dx0 = None
                if first:
                    parts, chain.parts = chain.parts, []
                    if chain.acc is not None:
                        parts.append(chain.acc)
                        chain.acc = None
                    dx0 = parts[0] if len(parts) == 1 else (K.sum_n(parts) if len(parts) <= 8 else sum(parts[1:], parts[0]))
        if not _fused_bwd() and fused_dw is not None:
            dw, db = fused_dw
        else:
            dw, db = _linear_param_grads(dz, [yr, xr], [d, d], ctx.needs_input_grad[2],
                                         ctx.needs_input_grad[3] and bdt is not None, wdt, bdt)
        dgamma, dbeta = _bn_param_grads(stats, d, g32, be32, gdt, shard)
        return dy, dx0, dw, db, dgamma, dbeta, None, None, None, None, None, None, None


def linear_bn_act_res(y, x0, w, b, gamma, beta, book, relu, use_res, shard, chain, first, pack=None):
    return _LinearBNActRes.apply(y, x0, w, b, gamma, beta, book, relu, use_res, shard, chain, first, pack)


def _linear(w, b, *xs):
    return _Linear.apply(w, b, False, None, *xs)[0]


def linear(x, w, b):
    """nn.Linear: square bf16 layers / fp32 layers up to 256 wide on the streaming row kernels (sgf_gcn_epilogue_stats / _dx),
    every other shape on sgf_gemm; weight / bias gradients on sgf_gram."""
    return _linear(w, b, x)


def linear_bn_stats(xs, w, b, shard=None):
    """(y, (mean, var, n_tot)): nn.Linear of x (or of [x_1 | x_2] for a tuple, GraphConvLayer's use_init) and the
    batch statistics BatchNorm1d needs of its output (large/ours.py:36-40 followed by :87-88) — from the Linear's own
    pass when its blocks are square bf16, else linear + batch_stats."""
    y, stats = _Linear.apply(w, b, True, shard, *(xs if isinstance(xs, (tuple, list)) else (xs,)))
    return y, stats.moments()


def linear_cat(xs, w, b):
    """[x_1 | x_2 | ...] W^T + b without the concatenation (GraphConvLayer with use_init)."""
    return _linear(w, b, *xs)


def _pad_out_rows(w, b, q: int):
    """(W, b) with zero rows up to the next multiple of q classes: the caller slices the result, autograd the gradients."""
    pad = -w.shape[0] % q
    return F.pad(w, (0, 0, 0, pad)), None if b is None else F.pad(b, (0, pad))


def out_linear_cat(xs, w, b):
    """The output head of aggregate='cat' (large/ours.py:271-275: fc(cat(x1, x2))) WITHOUT the [N, 2 d] concatenation:
    W = [W_1 | W_2] applied operand by operand (fp32 storage: two passes on the exact-fp32 matrix cores, the first product
    parked as an [N, C] fp32 partial — small next to the [N, d] operands; bf16: GEMM + GEMM(beta = 1)).  Class counts that
    are not multiples of 4 are padded with zero rows for the fp32 kernel, as in out_linear."""
    m = w.shape[0]
    if (xs[0].dtype == _F32 and xs[0].is_cuda and m % 4 != 0
            and all(K.gcn_epilogue_supported(x.shape[1], (m + 3) // 4 * 4, _F32) for x in xs)):
        return _linear(*_pad_out_rows(w, b, 4), *xs)[:, :m]
    return _linear(w, b, *xs)


def out_linear(x, w, b):
    """The output head (large/ours.py:275).  fp32 storage and a class count that is not a multiple of 4 (C = 47): W and b
    are padded with zero rows to the next multiple and the result sliced, so that the layer still runs on the streaming
    fp32 kernel (csrc/linear_f32.hip) instead of a library GEMM; autograd slices the gradients back."""
    m = w.shape[0]
    if (x.dtype == _F32 and x.is_cuda and x.dim() == 2 and m % 4 != 0
            and K.gcn_epilogue_supported(w.shape[1], (m + 3) // 4 * 4, _F32)):
        return _linear(*_pad_out_rows(w, b, 4), x)[:, :m]
    if x.dtype == _BF16 and x.dim() == 2 and m % 8 != 0 and not K.gcn_epilogue_supported(w.shape[1], m, _BF16):
        # bf16 storage and a class count whose rows would not be 16-byte aligned (the 100M recipe: C = 172 -> 344-byte rows):
        # W / b padded with zero rows to the next multiple of 8, so that sgf_gemm stages the logits' gradient with 16-byte
        # loads in the backward (dx = g W) as it stages x in the forward; the result is sliced, autograd slices back
        return _linear(*_pad_out_rows(w, b, 8), x)[:, :m]
    return _linear(w, b, x)
