"""DIFFormer's all-pair sigmoid attention (medium/difformer.py:41-52) on the tiled kernels of csrc/pair_attn.hip (include/sgf.h
block N7): no [n, l, H] score tensor, in the forward or under autograd.

    sigmoid_attention(q [n, H, D], k [l, H, D], v [l, Hv, D]) -> [n, H, D]      Hv = H, or 1 (use_weight=False)
        out_i = sum_j sigmoid(q_i . k_j) v_j / sum_j sigmoid(q_i . k_j), per head

One forward launch; the backward is two launches that both recompute the scores (dq with the query tile resident, dk / dv
with the key tile resident), so every gradient is a fixed-order sum: bit-reproducible, no atomics.  Saved for the backward:
q, k, v, out and the fp32 row sums [n, H].

`supported(q, k, v)` says whether the kernels take the call (D in {32, 64, 128}, H <= 8, fp32 or bf16, l > 0); what they do
not take stays on difformer._dense_attention.  `use_kernels(q, k, v)` adds the switch SGF_PAIR_ATTN: 0 = always the dense
path, 1 = the kernels wherever supported, unset = the kernels from PAIR_MIN_PAIRS (fp32) / PAIR_MIN_PAIRS_BF16 score
entries (n l H) upward.

The exact softmax attention of medium/ablation/oursSOFT.py runs on the same skeleton with an online maximum (include/sgf.h
block N8):

    softmax_attention(q [n, H, D], k [l, H, D], v [l, Hv, D], scale=1.0) -> [n, H, D]
        out_i = sum_j softmax_j(scale q_i . k_j) v_j, per head

Saved for the backward: q, k, v, out and the fp32 log-sum-exp [n, H].  `softmax_supported` / `use_softmax_kernels` are the
counterparts of `supported` / `use_kernels` under the switch SGF_PAIR_SOFTMAX and the thresholds SOFTMAX_MIN_PAIRS /
SOFTMAX_MIN_PAIRS_BF16; what the kernels do not take stays on ours_soft._dense_attention.
"""
from __future__ import annotations

import os

import torch

from . import _lib, ops
from .kernels import _code, _launch
from .linear import _switch

__all__ = ["sigmoid_attention", "supported", "use_kernels", "PAIR_MIN_PAIRS",
           "softmax_attention", "softmax_supported", "use_softmax_kernels", "SOFTMAX_MIN_PAIRS", "SOFTMAX_MIN_PAIRS_BF16"]

_F32 = torch.float32
_BF16 = torch.bfloat16

# Score entries n * l * H from which the kernels run when SGF_PAIR_ATTN is unset, per storage dtype: the smallest probed size
# from which they were ahead of the dense path beyond the spread of the repetitions, forward and forward + backward, at every
# probed head count (profiles/pair_attn_probe.md says how it follows from the table).  0: ahead at every probed size.
PAIR_MIN_PAIRS = 19717 * 19717 * 4      # fp32 storage: the exact fp32 matrix cores against a library GEMM that keeps its scores
PAIR_MIN_PAIRS_BF16 = 0                 # bf16 storage

# The same rule for the softmax kernels under SGF_PAIR_SOFTMAX (profiles/pair_softmax_probe.md; widths 32 / 64 / 128 and 1 / 2 / 4
# heads were probed).  With one head the dense path is two plain GEMMs around a softmax and stays ahead in time up to the largest
# probed size (while holding gigabytes of scores): the smallest size from which every probed cell is ahead is 40 000 nodes x 2 heads.
SOFTMAX_MIN_PAIRS = 40000 * 40000 * 2        # fp32 storage
SOFTMAX_MIN_PAIRS_BF16 = 40000 * 40000 * 2   # bf16 storage


# ------------------------------------------------------------------------------------------------
# the entries on the current stream (private: the kernel table of kernels.py is not extended)
# ------------------------------------------------------------------------------------------------
class _Hip:
    @staticmethod
    def pair_sigmoid_supported(heads: int, v_heads: int, d: int, dtype) -> bool:
        if dtype not in (_F32, _BF16):
            return False
        return bool(_lib.load().sgf_pair_sigmoid_supported(int(heads), int(v_heads), int(d),
                                                           _lib.SGF_BF16 if dtype == _BF16 else _lib.SGF_F32))

    @staticmethod
    def pair_sigmoid_fwd(q, k, v):
        """(out [n, H, D] in the storage dtype, rowsum fp32 [n, H])"""
        dev, (n, h, d), l, hv = q.device, q.shape, k.shape[0], v.shape[1]
        out = torch.empty((n, h, d), dtype=q.dtype, device=dev)
        rowsum = torch.empty((n, h), dtype=_F32, device=dev)
        _launch(dev, "sgf_pair_sigmoid_fwd", q, q.stride(0), k, k.stride(0), v, v.stride(0), n, l, h, hv, d, _code(q), out,
                h * d, rowsum)
        return out, rowsum

    @staticmethod
    def pair_sigmoid_bwd_q(g, out, rowsum, q, k, v, want_dq: bool = True):
        """(dq [n, H, D] or None, delta fp32 [n, H] = g . out per row and head: the operand of pair_sigmoid_bwd_kv)"""
        dev, (n, h, d), l, hv = q.device, q.shape, k.shape[0], v.shape[1]
        dq = torch.empty((n, h, d), dtype=q.dtype, device=dev) if want_dq else None
        delta = torch.empty((n, h), dtype=_F32, device=dev)
        _launch(dev, "sgf_pair_sigmoid_bwd_q", g, g.stride(0), out, out.stride(0), rowsum, q, q.stride(0), k, k.stride(0), v,
                v.stride(0), n, l, h, hv, d, _code(q), dq, h * d, delta, delta.numel() * 4)
        return dq, delta

    @staticmethod
    def pair_sigmoid_bwd_kv(g, rowsum, delta, q, k, v):
        """(dk [l, H, D], dv [l, Hv, D]; Hv = 1: dv summed over the heads)"""
        dev, (n, h, d), l, hv = q.device, q.shape, k.shape[0], v.shape[1]
        dk = torch.empty((l, h, d), dtype=q.dtype, device=dev)
        dv = torch.empty((l, hv, d), dtype=q.dtype, device=dev)
        _launch(dev, "sgf_pair_sigmoid_bwd_kv", g, g.stride(0), rowsum, q, q.stride(0), k, k.stride(0), v, v.stride(0), n, l,
                h, hv, d, _code(q), dk, h * d, dv, hv * d, delta, delta.numel() * 4)
        return dk, dv

    @staticmethod
    def pair_softmax_supported(heads: int, v_heads: int, d: int, dtype) -> bool:
        if dtype not in (_F32, _BF16):
            return False
        return bool(_lib.load().sgf_pair_softmax_supported(int(heads), int(v_heads), int(d),
                                                           _lib.SGF_BF16 if dtype == _BF16 else _lib.SGF_F32))

    @staticmethod
    def pair_softmax_fwd(q, k, v, scale: float = 1.0):
        """(out [n, H, D] in the storage dtype, lse fp32 [n, H])"""
        dev, (n, h, d), l, hv = q.device, q.shape, k.shape[0], v.shape[1]
        out = torch.empty((n, h, d), dtype=q.dtype, device=dev)
        lse = torch.empty((n, h), dtype=_F32, device=dev)
        _launch(dev, "sgf_pair_softmax_fwd", q, q.stride(0), k, k.stride(0), v, v.stride(0), n, l, h, hv, d, _code(q),
                float(scale), out, h * d, lse)
        return out, lse

    @staticmethod
    def pair_softmax_bwd_q(g, out, lse, q, k, v, scale: float = 1.0, want_dq: bool = True):
        """(dq [n, H, D] or None, delta fp32 [n, H] = g . out per row and head: the operand of pair_softmax_bwd_kv)"""
        dev, (n, h, d), l, hv = q.device, q.shape, k.shape[0], v.shape[1]
        dq = torch.empty((n, h, d), dtype=q.dtype, device=dev) if want_dq else None
        delta = torch.empty((n, h), dtype=_F32, device=dev)
        _launch(dev, "sgf_pair_softmax_bwd_q", g, g.stride(0), out, out.stride(0), lse, q, q.stride(0), k, k.stride(0), v,
                v.stride(0), n, l, h, hv, d, _code(q), float(scale), dq, h * d, delta, delta.numel() * 4)
        return dq, delta

    @staticmethod
    def pair_softmax_bwd_kv(g, lse, delta, q, k, v, scale: float = 1.0):
        """(dk [l, H, D], dv [l, Hv, D]; Hv = 1: dv summed over the heads)"""
        dev, (n, h, d), l, hv = q.device, q.shape, k.shape[0], v.shape[1]
        dk = torch.empty((l, h, d), dtype=q.dtype, device=dev)
        dv = torch.empty((l, hv, d), dtype=q.dtype, device=dev)
        _launch(dev, "sgf_pair_softmax_bwd_kv", g, g.stride(0), lse, q, q.stride(0), k, k.stride(0), v, v.stride(0), n, l,
                h, hv, d, _code(q), float(scale), dk, h * d, dv, hv * d, delta, delta.numel() * 4)
        return dk, dv


def _table(entry: str = "pair_sigmoid_fwd"):
    """Where pair_sigmoid_supported / _fwd / _bwd_q / _bwd_kv (or the pair_softmax_* family, told by `entry`) live: a test's
    CPU table that has them, the entries above on the HIP table, nothing otherwise (every call then takes the dense path)."""
    k = ops.K
    if hasattr(k, entry):
        return k
    return _Hip if k.name == "hip" else None


# ------------------------------------------------------------------------------------------------
# which calls the kernels take
# ------------------------------------------------------------------------------------------------
def supported(q, k, v) -> bool:
    """q [n, H, D], k [l, H, D], v [l, H | 1, D]: tensors of one dtype on the GPU, contiguous in the last dimension, in a
    shape the library accepts, with at least one query and one key, and a kernel table that has the entries."""
    return _supported(q, k, v, "pair_sigmoid")


def _supported(q, k, v, family: str) -> bool:
    t = _table(family + "_fwd")
    if t is None or not all(torch.is_tensor(x) and x.dim() == 3 for x in (q, k, v)):
        return False
    if t is _Hip and not (q.is_cuda and k.is_cuda and v.is_cuda):
        return False
    if not (q.dtype == k.dtype == v.dtype and q.device == k.device == v.device):
        return False
    if any(x.stride(2) != 1 for x in (q, k, v)):
        return False
    (n, h, d), l, hv = q.shape, k.shape[0], v.shape[1]
    if k.shape[1:] != (h, d) or v.shape[0] != l or v.shape[2] != d or n < 1 or l < 1 or max(n, l) >= 2 ** 31:
        return False
    return bool(getattr(t, family + "_supported")(h, hv, d, q.dtype))


def use_kernels(q, k, v) -> bool:
    """supported(q, k, v) under the switch SGF_PAIR_ATTN (read on every call)."""
    s = os.environ.get("SGF_PAIR_ATTN")
    if s is not None and not _switch("SGF_PAIR_ATTN", True):
        return False
    if not supported(q, k, v):
        return False
    return s is not None or q.shape[0] * k.shape[0] * q.shape[1] >= (PAIR_MIN_PAIRS_BF16 if q.dtype == _BF16 else PAIR_MIN_PAIRS)


def _rows(t: torch.Tensor) -> torch.Tensor:
    """[rows, heads, D] with the heads side by side in 16-byte aligned rows: the [rows, heads * D] operand of the entries."""
    if (t.stride(2) != 1 or t.stride(1) != t.shape[2] or (t.stride(0) * t.element_size()) % 16 != 0
            or t.stride(0) < t.shape[1] * t.shape[2] or t.data_ptr() % 16 != 0):
        t = t.contiguous()
    return t


class _SigmoidAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v):
        ops.K.check(q, k, v)
        t = _table()
        q, k, v = _rows(q), _rows(k), _rows(v)
        out, rowsum = t.pair_sigmoid_fwd(q, k, v)
        ctx.save_for_backward(q, k, v, out, rowsum)
        ctx.table = t
        return out

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():          # (only under create_graph=True)
            raise RuntimeError("sgformer_amd: pair_attn.sigmoid_attention is once differentiable; backward with "
                               "create_graph=True is not implemented (SGF_PAIR_ATTN=0 keeps the twice differentiable path)")
        q, k, v, out, rowsum = ctx.saved_tensors
        t = ctx.table
        need_q, need_k, need_v = ctx.needs_input_grad
        if not (need_q or need_k or need_v):
            return None, None, None
        g = _rows(g if g.dtype == q.dtype else g.to(q.dtype))
        dq, delta = t.pair_sigmoid_bwd_q(g, out, rowsum, q, k, v, want_dq=need_q)      # (delta is bwd_kv's operand too)
        dk = dv = None
        if need_k or need_v:
            dk, dv = t.pair_sigmoid_bwd_kv(g, rowsum, delta, q, k, v)
        return dq, (dk if need_k else None), (dv if need_v else None)


def sigmoid_attention(q, k, v) -> torch.Tensor:
    """out [n, H, D] of the sigmoid kernel for q [n, H, D], k [l, H, D], v [l, H | 1, D]; differentiable once in q, k and v.
    The caller asks supported() / use_kernels() first: an unsupported call is an error here, not a fallback."""
    if not supported(q, k, v):
        raise RuntimeError(f"pair_attn.sigmoid_attention: unsupported operands q {tuple(q.shape)} {q.dtype}, k {tuple(k.shape)}, "
                           f"v {tuple(v.shape)} (D in {{32, 64, 128}}, H <= 8, float32 or bfloat16, one device)")
    return _SigmoidAttention.apply(q, k, v)


# ------------------------------------------------------------------------------------------------
# the exact softmax attention
# ------------------------------------------------------------------------------------------------
def softmax_supported(q, k, v) -> bool:
    """supported() for the softmax kernels: the same operand rules, and a kernel table that has the pair_softmax_* entries."""
    return _supported(q, k, v, "pair_softmax")


def use_softmax_kernels(q, k, v) -> bool:
    """softmax_supported(q, k, v) under the switch SGF_PAIR_SOFTMAX (read on every call): 0 = always the dense path, 1 = the
    kernels wherever supported, unset = the kernels from SOFTMAX_MIN_PAIRS / SOFTMAX_MIN_PAIRS_BF16 score entries upward."""
    s = os.environ.get("SGF_PAIR_SOFTMAX")
    if s is not None and not _switch("SGF_PAIR_SOFTMAX", True):
        return False
    if not softmax_supported(q, k, v):
        return False
    return s is not None or q.shape[0] * k.shape[0] * q.shape[1] >= (SOFTMAX_MIN_PAIRS_BF16 if q.dtype == _BF16
                                                                      else SOFTMAX_MIN_PAIRS)


class _SoftmaxAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale):
        ops.K.check(q, k, v)
        t = _table("pair_softmax_fwd")
        q, k, v = _rows(q), _rows(k), _rows(v)
        out, lse = t.pair_softmax_fwd(q, k, v, scale)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.table, ctx.scale = t, scale
        return out

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():          # (only under create_graph=True)
            raise RuntimeError("sgformer_amd: pair_attn.softmax_attention is once differentiable; backward with "
                               "create_graph=True is not implemented (SGF_PAIR_SOFTMAX=0 keeps the twice differentiable path)")
        q, k, v, out, lse = ctx.saved_tensors
        t, scale = ctx.table, ctx.scale
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        if not (need_q or need_k or need_v):
            return None, None, None, None
        g = _rows(g if g.dtype == q.dtype else g.to(q.dtype))
        dq, delta = t.pair_softmax_bwd_q(g, out, lse, q, k, v, scale, want_dq=need_q)      # (delta is bwd_kv's operand too)
        dk = dv = None
        if need_k or need_v:
            dk, dv = t.pair_softmax_bwd_kv(g, lse, delta, q, k, v, scale)
        return dq, (dk if need_k else None), (dv if need_v else None), None


def softmax_attention(q, k, v, scale: float = 1.0) -> torch.Tensor:
    """out [n, H, D] = softmax over the keys of scale q . k, times v, for q [n, H, D], k [l, H, D], v [l, H | 1, D];
    differentiable once in q, k and v (scale is a constant: a finite, positive float).  The caller asks softmax_supported() /
    use_softmax_kernels() first: an unsupported call is an error here, not a fallback."""
    if not softmax_supported(q, k, v):
        raise RuntimeError(f"pair_attn.softmax_attention: unsupported operands q {tuple(q.shape)} {q.dtype}, k {tuple(k.shape)}, "
                           f"v {tuple(v.shape)} (D in {{32, 64, 128}}, H <= 8, float32 or bfloat16, one device)")
    scale = float(scale)
    if not (0.0 < scale < float("inf")):
        raise ValueError(f"pair_attn.softmax_attention: scale must be finite and positive, got {scale}")
    return _SoftmaxAttention.apply(q, k, v, scale)
