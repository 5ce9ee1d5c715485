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

fp32 tensors under torch.set_float32_matmul_precision('high') run the split-bf16 kernels (the sgf_pair_*_x3_* entries of
block N9, dtype code SGF_F32_BF16X3: every matrix product as three bf16 matrix-core products, everything else in fp32)
wherever sgf_pair_*_x3_supported takes the shape, chosen at each launch as kernels._mm_code chooses for every other
product; 'highest' and bf16 tensors run what they always ran.  Their thresholds are PAIR_MIN_PAIRS_X3 / SOFTMAX_MIN_PAIRS_X3.

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

from . import _lib, kernels, ops
from .kernels import _launch
from .linear import _switch

__all__ = ["sigmoid_attention", "supported", "use_kernels", "PAIR_MIN_PAIRS", "PAIR_MIN_PAIRS_X3",
           "softmax_attention", "softmax_supported", "use_softmax_kernels", "SOFTMAX_MIN_PAIRS", "SOFTMAX_MIN_PAIRS_BF16",
           "SOFTMAX_MIN_PAIRS_X3"]

_F32 = torch.float32
_BF16 = torch.bfloat16

# Score entries n * l * H from which the kernels run when SGF_PAIR_ATTN is unset, per storage dtype: the smallest probed size
# from which they were ahead of the dense path beyond the spread of the repetitions, forward and forward + backward, at every
# probed head count (profiles/pair_attn_probe.md says how it follows from the table).  0: ahead at every probed size.
PAIR_MIN_PAIRS = 19717 * 19717 * 4      # fp32 storage: the exact fp32 matrix cores against a library GEMM that keeps its scores
PAIR_MIN_PAIRS_BF16 = 0                 # bf16 storage
# fp32 storage when the split-bf16 kernels would run ('high'), against the dense path under the same setting, whose library GEMMs
# gain from it too (profiles/pair_x3_probe.md): the kernels are 1.3 - 1.8 x the exact ones, and the last probed cell that is not
# ahead beyond the spread is 40 000 nodes x 1 head at D = 128 (forward + backward level with the dense path).
PAIR_MIN_PAIRS_X3 = 40000 * 40000 * 2

# The same rule for the softmax kernels under SGF_PAIR_SOFTMAX (profiles/pair_softmax_probe.md; widths 32 / 64 / 128 and 1 / 2 / 4
# heads were probed).  With one head the dense path is two plain GEMMs around a softmax and stays ahead in time up to the largest
# probed size (while holding gigabytes of scores): the smallest size from which every probed cell is ahead is 40 000 nodes x 2 heads.
SOFTMAX_MIN_PAIRS = 40000 * 40000 * 2        # fp32 storage
SOFTMAX_MIN_PAIRS_BF16 = 40000 * 40000 * 2   # bf16 storage
SOFTMAX_MIN_PAIRS_X3 = 40000 * 40000 * 2     # fp32 storage on the split-bf16 kernels under 'high' (profiles/pair_x3_probe.md)


# The two arms.  An arm is told by its entry family ("pair_sigmoid" / "pair_softmax": the prefix of the sgf_* entries and of the
# kernel table's methods); here is what else differs: the public function's name, its switch and its three thresholds (module
# attributes, looked up by name on every call: fp32, bf16, fp32 on the split-bf16 kernels).
_ARMS = {"pair_sigmoid": ("sigmoid_attention", "SGF_PAIR_ATTN", "PAIR_MIN_PAIRS", "PAIR_MIN_PAIRS_BF16", "PAIR_MIN_PAIRS_X3"),
         "pair_softmax": ("softmax_attention", "SGF_PAIR_SOFTMAX", "SOFTMAX_MIN_PAIRS", "SOFTMAX_MIN_PAIRS_BF16",
                          "SOFTMAX_MIN_PAIRS_X3")}


# ------------------------------------------------------------------------------------------------
# the entries on the current stream (private: the kernel table of kernels.py is not extended)
# ------------------------------------------------------------------------------------------------
def _hip_supported(family: str, heads: int, v_heads: int, d: int, dtype) -> bool:
    if dtype not in (_F32, _BF16):
        return False
    return bool(getattr(_lib.load(), f"sgf_{family}_supported")(int(heads), int(v_heads), int(d),
                                                                _lib.SGF_BF16 if dtype == _BF16 else _lib.SGF_F32))


def _entry(family: str, launch: str, q, hv: int):
    """(entry name, dtype code) of one launch, decided when it is made: fp32 operands under 'high' go to the split-bf16
    family with SGF_F32_BF16X3 where sgf_<family>_x3_supported takes the shape; everything else is the exact family with the
    storage code."""
    code = kernels._mm_code(q, f"sgf_{family}_x3_supported", q.shape[1], hv, q.shape[2])
    if code == _lib.SGF_F32_BF16X3:
        return f"sgf_{family}_x3_{launch}", code
    return f"sgf_{family}_{launch}", code


def _x3_would_run(family: str, q, v) -> bool:
    return q.dtype == _F32 and _entry(family, "fwd", q, v.shape[1])[1] == _lib.SGF_F32_BF16X3


# `scale`: () for the sigmoid entries, (scale,) for the softmax entries, whose argument lists have it after the dtype code
def _hip_fwd(family: str, scale: tuple, q, k, v):
    dev, (n, h, d), l, hv = q.device, q.shape, k.shape[0], v.shape[1]
    out = torch.empty((n, h, d), dtype=q.dtype, device=dev)
    saved = torch.empty((n, h), dtype=_F32, device=dev)
    entry, code = _entry(family, "fwd", q, hv)
    _launch(dev, entry, q, q.stride(0), k, k.stride(0), v, v.stride(0), n, l, h, hv, d, code, *scale, out, h * d, saved)
    return out, saved


def _hip_bwd_q(family: str, scale: tuple, g, out, saved, q, k, v, want_dq: bool):
    dev, (n, h, d), l, hv = q.device, q.shape, k.shape[0], v.shape[1]
    dq = torch.empty((n, h, d), dtype=q.dtype, device=dev) if want_dq else None
    delta = torch.empty((n, h), dtype=_F32, device=dev)
    entry, code = _entry(family, "bwd_q", q, hv)
    _launch(dev, entry, g, g.stride(0), out, out.stride(0), saved, q, q.stride(0), k, k.stride(0), v, v.stride(0), n, l, h,
            hv, d, code, *scale, dq, h * d, delta, delta.numel() * 4)
    return dq, delta


def _hip_bwd_kv(family: str, scale: tuple, g, saved, delta, q, k, v):
    dev, (n, h, d), l, hv = q.device, q.shape, k.shape[0], v.shape[1]
    dk = torch.empty((l, h, d), dtype=q.dtype, device=dev)
    dv = torch.empty((l, hv, d), dtype=q.dtype, device=dev)
    entry, code = _entry(family, "bwd_kv", q, hv)
    _launch(dev, entry, g, g.stride(0), saved, q, q.stride(0), k, k.stride(0), v, v.stride(0), n, l, h, hv, d, code, *scale,
            dk, h * d, dv, hv * d, delta, delta.numel() * 4)
    return dk, dv


class _Hip:
    @staticmethod
    def pair_sigmoid_supported(heads: int, v_heads: int, d: int, dtype) -> bool:
        return _hip_supported("pair_sigmoid", heads, v_heads, d, dtype)

    @staticmethod
    def pair_sigmoid_fwd(q, k, v):
        """(out [n, H, D] in the storage dtype, rowsum fp32 [n, H])"""
        return _hip_fwd("pair_sigmoid", (), q, k, v)

    @staticmethod
    def pair_sigmoid_bwd_q(g, out, rowsum, q, k, v, want_dq: bool = True):
        """(dq [n, H, D] or None, delta fp32 [n, H] = g . out per row and head: the operand of pair_sigmoid_bwd_kv)"""
        return _hip_bwd_q("pair_sigmoid", (), g, out, rowsum, q, k, v, want_dq)

    @staticmethod
    def pair_sigmoid_bwd_kv(g, rowsum, delta, q, k, v):
        """(dk [l, H, D], dv [l, Hv, D]; Hv = 1: dv summed over the heads)"""
        return _hip_bwd_kv("pair_sigmoid", (), g, rowsum, delta, q, k, v)

    @staticmethod
    def pair_softmax_supported(heads: int, v_heads: int, d: int, dtype) -> bool:
        return _hip_supported("pair_softmax", heads, v_heads, d, dtype)

    @staticmethod
    def pair_softmax_fwd(q, k, v, scale: float = 1.0):
        """(out [n, H, D] in the storage dtype, lse fp32 [n, H])"""
        return _hip_fwd("pair_softmax", (float(scale),), q, k, v)

    @staticmethod
    def pair_softmax_bwd_q(g, out, lse, q, k, v, scale: float = 1.0, want_dq: bool = True):
        """(dq [n, H, D] or None, delta fp32 [n, H] = g . out per row and head: the operand of pair_softmax_bwd_kv)"""
        return _hip_bwd_q("pair_softmax", (float(scale),), g, out, lse, q, k, v, want_dq)

    @staticmethod
    def pair_softmax_bwd_kv(g, lse, delta, q, k, v, scale: float = 1.0):
        """(dk [l, H, D], dv [l, Hv, D]; Hv = 1: dv summed over the heads)"""
        return _hip_bwd_kv("pair_softmax", (float(scale),), g, lse, delta, q, k, v)


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


def _use(q, k, v, family: str) -> bool:
    """_supported under the arm's switch (read on every call): 0 = always the dense path, 1 = the kernels wherever supported,
    unset = the kernels from the arm's threshold (n l H score entries) upward: the one for bf16 storage, for fp32 storage, or
    for fp32 storage when the HIP table would run the split-bf16 kernels."""
    _, switch, min_pairs, min_pairs_bf16, min_pairs_x3 = _ARMS[family]
    s = os.environ.get(switch)
    if s is not None and not _switch(switch, True):
        return False
    if not _supported(q, k, v, family):
        return False
    if s is not None:
        return True
    if q.dtype == _BF16:
        name = min_pairs_bf16
    else:
        name = min_pairs_x3 if _table(family + "_fwd") is _Hip and _x3_would_run(family, q, v) else min_pairs
    return q.shape[0] * k.shape[0] * q.shape[1] >= globals()[name]


def supported(q, k, v) -> bool:
    """q [n, H, D], k [l, H, D], v [l, H | 1, D]: tensors of one dtype on the GPU, contiguous in the last dimension, in a
    shape the library accepts, with at least one query and one key, and a kernel table that has the entries."""
    return _supported(q, k, v, "pair_sigmoid")


def use_kernels(q, k, v) -> bool:
    """supported(q, k, v) under the switch SGF_PAIR_ATTN (read on every call)."""
    return _use(q, k, v, "pair_sigmoid")


def softmax_supported(q, k, v) -> bool:
    """supported() for the softmax kernels: the same operand rules, and a kernel table that has the pair_softmax_* entries."""
    return _supported(q, k, v, "pair_softmax")


def use_softmax_kernels(q, k, v) -> bool:
    """softmax_supported(q, k, v) under the switch SGF_PAIR_SOFTMAX (read on every call): 0 = always the dense path, 1 = the
    kernels wherever supported, unset = the kernels from SOFTMAX_MIN_PAIRS / SOFTMAX_MIN_PAIRS_BF16 score entries upward."""
    return _use(q, k, v, "pair_softmax")


def _rows(t: torch.Tensor) -> torch.Tensor:
    """[rows, heads, D] with the heads side by side in 16-byte aligned rows: the [rows, heads * D] operand of the entries."""
    if (t.stride(2) != 1 or t.stride(1) != t.shape[2] or (t.stride(0) * t.element_size()) % 16 != 0
            or t.stride(0) < t.shape[1] * t.shape[2] or t.data_ptr() % 16 != 0):
        t = t.contiguous()
    return t


# ------------------------------------------------------------------------------------------------
# autograd: one implementation; `scale` is () for the sigmoid function and (scale,) for the softmax function, and goes to the
# table's methods where their signatures have it (the methods are looked up on the table at call time)
# ------------------------------------------------------------------------------------------------
def _forward(ctx, family: str, q, k, v, *scale):
    ops.K.check(q, k, v)
    t = _table(family + "_fwd")
    q, k, v = _rows(q), _rows(k), _rows(v)
    out, saved = getattr(t, family + "_fwd")(q, k, v, *scale)
    ctx.save_for_backward(q, k, v, out, saved)       # saved: the fp32 row sums (sigmoid) / log-sum-exp (softmax) [n, H]
    ctx.table, ctx.family, ctx.scale = t, family, scale
    return out


def _backward(ctx, g):
    """one gradient per input of the function: dq, dk, dv and, for the softmax function, None for the scale"""
    t, family, scale = ctx.table, ctx.family, ctx.scale
    if torch.is_grad_enabled():          # (only under create_graph=True)
        name, switch = _ARMS[family][:2]
        raise RuntimeError(f"sgformer_amd: pair_attn.{name} is once differentiable; backward with "
                           f"create_graph=True is not implemented ({switch}=0 keeps the twice differentiable path)")
    q, k, v, out, saved = ctx.saved_tensors
    need_q, need_k, need_v = ctx.needs_input_grad[:3]
    none = (None,) * len(scale)
    if not (need_q or need_k or need_v):
        return (None, None, None) + none
    g = _rows(g if g.dtype == q.dtype else g.to(q.dtype))
    dq, delta = getattr(t, family + "_bwd_q")(g, out, saved, q, k, v, *scale, want_dq=need_q)      # (delta is bwd_kv's operand too)
    dk = dv = None
    if need_k or need_v:
        dk, dv = getattr(t, family + "_bwd_kv")(g, saved, delta, q, k, v, *scale)
    return (dq, (dk if need_k else None), (dv if need_v else None)) + none


class _SigmoidAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v):
        return _forward(ctx, "pair_sigmoid", q, k, v)

    backward = staticmethod(_backward)


class _SoftmaxAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale):
        return _forward(ctx, "pair_softmax", q, k, v, scale)

    backward = staticmethod(_backward)


def _require(q, k, v, family: str) -> None:
    if not _supported(q, k, v, family):
        raise RuntimeError(f"pair_attn.{_ARMS[family][0]}: unsupported operands q {tuple(q.shape)} {q.dtype}, k {tuple(k.shape)}, "
                           f"v {tuple(v.shape)} (D in {{32, 64, 128}}, H <= 8, float32 or bfloat16, one device)")


def sigmoid_attention(q, k, v) -> torch.Tensor:
    """out [n, H, D] of the sigmoid kernel for q [n, H, D], k [l, H, D], v [l, H | 1, D]; differentiable once in q, k and v.
    The caller asks supported() / use_kernels() first: an unsupported call is an error here, not a fallback."""
    _require(q, k, v, "pair_sigmoid")
    return _SigmoidAttention.apply(q, k, v)


def softmax_attention(q, k, v, scale: float = 1.0) -> torch.Tensor:
    """out [n, H, D] = softmax over the keys of scale q . k, times v, for q [n, H, D], k [l, H, D], v [l, H | 1, D];
    differentiable once in q, k and v (scale is a constant: a finite, positive float).  The caller asks softmax_supported() /
    use_softmax_kernels() first: an unsupported call is an error here, not a fallback."""
    _require(q, k, v, "pair_softmax")
    scale = float(scale)
    if not (0.0 < scale < float("inf")):
        raise ValueError(f"pair_attn.softmax_attention: scale must be finite and positive, got {scale}")
    return _SoftmaxAttention.apply(q, k, v, scale)
