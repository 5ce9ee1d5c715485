"""Drop-in for the reference's `medium/ablation/oursSOFT.py`: SGFormer with an all-pair softmax attention in place of the
linear one (the paper's "is linear attention enough?" ablation).  Same class names, constructor signatures, `forward(data)`,
`get_attentions(x)` and `state_dict` keys as the reference; everything but the attention call is ours_medium's (fc ->
LayerNorm -> relu, alpha residual, LayerNorm, the injected `gnn`, the output Linear).

    softmax_attention(qs [N, H, M], ks [L, H, M], vs [L, H | 1, D], output_attn=False, over='heads') -> [N, H, D] (, [N, L])
        qs, ks divided by their Frobenius norms over ALL heads (oursSOFT.py:16-17), scores [N, L, H], a softmax, then
        out_n = sum_l weights_nl vs_l per head;  the map is the mean of the weights over the heads.

Which axis the softmax runs over is `over`:
  * 'heads' (the default): the reference exactly as shipped.  oursSOFT.py:22 passes `dim=-1` to F.softmax on scores laid out
    [N, L, H], so the weights are normalised over the HEADS (with one head every weight is 1 and the layer returns the sum of
    the value rows).  A model built here computes what the reference's model computes, logits and gradients
    (tests/golden/soft/, the `logits` / `grad/*` recording).  This is plain PyTorch with the reference's [N, L, H] tensors: it is
    not a softmax over the keys and no kernel of this package computes it.
  * 'keys': the exact softmax attention, weights normalised over the keys — what the ablation is about, and what
    sgformer_amd.pair_attn's kernels compute without an [N, L, H] tensor (include/sgf.h block N8, switch SGF_PAIR_SOFTMAX).  It
    equals the reference's code with that one call taken over dim=1 (the fixtures' `logits_keys` / `grad_keys/*` recording).
    `SGFormerSOFT(...).set_softmax_over('keys')` selects it for a model; the choice is no constructor argument and no part of
    the state_dict.

With 'keys', the two norms are differentiable tensor ops ahead of the kernel (scale = 1); the attention maps
(`output_attn=True`), shapes the kernels do not take and the node-sharded case stay on `_dense_attention`, plain PyTorch that
forms the scores.
"""
from __future__ import annotations

import torch

from . import ops, pair_attn
from . import ours_medium as _medium

__all__ = ["softmax_attention", "TransConvLayer", "TransConv", "SGFormerSOFT"]

_AXES = {"heads": -1, "keys": 1}


def _dense_attention(qs, ks, vs, want_attn, over="keys"):
    """The arithmetic in plain PyTorch on operands that are already normalised: scores and weights [N, L, H]."""
    weights = torch.softmax(torch.einsum("nhm,lhm->nlh", qs, ks), dim=_AXES[over])
    out = torch.einsum("nlh,lhd->nhd", weights, vs)
    return out, (weights.mean(dim=-1) if want_attn else None)


def softmax_attention(qs, ks, vs, output_attn=False, over="heads", shard=None):
    """medium/ablation/oursSOFT.py:14-34.  `over` and `shard` are not in the reference signature: the axis of the softmax
    ('heads': as shipped; 'keys': the exact softmax attention, on the tiled kernels where pair_attn takes the call), and the
    node-sharded case, which keeps the dense path."""
    if over not in _AXES:
        raise ValueError(f"ours_soft.softmax_attention: over must be 'heads' or 'keys', got {over!r}")
    qs = qs / torch.norm(qs, p=2)
    ks = ks / torch.norm(ks, p=2)
    if over == "keys" and not output_attn and shard is None and pair_attn.use_softmax_kernels(qs, ks, vs):
        return pair_attn.softmax_attention(qs, ks, vs, 1.0)
    out, attn = _dense_attention(qs, ks, vs, output_attn, over)
    return (out, attn) if output_attn else out


class TransConvLayer(_medium.TransConvLayer):
    """oursSOFT.py:37-88: the projections of the linear layer, the softmax attention, the mean over the heads."""

    softmax_over = "heads"       # the reference as shipped; SGFormerSOFT.set_softmax_over('keys') for the exact softmax attention

    def forward(self, query_input, source_input, edge_index=None, edge_weight=None, output_attn=False, grad_tap=None):
        ops._require_cuda(query_input, source_input)
        h, d = self.num_heads, self.out_channels
        qkv = self._project(query_input, source_input)
        n = qkv.shape[0]
        query = qkv[:, :h * d].reshape(n, h, d)
        key = qkv[:, h * d:2 * h * d].reshape(n, h, d)
        if self.use_weight:
            value = qkv[:, 2 * h * d:].reshape(n, h, d)
        else:
            value = source_input.reshape(-1, 1, d)
        if output_attn:
            out, attn = softmax_attention(query, key, value, True, self.softmax_over, self._shard)
            return out.mean(dim=1), attn
        return softmax_attention(query, key, value, False, self.softmax_over, self._shard).mean(dim=1)


class TransConv(_medium.TransConv):
    """oursSOFT.py:91-165."""

    def __init__(self, in_channels, hidden_channels, num_layers=2, num_heads=1, alpha=0.5, dropout=0.5,
                 use_bn=True, use_residual=True, use_weight=True, use_act=False):
        super(_medium.TransConv, self).__init__(in_channels, hidden_channels, num_layers, num_heads, dropout, use_bn,
                                                use_residual, use_weight, use_act, alpha=alpha, layer_cls=TransConvLayer)
        self.residual = use_residual


class SGFormerSOFT(_medium.SGFormer):
    """oursSOFT.py:167-211: medium/ours.py's SGFormer (same signature, `use_act` dropped the same way at :171) around the
    TransConv above."""

    _trans_cls = TransConv

    def set_softmax_over(self, over: str):
        """'heads': the reference as shipped (the default); 'keys': the exact softmax attention.  Returns the model."""
        if over not in _AXES:
            raise ValueError(f"SGFormerSOFT.set_softmax_over: over must be 'heads' or 'keys', got {over!r}")
        for conv in self.trans_conv.convs:
            conv.softmax_over = over
        return self
