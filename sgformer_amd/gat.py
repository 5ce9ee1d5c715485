"""The GAT graph branch of the medium recipes (`--backbone gat`, medium/models.py:116-155) on the edge-softmax kernels of
csrc/gat.hip (include/sgf.h block N10): torch_geometric 1.7.2 GATConv without an [E, H] or [E, H, C] tensor, in the forward or
under autograd.

    GATConv(in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True, bias=True)
        xw = x @ lin_l.weight.T                      [N, H, C]   (lin_r IS lin_l: the state_dict has both names)
        al = <xw, att_l>, ar = <xw, att_r>           [N, H]
        per target i and head: softmax over its stored entries e (source j) of leaky_relu(al[j] + ar[i]), dropout on the
        weights, out[i] = sum_e p~_e xw[j]; concat -> [N, H * C], else the mean over the heads [N, C]; + bias
    GAT(in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5, use_bn=False, heads=2, out_heads=1)

`gat_aggregate(graph, xw, att_l, att_r, ...)` is the autograd function over sgf_gat_scores / _fwd / _bwd_dst / _bwd_src: one
launch for the two node scores, one forward launch, two backward launches (the target side, then the source side over the
transposed CSR, which also folds the score terms dal att_l + dar att_r into dxw, which is why the function takes att_l / att_r
and not al / ar).  Saved for the backward: xw, al, ar and norm = (m, 1 / l) fp32 [N, H, 2]; the keep decisions are recomputed
from the seed.  datt_l, datt_r (column sums of dal xw, dar xw) and dbias stay ATen reductions.

`supported(xw, heads, channels)` says whether the kernels take the call (1 <= H <= 8, C % 4 == 0, H C <= 1024, fp32 or bf16, GPU
tensors, a kernel table that has the entries); GATConv pads a C that is not a multiple of 4 with zero channels and slices, as
ours_medium.GCNConv does.  What the kernels do not take, CPU tensors and SGF_GAT=0 run `edge_list_aggregate`: the same
arithmetic in plain PyTorch over the edge list (index_select + index_add, any dtype; it holds [E, H, C] and uses ATen's
dropout stream).  SGF_GAT: 0 = that path, 1 = the kernels wherever supported; unset = GAT_DEFAULT_ON (profiles/gat_probe.md).

Dropout: Philox keep decisions keyed on (seed, target, source, head): parallel edges i <- j share their draw (PyG draws one
per edge; ATen's stream cannot be matched anyway).  The seed is drawn as ops.dropout_res draws it; a step being
captured into a hipGraph cannot carry it (no device-seed variant): active dropout under capture raises.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, kernels, ops
from .kernels import _launch
from .linear import _switch

__all__ = ["GATConv", "GAT", "gat_aggregate", "edge_list_aggregate", "supported", "use_kernels", "GAT_DEFAULT_ON"]

_F32 = torch.float32
_BF16 = torch.bfloat16

# SGF_GAT unset: the kernels run wherever supported, because they were ahead of the edge-list path beyond the spread of the
# repetitions at every probed size, forward and forward + backward (profiles/gat_probe.md: 3.8 - 14.0 x at 100 k and 1 M nodes).
GAT_DEFAULT_ON = True


# ------------------------------------------------------------------------------------------------
# the entries on the current stream (private: the kernel table of kernels.py is not extended)
# ------------------------------------------------------------------------------------------------
class _Hip:
    @staticmethod
    def gat_supported(heads: int, c: int, dtype) -> bool:
        if dtype not in (_F32, _BF16):
            return False
        return bool(_lib.load().sgf_gat_supported(int(heads), int(c), _lib.SGF_BF16 if dtype == _BF16 else _lib.SGF_F32))

    @staticmethod
    def gat_scores(xw, att_l, att_r, heads: int):
        """(al, ar) fp32 [n, H] of xw [n, H * C] and att_l, att_r fp32 [H * C]"""
        n, c = xw.shape[0], xw.shape[1] // heads
        al = torch.empty((n, heads), dtype=_F32, device=xw.device)
        ar = torch.empty((n, heads), dtype=_F32, device=xw.device)
        _launch(xw.device, "sgf_gat_scores", xw, xw.stride(0), att_l, att_r, n, heads, c, kernels._code(xw), al, ar)
        return al, ar

    @staticmethod
    def gat_fwd(rowptr, colind, xw, al, ar, bias, heads: int, mean: bool, slope: float, p: float, seed: int):
        """(out [n, H * C] or [n, C] in the storage dtype, lse fp32 [n, H], norm fp32 [n, H, 2])"""
        n, c, dev = rowptr.numel() - 1, xw.shape[1] // heads, xw.device
        out = torch.empty((n, c if mean else heads * c), dtype=xw.dtype, device=dev)
        lse = torch.empty((n, heads), dtype=_F32, device=dev)
        norm = torch.empty((n, heads, 2), dtype=_F32, device=dev)
        _launch(dev, "sgf_gat_fwd", rowptr, colind, xw, xw.stride(0), al, ar, bias, n, xw.shape[0], heads, c, kernels._code(xw),
                int(mean), float(slope), float(p), int(seed), out, out.stride(0), lse, norm)
        return out, lse, norm

    @staticmethod
    def gat_bwd_dst(rowptr, colind, g, xw, al, ar, norm, heads: int, mean: bool, slope: float, p: float, seed: int):
        """(delta, dar) fp32 [n, H]"""
        n, c, dev = rowptr.numel() - 1, xw.shape[1] // heads, xw.device
        delta = torch.empty((n, heads), dtype=_F32, device=dev)
        dar = torch.empty((n, heads), dtype=_F32, device=dev)
        _launch(dev, "sgf_gat_bwd_dst", rowptr, colind, g, g.stride(0), xw, xw.stride(0), al, ar, norm, n, xw.shape[0], heads, c,
                kernels._code(xw), int(mean), float(slope), float(p), int(seed), delta, dar)
        return delta, dar

    @staticmethod
    def gat_bwd_src(t_rowptr, t_colind, g, xw, al, ar, norm, delta, dar, att_l, att_r, heads: int, mean: bool, slope: float,
                    p: float, seed: int):
        """(dal fp32 [n_src, H], dxw [n_src, H * C] with the score terms dal att_l + dar att_r)"""
        n_src, c, dev = xw.shape[0], xw.shape[1] // heads, xw.device
        dal = torch.empty((n_src, heads), dtype=_F32, device=dev)
        dxw = torch.empty((n_src, heads * c), dtype=xw.dtype, device=dev)
        _launch(dev, "sgf_gat_bwd_src", t_rowptr, t_colind, g, g.stride(0), xw, xw.stride(0), al, ar, norm, delta, dar, att_l,
                att_r, norm.shape[0], n_src, heads, c, kernels._code(xw), int(mean), float(slope), float(p), int(seed), dal, dxw,
                dxw.stride(0))
        return dal, dxw


def _table():
    """Where the gat_* entries live: a test's CPU table that has them, the entries above on the HIP table, nothing otherwise
    (every call then takes the edge-list path)."""
    k = ops.K
    if hasattr(k, "gat_fwd"):
        return k
    return _Hip if k.name == "hip" else None


# ------------------------------------------------------------------------------------------------
# which calls the kernels take
# ------------------------------------------------------------------------------------------------
def _takes(is_cuda: bool, dtype, n: int, heads: int, channels: int) -> bool:
    t = _table()
    if t is None or (t is _Hip and not is_cuda) or n < 1 or n >= 2 ** 31:
        return False
    return bool(t.gat_supported(int(heads), int(channels), dtype))


def supported(xw, heads: int, channels: int) -> bool:
    """xw [N, H * C]: a GPU tensor (or a CPU tensor under a test's CPU table), fp32 or bf16, in a shape the library accepts."""
    if not torch.is_tensor(xw) or xw.dim() != 2 or xw.shape[1] != heads * channels:
        return False
    return _takes(xw.is_cuda, xw.dtype, xw.shape[0], heads, channels)


def use_kernels(x, heads: int, channels: int) -> bool:
    """Whether a layer whose input is x [N, .] runs the kernels for H heads of C channels: supported() for its projection
    (same rows, device and dtype) under the switch SGF_GAT (read on every call): 0 = the edge-list path, 1 = the kernels
    wherever supported, unset = GAT_DEFAULT_ON."""
    if not _switch("SGF_GAT", GAT_DEFAULT_ON):
        return False
    return torch.is_tensor(x) and x.dim() == 2 and _takes(x.is_cuda, x.dtype, x.shape[0], heads, channels)


def _rows(t: torch.Tensor) -> torch.Tensor:
    """rows contiguous and aligned to what a lane moves (4 channels)"""
    if t.stride(1) != 1 or t.stride(0) % 4 != 0 or t.data_ptr() % 16 != 0 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def _draw_seed() -> int:
    """as ops.dropout_res draws it: 62 bits from torch's CPU generator, reproducible under torch.manual_seed, no sync"""
    if kernels.seed_scope() is not None:
        raise RuntimeError("sgformer_amd: gat attention dropout has no device-seed variant; it cannot run inside a captured "
                           "step (SGF_GAT=0 keeps ATen's dropout)")
    seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64))
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        seed = (seed + (torch.distributed.get_rank() + 1) * 0x9E3779B97F4A7C15) % (2 ** 62)
    return seed


# ------------------------------------------------------------------------------------------------
# autograd over the four launches
# ------------------------------------------------------------------------------------------------
class _GatAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xw, att_l, att_r, bias, graph, heads, slope, p, mean, seed):
        ops.K.check(xw, att_l, att_r, bias)
        t = _table()
        xw = _rows(xw)
        wl = att_l.detach().reshape(-1).to(_F32).contiguous()
        wr = att_r.detach().reshape(-1).to(_F32).contiguous()
        b = None if bias is None else bias.detach().to(_F32).contiguous()
        al, ar = t.gat_scores(xw, wl, wr, heads)
        out, lse, norm = t.gat_fwd(graph.rowptr, graph.colind, xw, al, ar, b, heads, mean, slope, p, seed)
        ctx.save_for_backward(xw, al, ar, norm, wl, wr)
        ctx.meta = (t, graph, heads, slope, p, mean, seed, att_l.shape, att_l.dtype, bias is not None and bias.dtype)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, g, _g_lse):
        if torch.is_grad_enabled():          # (only under create_graph=True)
            raise RuntimeError("sgformer_amd: gat.gat_aggregate is once differentiable; backward with create_graph=True is "
                               "not implemented (SGF_GAT=0 keeps the twice differentiable path)")
        xw, al, ar, norm, wl, wr = ctx.saved_tensors
        t, graph, heads, slope, p, mean, seed, att_shape, att_dtype, bias_dtype = ctx.meta
        g = _rows(g if g.dtype == xw.dtype else g.to(xw.dtype))
        delta, dar = t.gat_bwd_dst(graph.rowptr, graph.colind, g, xw, al, ar, norm, heads, mean, slope, p, seed)
        t_rowptr, t_colind = graph.transposed()[:2]
        dal, dxw = t.gat_bwd_src(t_rowptr, t_colind, g, xw, al, ar, norm, delta, dar, wl, wr, heads, mean, slope, p, seed)
        # the parameter gradients: column sums over the nodes (ATen)
        x3 = xw.view(xw.shape[0], heads, -1).float()
        datt_l = torch.einsum("nh,nhc->hc", dal, x3).reshape(att_shape).to(att_dtype) if ctx.needs_input_grad[1] else None
        datt_r = torch.einsum("nh,nhc->hc", dar, x3).reshape(att_shape).to(att_dtype) if ctx.needs_input_grad[2] else None
        dbias = g.float().sum(0).to(bias_dtype) if ctx.needs_input_grad[3] else None
        return dxw, datt_l, datt_r, dbias, None, None, None, None, None, None


def gat_aggregate(graph, xw, att_l, att_r, *, negative_slope=0.2, dropout=0.0, training=False, concat=True, bias=None,
                  return_lse=False):
    """out [N, H * C] (concat) or [N, C] (head mean) of the edge-softmax attention over `graph` (a graph.CSRGraph whose rows are
    the targets) for xw [N, H * C] and att_l, att_r [1, H, C] (or [H, C]); + bias.  Differentiable once in xw, att_l, att_r and
    bias.  The caller asks supported() / use_kernels() first: an unsupported call is an error here, not a fallback."""
    heads, c = att_l.shape[-2], att_l.shape[-1]
    if not supported(xw, heads, c) or graph.n != xw.shape[0]:
        raise RuntimeError(f"gat.gat_aggregate: unsupported operands xw {tuple(xw.shape)} {xw.dtype} for {heads} heads of {c} "
                           f"channels on {graph.n} nodes (1 <= H <= 8, C % 4 == 0, H C <= 1024, float32 or bfloat16)")
    p = float(dropout) if training else 0.0
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"gat.gat_aggregate: dropout must be in [0, 1], got {p}")
    seed = _draw_seed() if p > 0.0 else 0
    out, lse = _GatAggregate.apply(xw, att_l, att_r, bias, graph, heads, float(negative_slope), p, not concat, seed)
    return (out, lse) if return_lse else out


# ------------------------------------------------------------------------------------------------
# the same arithmetic in plain PyTorch over the edge list
# ------------------------------------------------------------------------------------------------
def _with_self_loops(edge_index, n: int):
    keep = edge_index[0] != edge_index[1]
    loops = torch.arange(n, dtype=edge_index.dtype, device=edge_index.device)
    return torch.cat([edge_index[:, keep], torch.stack([loops, loops])], dim=1)


def edge_list_aggregate(edge_index, n: int, xw, att_l, att_r, *, negative_slope=0.2, dropout=0.0, training=False, concat=True,
                        bias=None):
    """gat_aggregate over the edge list `edge_index` ([2, E]: source, target; taken as it is) in ATen operators, any dtype."""
    heads, c = att_l.shape[-2], att_l.shape[-1]
    src, dst = edge_index[0], edge_index[1]
    x3 = xw.reshape(n, heads, c)
    al = (x3 * att_l.reshape(1, heads, c)).sum(-1)
    ar = (x3 * att_r.reshape(1, heads, c)).sum(-1)
    s = F.leaky_relu(al.index_select(0, src) + ar.index_select(0, dst), negative_slope)            # [E, H]
    idx = dst.unsqueeze(1).expand(-1, heads)
    m = torch.full((n, heads), -math.inf, dtype=s.dtype, device=s.device).scatter_reduce(0, idx, s.detach(), "amax")
    e = torch.exp(s - m.index_select(0, dst))
    l = torch.zeros((n, heads), dtype=s.dtype, device=s.device).index_add(0, dst, e)
    w = F.dropout(e / l.index_select(0, dst), p=float(dropout), training=training)
    out = torch.zeros((n, heads, c), dtype=xw.dtype, device=xw.device).index_add(0, dst, w.unsqueeze(-1) * x3.index_select(0, src))
    out = out.reshape(n, heads * c) if concat else out.mean(1)
    return out if bias is None else out + bias.to(out.dtype)


# ------------------------------------------------------------------------------------------------
# modules
# ------------------------------------------------------------------------------------------------
def _glorot(t: torch.Tensor):
    a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    t.data.uniform_(-a, a)


class GATConv(nn.Module):
    """torch_geometric 1.7.2 GATConv with an int `in_channels`: parameter names, shapes and initialisation as there."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True,
                 bias=True, **kwargs):
        super().__init__()
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope, self.dropout, self.add_self_loops = concat, negative_slope, dropout, add_self_loops
        self.lin_l = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.lin_r = self.lin_l
        self.att_l = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_r = nn.Parameter(torch.empty(1, heads, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(heads * out_channels if concat else out_channels))
        else:
            self.register_parameter("bias", None)
        self._shard = None
        self.reset_parameters()

    def reset_parameters(self):
        _glorot(self.lin_l.weight)
        _glorot(self.att_l)
        _glorot(self.att_r)
        if self.bias is not None:
            self.bias.data.fill_(0)

    def _graph(self, edge_index, n: int):
        if not self.add_self_loops:
            return ops.graph_cache.get(edge_index, n, tag="gat")
        return ops.graph_cache.get(edge_index, n, factory=lambda ei, _n: ops.CSRGraph(_with_self_loops(ei, n), n),
                                   tag="gat_self_loops")

    def forward(self, x, edge_index):
        if self._shard is not None:
            raise NotImplementedError("sgformer_amd: GATConv has no node-sharded path")
        n, h, c = x.shape[0], self.heads, self.out_channels
        w, att_l, att_r, bias = self.lin_l.weight, self.att_l, self.att_r, self.bias
        cp = c + (-c % 4)
        kw = dict(negative_slope=self.negative_slope, dropout=self.dropout, training=self.training, concat=self.concat)
        if use_kernels(x, h, cp):
            if cp != c:
                # the kernels move 4 channels per lane: compute on the head width rounded up to a multiple of 4 (zero weight
                # rows, zero att and bias entries) and slice — `--method gat` ends in a layer as wide as the class count
                w = F.pad(w.view(h, c, -1), (0, 0, 0, cp - c)).reshape(h * cp, -1)
                att_l, att_r = F.pad(att_l, (0, cp - c)), F.pad(att_r, (0, cp - c))
                if bias is not None:
                    bias = F.pad(bias.view(-1, c), (0, cp - c)).reshape(-1)
            xw = ops.linear(x, w, None)
            out = gat_aggregate(self._graph(edge_index, n), xw, att_l, att_r, bias=bias, **kw)
            if cp != c:
                out = out.view(n, -1, cp)[:, :, :c].reshape(n, -1)
            return out
        ei = _with_self_loops(edge_index, n) if self.add_self_loops else edge_index
        return edge_list_aggregate(ei, n, F.linear(x, w), att_l, att_r, bias=bias, **kw)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, heads={self.heads})"


class GAT(nn.Module):
    """medium/models.py:116-155: input dropout, GATConv(concat) + optional BatchNorm1d(hidden * heads) + ELU + dropout per
    hidden layer, a last GATConv with out_heads heads and concat=False."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, dropout=0.5, use_bn=False, heads=2,
                 out_heads=1):
        super().__init__()
        self.convs = nn.ModuleList()
        self.convs.append(GATConv(in_channels, hidden_channels, dropout=dropout, heads=heads, concat=True))
        self.bns = nn.ModuleList()
        self.bns.append(nn.BatchNorm1d(hidden_channels * heads))
        for _ in range(num_layers - 2):
            self.convs.append(GATConv(hidden_channels * heads, hidden_channels, dropout=dropout, heads=heads, concat=True))
            self.bns.append(nn.BatchNorm1d(hidden_channels * heads))
        self.convs.append(GATConv(hidden_channels * heads, out_channels, dropout=dropout, heads=out_heads, concat=False))
        self.dropout = dropout
        self.activation = F.elu
        self.use_bn = use_bn

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()
        for bn in self.bns:
            bn.reset_parameters()

    def forward(self, data):
        x = data.graph['node_feat']
        edge_index = data.graph['edge_index']
        x = F.dropout(x, p=self.dropout, training=self.training)
        for i, conv in enumerate(self.convs[:-1]):
            x = conv(x, edge_index)
            if self.use_bn:
                x = self.bns[i](x)
            x = self.activation(x)
            x = F.dropout(x, p=self.dropout, training=self.training)
        return self.convs[-1](x, edge_index)
