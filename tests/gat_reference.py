"""GATConv's aggregation (torch_geometric 1.7.2, as restated in include/sgf.h block N10) as DENSE fp64 algebra — TEST ONLY, written
independently of sgformer_amd.gat's edge-list path: an [N, N] multiplicity matrix (mult[i, j] = stored entries of target i with
source j; parallel edges count, each once), a masked softmax over every target's row, and a keep mask handed in.  [N, N, H]
tensors: usable to about 600 nodes.

    dense(xw [N, H, C], att_l [H, C], att_r [H, C], mult [N, N], ...) -> (out, lse [N, H])          differentiable (fp64 autograd)
    backward(...)  -> dict(delta, dar, dal, dxw, datt_l, datt_r, dbias) by the closed formulas, for a given dOut
    multiplicity(edge_index, n, add_self_loops) -> mult
"""
import torch

F64 = torch.float64


def multiplicity(edge_index, n, add_self_loops=True):
    """mult[target, source]; add_self_loops: every existing self-loop dropped, exactly one per node added"""
    src, dst = edge_index[0].long(), edge_index[1].long()
    mult = torch.zeros(n * n, dtype=F64, device=edge_index.device)
    mult.index_add_(0, dst * n + src, torch.ones(src.numel(), dtype=F64, device=edge_index.device))
    mult = mult.view(n, n)
    if add_self_loops:
        eye = torch.eye(n, dtype=F64, device=edge_index.device)
        mult = mult * (1 - eye) + eye
    return mult


def _weights(xw, att_l, att_r, mult, slope):
    """(p [N, N, H] per PAIR: multiplicity times the weight of one entry; sl [N, N, H]; lse [N, H])"""
    al = (xw * att_l[None]).sum(-1)                       # [N, H]
    ar = (xw * att_r[None]).sum(-1)
    z = al[None, :, :] + ar[:, None, :]                   # [target, source, H]
    pos = z > 0
    s = torch.where(pos, z, slope * z)
    on = (mult > 0)[:, :, None]
    sm = torch.where(on, s, torch.full_like(s, -float("inf")))
    m = sm.max(dim=1).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m)).detach()     # an empty row
    e = torch.where(on, torch.exp(s - m[:, None, :]), torch.zeros_like(s)) * mult[:, :, None]
    l = e.sum(1)
    safe = torch.where(l > 0, l, torch.ones_like(l))
    p = e / safe[:, None, :]
    lse = torch.where(l > 0, m + torch.log(safe), torch.zeros_like(l))
    sl = torch.where(pos, torch.ones_like(z), torch.full_like(z, slope))
    return p, sl, lse


def dense(xw, att_l, att_r, mult, negative_slope=0.2, keep=None, p_drop=0.0, concat=True, bias=None):
    """keep: [N, N, H] bool (target, source, head) or None; the normalisation is over the undropped weights"""
    xw, att_l, att_r, mult = xw.to(F64), att_l.to(F64), att_r.to(F64), mult.to(F64)
    p, _, lse = _weights(xw, att_l, att_r, mult, negative_slope)
    if keep is not None and p_drop > 0:
        p = p * keep.to(F64) * (1.0 / (1.0 - p_drop) if p_drop < 1 else 0.0)
    out = torch.einsum("ijh,jhc->ihc", p, xw)
    out = out.reshape(out.shape[0], -1) if concat else out.mean(1)
    if bias is not None:
        out = out + bias.to(F64)
    return out, lse


def backward(xw, att_l, att_r, mult, g, negative_slope=0.2, keep=None, p_drop=0.0, concat=True):
    """The closed formulas of the backward for dOut = g ([N, H * C], or [N, C] with concat=False)."""
    xw, att_l, att_r, mult, g = xw.to(F64), att_l.to(F64), att_r.to(F64), mult.to(F64), g.to(F64)
    n, h, c = xw.shape
    p, sl, _ = _weights(xw, att_l, att_r, mult, negative_slope)
    kf = torch.ones_like(p)
    if keep is not None and p_drop > 0:
        kf = keep.to(F64) * (1.0 / (1.0 - p_drop) if p_drop < 1 else 0.0)
    gh = g.view(n, h, c) if concat else (g / h)[:, None, :].expand(n, h, c)
    dp = torch.einsum("ihc,jhc->ijh", gh, xw)
    pt = p * kf
    delta = (pt * dp).sum(1)
    dz = p * (kf * dp - delta[:, None, :]) * sl
    dar, dal = dz.sum(1), dz.sum(0)
    dxw = torch.einsum("ijh,ihc->jhc", pt, gh) + dal[:, :, None] * att_l[None] + dar[:, :, None] * att_r[None]
    return dict(delta=delta, dar=dar, dal=dal, dxw=dxw, datt_l=torch.einsum("nh,nhc->hc", dal, xw),
                datt_r=torch.einsum("nh,nhc->hc", dar, xw), dbias=g.sum(0))
