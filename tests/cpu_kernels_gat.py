"""The CPU kernel table of tests/cpu_kernels.py plus the edge-softmax entries (sgf_gat_*, include/sgf.h block N10) restated in
fp64 torch over the stored entries of the CSR — TEST ONLY, the contract of sgformer_amd.gat._Hip: what each launch reads and
writes, norm = (m, 1 / l), the Philox keep convention (counter (target, source, 0x53474154, head / 4), word head % 4, key =
seed; the integer Philox is tests/philox_host.py).  Every call is counted in `calls`."""
import torch

from tests.cpu_kernels import CpuKernels
from tests.philox_host import philox4x32_10

GAT_TAG = 0x53474154
_M32 = 0xFFFFFFFF
F64 = torch.float64


def gat_keep(seed, tgt, src, heads, p):
    """keep [E, H] bool for the entries (tgt[e] <- src[e]): a function of (target, source, head) alone"""
    tgt, src = tgt.to(torch.int64), src.to(torch.int64)
    cols = []
    for h in range(heads):
        z = torch.zeros_like(tgt)
        words = philox4x32_10((tgt & _M32, src & _M32, z + GAT_TAG, z + (h >> 2)), (seed & _M32, (seed >> 32) & _M32))
        u = (words[h & 3] >> 8).to(torch.float32) * (1.0 / 16777216.0)
        cols.append(u >= torch.tensor(p, dtype=torch.float32, device=tgt.device))
    return torch.stack(cols, 1)


def _rows_of(rowptr):
    n = rowptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=rowptr.device), rowptr[1:] - rowptr[:-1])


def _kf(seed, tgt, src, heads, p):
    if p <= 0:
        return torch.ones((tgt.numel(), heads), dtype=F64, device=tgt.device)
    return gat_keep(seed, tgt, src, heads, p).to(F64) * (1.0 / (1.0 - p) if p < 1 else 0.0)


def _entry_weights(tgt, src, al, ar, norm, slope):
    z = al.to(F64)[src] + ar.to(F64)[tgt]
    sl = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    p = torch.exp(z * sl - norm.to(F64)[tgt, :, 0]) * norm.to(F64)[tgt, :, 1]
    return p, sl


class CpuKernelsGat(CpuKernels):
    calls = {}

    @classmethod
    def _count(cls, name, rows):
        cls.calls.setdefault(name, []).append(int(rows))

    @staticmethod
    def gat_supported(heads, c, dtype):
        return dtype in (torch.float32, torch.bfloat16) and 1 <= heads <= 8 and c >= 4 and c % 4 == 0 and heads * c <= 1024

    @classmethod
    def gat_scores(cls, xw, att_l, att_r, heads):
        cls._count("gat_scores", xw.shape[0])
        x3 = xw.to(F64).view(xw.shape[0], heads, -1)
        return ((x3 * att_l.to(F64).view(1, heads, -1)).sum(-1).float(), (x3 * att_r.to(F64).view(1, heads, -1)).sum(-1).float())

    @classmethod
    def gat_fwd(cls, rowptr, colind, xw, al, ar, bias, heads, mean, slope, p, seed):
        n = rowptr.numel() - 1
        cls._count("gat_fwd", n)
        tgt, src = _rows_of(rowptr), colind.long()
        x3 = xw.to(F64).view(xw.shape[0], heads, -1)
        z = al.to(F64)[src] + ar.to(F64)[tgt]
        s = torch.where(z > 0, z, slope * z)
        m = torch.full((n, heads), -float("inf"), dtype=F64).scatter_reduce(0, tgt[:, None].expand(-1, heads), s, "amax")
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        e = torch.exp(s - m[tgt])
        l = torch.zeros((n, heads), dtype=F64).index_add(0, tgt, e)
        any_ = l > 0
        linv = torch.where(any_, 1.0 / torch.where(any_, l, torch.ones_like(l)), torch.zeros_like(l))
        w = e * linv[tgt] * _kf(seed, tgt, src, heads, p)
        out = torch.zeros((n, heads, x3.shape[2]), dtype=F64).index_add(0, tgt, w[:, :, None] * x3[src])
        out = out.mean(1) if mean else out.reshape(n, -1)
        if bias is not None:
            out = out + bias.to(F64)
        lse = torch.where(any_, m + torch.log(torch.where(any_, l, torch.ones_like(l))), torch.zeros_like(l))
        return out.to(xw.dtype), lse.float(), torch.stack([m, linv], 2).float()

    @classmethod
    def gat_bwd_dst(cls, rowptr, colind, g, xw, al, ar, norm, heads, mean, slope, p, seed):
        n = rowptr.numel() - 1
        cls._count("gat_bwd_dst", n)
        tgt, src = _rows_of(rowptr), colind.long()
        x3 = xw.to(F64).view(xw.shape[0], heads, -1)
        gh = (g.to(F64) / heads)[:, None, :].expand(-1, heads, -1) if mean else g.to(F64).view(n, heads, -1)
        pe, sl = _entry_weights(tgt, src, al, ar, norm, slope)
        t = pe * _kf(seed, tgt, src, heads, p) * (gh[tgt] * x3[src]).sum(-1)
        zero = torch.zeros((n, heads), dtype=F64)
        a, b, s = zero.index_add(0, tgt, t), zero.index_add(0, tgt, t * sl), zero.index_add(0, tgt, pe * sl)
        return a.float(), (b - a * s).float()

    @classmethod
    def gat_bwd_src(cls, t_rowptr, t_colind, g, xw, al, ar, norm, delta, dar, att_l, att_r, heads, mean, slope, p, seed):
        n_src = t_rowptr.numel() - 1
        cls._count("gat_bwd_src", n_src)
        src, tgt = _rows_of(t_rowptr), t_colind.long()
        x3 = xw.to(F64).view(n_src, heads, -1)
        gh = (g.to(F64) / heads)[:, None, :].expand(-1, heads, -1) if mean else g.to(F64).view(g.shape[0], heads, -1)
        pe, sl = _entry_weights(tgt, src, al, ar, norm, slope)
        kf = _kf(seed, tgt, src, heads, p)
        dp = (gh[tgt] * x3[src]).sum(-1)
        dz = pe * (kf * dp - delta.to(F64)[tgt]) * sl
        dal = torch.zeros((n_src, heads), dtype=F64).index_add(0, src, dz)
        dxw = torch.zeros_like(x3).index_add(0, src, (pe * kf)[:, :, None] * gh[tgt])
        dxw = dxw + dal[:, :, None] * att_l.to(F64).view(1, heads, -1) + dar.to(F64)[:, :, None] * att_r.to(F64).view(1, heads, -1)
        return dal.float(), dxw.reshape(n_src, -1).to(xw.dtype)
