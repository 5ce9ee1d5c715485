"""The CPU kernel table of tests/cpu_kernels.py plus the all-pair sigmoid attention entries (sgf_pair_sigmoid_*, include/sgf.h
block N7) in plain torch — TEST ONLY, the contract of sgformer_amd.pair_attn._Hip: q [n, H, D], k [l, H, D], v [l, Hv, D]
with Hv in {1, H}; out in the storage dtype, rowsum and delta fp32 [n, H]; Hv = 1: dv summed over the heads.  Every call is
counted in `calls` (entry name -> list of n) so that a test can tell which entries a path used."""
import torch

from tests.cpu_kernels import CpuKernels


def _scores(q, k):
    return torch.sigmoid(torch.einsum("nhd,lhd->nlh", q.float(), k.float()))          # [n, l, H]


class CpuKernelsPairAttn(CpuKernels):
    calls = {}

    @classmethod
    def _count(cls, name, rows):
        cls.calls.setdefault(name, []).append(int(rows))

    @staticmethod
    def pair_sigmoid_supported(heads, v_heads, d, dtype):
        return (dtype in (torch.float32, torch.bfloat16) and d in (32, 64, 128) and 1 <= heads <= 8
                and v_heads in (1, heads))

    @classmethod
    def pair_sigmoid_fwd(cls, q, k, v):
        cls._count("pair_sigmoid_fwd", q.shape[0])
        s = _scores(q, k)
        rowsum = s.sum(1)
        out = torch.einsum("nlh,lhd->nhd", s, v.float().expand(-1, q.shape[1], -1)) / rowsum[:, :, None]
        return out.to(q.dtype), rowsum

    @classmethod
    def pair_sigmoid_bwd_q(cls, g, out, rowsum, q, k, v, want_dq=True):
        cls._count("pair_sigmoid_bwd_q", q.shape[0])
        delta = (g.float() * out.float()).sum(2)
        if not want_dq:
            return None, delta
        s = _scores(q, k)
        p = torch.einsum("nhd,lhd->nlh", g.float(), v.float().expand(-1, q.shape[1], -1))
        dz = s * (1 - s) * (p - delta[:, None, :]) / rowsum[:, None, :]
        return torch.einsum("nlh,lhd->nhd", dz, k.float()).to(q.dtype), delta

    @classmethod
    def pair_sigmoid_bwd_kv(cls, g, rowsum, delta, q, k, v):
        cls._count("pair_sigmoid_bwd_kv", q.shape[0])
        s = _scores(q, k)
        p = torch.einsum("nhd,lhd->nlh", g.float(), v.float().expand(-1, q.shape[1], -1))
        dz = s * (1 - s) * (p - delta[:, None, :]) / rowsum[:, None, :]
        dk = torch.einsum("nlh,nhd->lhd", dz, q.float())
        dv = torch.einsum("nlh,nhd->lhd", s / rowsum[:, None, :], g.float())
        if v.shape[1] == 1 and q.shape[1] > 1:
            dv = dv.sum(1, keepdim=True)
        return dk.to(q.dtype), dv.to(q.dtype)
