"""The CPU kernel table of tests/cpu_kernels.py plus the all-pair softmax attention entries (sgf_pair_softmax_*, include/sgf.h
block N8) restated in fp64 torch — TEST ONLY, the contract of sgformer_amd.pair_attn._Hip: q [n, H, D], k [l, H, D],
v [l, Hv, D] with Hv in {1, H}; out in the storage dtype, lse and delta fp32 [n, H]; Hv = 1: dv summed over the heads.  Every
call is counted in `calls` (entry name -> list of n) so that a test can tell which entries a path used."""
import torch

from tests.cpu_kernels import CpuKernels


def _z(q, k, scale):
    return scale * torch.einsum("nhd,lhd->nlh", q.double(), k.double())               # [n, l, H]


def _gv(g, v, heads):
    return torch.einsum("nhd,lhd->nlh", g.double(), v.double().expand(-1, heads, -1))


class CpuKernelsPairSoftmax(CpuKernels):
    calls = {}

    @classmethod
    def _count(cls, name, rows):
        cls.calls.setdefault(name, []).append(int(rows))

    @staticmethod
    def pair_softmax_supported(heads, v_heads, d, dtype):
        return (dtype in (torch.float32, torch.bfloat16) and d in (32, 64, 128) and 1 <= heads <= 8
                and v_heads in (1, heads))

    @classmethod
    def pair_softmax_fwd(cls, q, k, v, scale=1.0):
        cls._count("pair_softmax_fwd", q.shape[0])
        z = _z(q, k, scale)
        m = z.max(dim=1).values
        e = torch.exp(z - m[:, None, :])
        r = e.sum(1)
        out = torch.einsum("nlh,lhd->nhd", e, v.double().expand(-1, q.shape[1], -1)) / r[:, :, None]
        return out.to(q.dtype), (m + torch.log(r)).float()

    @classmethod
    def pair_softmax_bwd_q(cls, g, out, lse, q, k, v, scale=1.0, want_dq=True):
        cls._count("pair_softmax_bwd_q", q.shape[0])
        delta = (g.double() * out.double()).sum(2)
        if not want_dq:
            return None, delta.float()
        p = torch.exp(_z(q, k, scale) - lse.double()[:, None, :])
        dz = scale * p * (_gv(g, v, q.shape[1]) - delta[:, None, :])
        return torch.einsum("nlh,lhd->nhd", dz, k.double()).to(q.dtype), delta.float()

    @classmethod
    def pair_softmax_bwd_kv(cls, g, lse, delta, q, k, v, scale=1.0):
        cls._count("pair_softmax_bwd_kv", q.shape[0])
        p = torch.exp(_z(q, k, scale) - lse.double()[:, None, :])
        dz = scale * p * (_gv(g, v, q.shape[1]) - delta.double()[:, None, :])
        dk = torch.einsum("nlh,nhd->lhd", dz, q.double())
        dv = torch.einsum("nlh,nhd->lhd", p, g.double())
        if v.shape[1] == 1 and q.shape[1] > 1:
            dv = dv.sum(1, keepdim=True)
        return dk.to(q.dtype), dv.to(q.dtype)
