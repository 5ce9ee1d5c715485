"""The CPU kernel table of tests/cpu_kernels.py plus the entries of the head on selected rows (sgf_head_rows_supported /
_fwd / _bwd, include/sgf.h block N6) — TEST ONLY, the contract of sgformer_amd.head_rows._Hip: prefix rows when idx is None,
z rounded once to the storage dtype, W rounded to bf16 for bf16 storage, compact fp32 logits, labels one per selected row.
Every call is counted in `calls` so that a test can tell which entries a path used."""
import torch

from tests.cpu_kernels import CpuKernels


def _z(x1, a, x2, b, idx, m):
    s1 = x1[:m] if idx is None else x1[idx]
    z = a * s1.float()
    if x2 is not None:
        z = z + b * (x2[:m] if idx is None else x2[idx]).float()
    return z.to(x1.dtype).float()


class CpuKernelsHeadRows(CpuKernels):
    calls = {}

    @classmethod
    def _count(cls, name, rows):
        cls.calls.setdefault(name, []).append(int(rows))

    @staticmethod
    def head_rows_supported(d, classes, dtype):
        if dtype == torch.bfloat16:
            return 0 < d <= 256 and d % 32 == 0 and 1 <= classes <= 256
        return dtype == torch.float32 and 0 < d <= 256 and d % 4 == 0 and 1 <= classes <= 256

    @classmethod
    def head_rows_fwd(cls, x1, a, x2, b, w, bias, idx, m, labels=None):
        cls._count("head_rows_fwd" if labels is None else "head_rows_ce", m)
        c = w.shape[0]
        logits = _z(x1, a, x2, b, idx, m) @ w.to(x1.dtype).float().t() + bias.float()
        if labels is None:
            return logits, None, None, None
        lse = torch.logsumexp(logits, dim=1)
        ok = (labels >= 0) & (labels < c)
        picked = logits.gather(1, labels.clamp(0, c - 1)[:, None])[:, 0]
        loss_sum = ((lse - picked) * ok).sum().reshape(1)
        hit = (logits.argmax(1) == labels) & ok if m > 0 else ok
        return logits, lse, loss_sum, torch.stack([ok.sum(), hit.sum()]).to(torch.int64)

    @classmethod
    def head_rows_bwd(cls, x1, a, x2, b, w, idx, m, dlogits=None, logits=None, lse=None, labels=None, gout=None,
                      inv_denom=1.0):
        cls._count("head_rows_bwd", m)
        c = w.shape[0]
        if dlogits is not None:
            g = dlogits.float()
        else:
            ok = (labels >= 0) & (labels < c)
            onehot = (labels[:, None] == torch.arange(c)[None, :]).float()
            g = (torch.exp(logits - lse[:, None]) - onehot) * (gout.reshape(-1)[0] * inv_denom)
            g = torch.where(ok[:, None], g, torch.zeros_like(g))
        dt = x1.dtype
        dx = g.to(dt).float() @ w.to(dt).float()
        sel = slice(0, m) if idx is None else idx
        dx1 = torch.zeros_like(x1)
        dx1[sel] = (a * dx).to(dt)
        dx2 = None
        if x2 is not None:
            dx2 = torch.zeros_like(x2)
            dx2[sel] = (b * dx).to(dt)
        z = _z(x1, a, x2, b, idx, m)
        return dx1, dx2, g.t() @ z, g.sum(0)
