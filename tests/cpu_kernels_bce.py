"""The CPU kernel table of tests/cpu_kernels.py plus the two entries of the multi-label loss (sgf_bce_fwd / sgf_bce_bwd,
include/sgf.h block N4b) — TEST ONLY, same contract as sgformer_amd.kernels.HipKernels.bce_fwd / bce_bwd: fp32 arithmetic
on the stored logits, the target read as float32 / int64 [n, c] or as int64 class indices [n], idx None = every row."""
import torch

from tests.cpu_kernels import CpuKernels


def _target_rows(logits, target, idx):
    """float32 [m, c] target of the selected rows; a class index outside [0, c) matches no column."""
    n, c = logits.shape
    assert target.dtype in (torch.float32, torch.int64), target.dtype
    t = target if idx is None else target[idx]
    if target.dim() == 1:
        assert target.shape[0] == n and target.dtype == torch.int64
        return (t[:, None] == torch.arange(c)[None, :]).to(torch.float32)
    assert target.shape == logits.shape
    return t.to(torch.float32)


class CpuKernelsBce(CpuKernels):
    @staticmethod
    def bce_fwd(logits, target, idx, inv_denom=1.0):
        x = (logits if idx is None else logits[idx]).float()
        t = _target_rows(logits, target, idx)
        return (x.clamp_min(0) - x * t + torch.log1p(torch.exp(-x.abs()))).sum() * torch.tensor(inv_denom, dtype=torch.float32)

    @staticmethod
    def bce_bwd(logits, target, idx, gout, inv_denom):
        x = (logits if idx is None else logits[idx]).float()
        t = _target_rows(logits, target, idx)
        z = torch.exp(-x.abs())
        g = (torch.where(x >= 0, torch.ones_like(z), z) / (1 + z) - t) * (gout.reshape(-1)[0] * inv_denom)
        if idx is None:
            return g.to(logits.dtype)
        d = torch.zeros(logits.shape, dtype=torch.float32)
        d[idx] = g
        return d.to(logits.dtype)
