"""The CPU kernel table of tests/cpu_kernels_metrics.py plus `dropout_dev` (sgf_dropout_dev, include/sgf.h: sgf_dropout with
the seed read from a slot of an int64 tensor) — TEST ONLY, same contract as sgformer_amd.kernels.HipKernels.dropout_dev.
Every call is recorded in `calls` as (kernel, slot or None, seed) so that a test can see which slot a call took."""
import torch

from tests.cpu_kernels_metrics import CpuKernelsMetrics


class CpuKernelsDropout(CpuKernelsMetrics):
    def __init__(self):
        super().__init__()
        self.calls = []

    def dropout(self, x, res, p, seed):
        self.calls.append(("dropout", None, int(seed)))
        return CpuKernelsMetrics.dropout(x, res, p, seed)

    def dropout_dev(self, x, res, p, seeds, slot):
        assert seeds.dtype == torch.int64 and seeds.dim() == 1 and seeds.is_contiguous()
        assert 0 <= slot < seeds.numel()
        self.calls.append(("dropout_dev", int(slot), int(seeds[slot])))
        return CpuKernelsMetrics.dropout(x, res, p, int(seeds[slot]))
