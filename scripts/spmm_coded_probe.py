"""sgf_spmm_code_rows (k_code_rows + k_count_escaped) back to back on a products-size operand: 5 launches per figure, HIP
events, two rounds, for a Gaussian operand and for one with nine tenths zero rows (profiles/spmm_coded_kernel_stats.md).

    python scripts/spmm_coded_probe.py
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sgformer_amd import ops
K = ops.K
dev = torch.device("cuda:0")
n = 2449029
torch.manual_seed(0)
ops_ = {"randn": torch.randn(n, 256, device=dev).to(torch.bfloat16)}
z = ops_["randn"].clone(); z[torch.rand(n, device=dev) < 0.9] = 0
ops_["90% zero rows"] = z
for name, x in ops_.items():
    for rnd in range(2):
        K.spmm_code_rows(x); torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(5):
            out = K.spmm_code_rows(x)
        b.record(); torch.cuda.synchronize()
        print(f"k_code_rows {name} round {rnd}: {a.elapsed_time(b) / 5:.3f} ms per launch, escaped {int(out[2].item())}", flush=True)
