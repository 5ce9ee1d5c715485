"""Host cost per call of the kernel table (profiles/kernel_table_host_cost.md): 20 000 eager calls each of K.axpby,
K.bn_apply, K.colstats, K.bce_fwd and K.gcn_epilogue_dx at n = 256, d = 64, bf16 after a warm-up, a host clock around the
loop ending in a synchronise.  Small shapes on purpose: the quantity is what the host spends to enqueue one launch.

    python scripts/kernel_table_host_cost.py LABEL [--tree DIR] [--out FILE.jsonl]

--tree DIR: import sgformer_amd from DIR (another checkout's sgformer_amd/*.py, e.g. the parent commit's) but load THIS
tree's libsgf.so, so that two trees are compared on identical GPU work.  Run one process per measurement, trees alternating.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("label")
ap.add_argument("--tree", default=ROOT)
ap.add_argument("--out", default=None)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))

import sgformer_amd                      # noqa: E402
from sgformer_amd import _lib            # noqa: E402
_lib.LIB_PATH = os.path.join(ROOT, "sgformer_amd", "lib", "libsgf.so")
from sgformer_amd import ops             # noqa: E402

K = ops.K
dev = torch.device("cuda:0")
torch.manual_seed(0)
n, d = 256, 64
bf = torch.bfloat16
x = torch.randn(n, d, device=dev).to(bf)
x2 = torch.randn(n, d, device=dev).to(bf)
res = torch.randn(n, d, device=dev).to(bf)
mean, rstd, gamma, beta, shift = (torch.rand(d, device=dev) + 0.5 for _ in range(5))
logits = torch.randn(n, d, device=dev).to(bf)
target = (torch.rand(n, d, device=dev) > 0.5).float()
dy = torch.randn(n, d, device=dev).to(bf)
w = torch.randn(d, d, device=dev).to(bf)

calls = {
    "axpby": lambda: K.axpby(x, 0.5, x2, 0.5),
    "bn_apply": lambda: K.bn_apply(x, mean, rstd, gamma, beta, res, True),
    "colstats": lambda: K.colstats(x, shift),
    "bce_fwd": lambda: K.bce_fwd(logits, target, None, 1.0 / n),
    "gcn_epilogue_dx": lambda: K.gcn_epilogue_dx(dy, w),
}
WARM, REPS = 2000, 20000
result = {"label": a.label, "package": os.path.dirname(sgformer_amd.__file__), "device": torch.cuda.get_device_name(0),
          "us_per_call": {}}
for name, f in calls.items():
    for _ in range(WARM):
        f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        f()
    torch.cuda.synchronize()
    result["us_per_call"][name] = round((time.perf_counter() - t0) / REPS * 1e6, 3)
line = json.dumps(result)
print(line, flush=True)
if a.out:
    with open(a.out, "a") as fh:
        fh.write(line + "\n")
