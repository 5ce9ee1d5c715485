"""Losses of three training steps as hex floats (profiles/model_layer_refactor.md): the default bf16 workload (ogbn-products
recipe) and the fp32 ogbn-arxiv recipe of benchlib/workloads.py at 70 000 nodes — above ours.OVERLAP_MIN_NODES, so that the
attention branch runs on its side stream.  Every reduction of the step is per-launch deterministic: two trees that enqueue
the same launches print the same bits.

    python scripts/model_layer_losses.py LABEL [--tree DIR] [--nodes N] [--steps K] [--graph uniform|community]

--graph community with SGF_REORDER=1 (profiles/graph_layer_refactor.md): a graph whose re-ordered CSR is adopted, so that the
steps run the tile plan (bf16) and the stream kernel (fp32); the line "view" says what was decided.

--tree DIR: import sgformer_amd from DIR (another checkout's sgformer_amd/*.py, e.g. the parent commit's) but load THIS
tree's libsgf.so, so that two trees are compared on identical kernels.  One process per tree.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("label")
ap.add_argument("--tree", default=ROOT)
ap.add_argument("--nodes", type=int, default=70000)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--graph", choices=("uniform", "community"), default="uniform")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))

import sgformer_amd                      # noqa: E402
from sgformer_amd import _lib            # noqa: E402
_lib.LIB_PATH = os.path.join(ROOT, "sgformer_amd", "lib", "libsgf.so")
from sgformer_amd import launch, ops, ours, synth    # noqa: E402
from sgformer_amd.loss import log_softmax_nll        # noqa: E402

dev = torch.device("cuda:0")
print(f"{a.label}: package {os.path.dirname(sgformer_amd.__file__)}, {a.nodes} nodes, side stream from "
      f"{ours.OVERLAP_MIN_NODES} nodes", flush=True)
for workload, dtype in (("ogbn-products", torch.bfloat16), ("ogbn-arxiv", None)):
    _, avg_deg, f, c, d = synth.SHAPES[workload]
    n, seed = a.nodes, 123
    ei = (synth.synthetic_graph if a.graph == "uniform" else synth.synthetic_graph_community)(n, avg_deg, seed=seed, device=dev)
    x, y, train_idx = (t.to(dev) for t in synth.synthetic_task(n, f, c, seed=seed))
    torch.manual_seed(seed)
    model = ours.SGFormer(f, d, c, trans_dropout=0.0, gnn_dropout=0.0, compute_dtype=dtype, **synth.RECIPES[workload]).to(dev)
    model.logits_dtype = torch.float32
    launch.patch_adam()
    opt = torch.optim.Adam([{"params": model.params1, "weight_decay": 1e-5},
                            {"params": model.params2, "weight_decay": 1e-5}], lr=0.01)
    model.train()
    view = ops.prepare_graph(ei, n)
    print(f"{a.label} {workload} view: " + ", ".join(f"{k}={view.stats[k]!r}" for k in ("reordered", "why", "kernel", "lds_fraction")
                                                      if k in view.stats), flush=True)
    losses = []
    for _ in range(a.steps):
        opt.zero_grad(set_to_none=True)
        loss = log_softmax_nll(model(x, ei), y, train_idx)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()).hex())
    torch.cuda.synchronize()
    print(f"{a.label} {workload} {'f32' if dtype is None else 'bf16'}: {' '.join(losses)}", flush=True)
    del model, opt
    ops.graph_cache.clear()
