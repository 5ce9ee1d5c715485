#!/usr/bin/env python
"""Timing of the multi-label loss (forward + backward) at the ogbn-proteins shapes, three ways, interleaved in one process:
  aten     the trainers' lines as written (large/main.py:130-137): out[train_idx], the cast, nn.BCEWithLogitsLoss() on ATen
  patched  the same lines under sgformer_amd.launch.patch_bce_loss() (ATen's indexing, the dense form of sgf_bce_fwd / _bwd)
  rows     sgformer_amd.loss.bce_with_logits_rows (row gather fused as well)
at the mini-batch shape (10 000 x 112, ~65 % training rows) and a full-graph step (132 534 x 112).  HIP events after
warm-up; the three variants take turns inside every repetition and the median per variant is reported.

--sweep adds the measurement behind launch.BCE_PATCH_MIN_ELEMENTS: the trainers' lines on ATen against the same lines with the
one-pass criterion at EVERY size (patch_bce_loss(min_elements=0)), over a range of node counts at C = 112.

    python scripts/bce_probe.py [--reps 30] [--sweep] [--md profiles/bce_probe.md]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgformer_amd import launch, loss as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--sweep", action="store_true", help="also measure where the one-pass criterion overtakes ATen")
ap.add_argument("--md", default=None, help="also write the table to this markdown file")
args = ap.parse_args()

dev = torch.device("cuda:0")
criterion = nn.BCEWithLogitsLoss()


def lines(out, true_label, train_idx):
    loss = criterion(out[train_idx], true_label.squeeze(1)[train_idx].to(torch.float))
    loss.backward()
    return loss


def rows(out, true_label, train_idx):
    loss = L.bce_with_logits_rows(out, true_label, train_idx)
    loss.backward()
    return loss


def once(fn, *a):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn(*a)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def measure(n, c, frac, variants=("aten", "patched", "rows"), min_elements=None):
    g = torch.Generator().manual_seed(123)
    out = (torch.randn(n, c, generator=g) * 3).to(dev).requires_grad_(True)
    true_label = torch.randint(0, 2, (n, c), generator=g).to(dev)            # int64 [N, 112], as ogbn-proteins holds them
    train_idx = torch.randperm(n, generator=g)[: int(frac * n)].to(dev)
    times = {v: [] for v in variants}

    def run(name):
        out.grad = None
        if name == "patched":
            launch.patch_bce_loss(min_elements)
        try:
            return once(rows if name == "rows" else lines, out, true_label, train_idx)
        finally:
            if name == "patched":
                launch.unpatch_bce_loss()

    for _ in range(5):
        for name in times:
            run(name)
    for _ in range(args.reps):
        for name in times:
            times[name].append(run(name))
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}


shapes = [("mini-batch 10 000 x 112, 65 % training rows", 10000, 112, 0.65),
          ("full graph 132 534 x 112, 65 % training rows", 132534, 112, 0.65)]
result = {}
for label, n, c, frac in shapes:
    result[label] = measure(n, c, frac)
sweep = {}
if args.sweep:
    for n in (10000, 30000, 60000, 90000, 110000, 132534, 200000):
        sweep[n] = measure(n, 112, 0.65, ("aten", "patched"), 0)
print(json.dumps({"bce_probe_ms": result, "sweep_ms": sweep, "reps": args.reps, "device": torch.cuda.get_device_name(0)}))
if args.md:
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write("# Multi-label loss, forward + backward (scripts/bce_probe.py)\n\n"
                f"One MI355X; HIP events, median of {args.reps} interleaved repetitions after warm-up, all three variants in one "
                "process; ms.\n"
                "`aten`: the trainers' lines as written on ATen (the yardstick); `patched`: the same lines under "
                "`launch.patch_bce_loss()`; `rows`: `loss.bce_with_logits_rows`.  Targets: int64 `[N, 112]`, as ogbn-proteins "
                "holds them.\nBox-to-box spread: +- 3 % (README).  Reading: DESIGN.md section 6.\n\n"
                "| shape | aten | patched | rows | patched / aten | rows / aten |\n|---|---|---|---|---|---|\n")
        for label, t in result.items():
            f.write(f"| {label} | {t['aten']:.4f} | {t['patched']:.4f} | {t['rows']:.4f} | {t['patched'] / t['aten']:.2f} | "
                    f"{t['rows'] / t['aten']:.2f} |\n")
        if sweep:
            f.write(f"\nWhere the one-pass criterion overtakes ATen (`--sweep`: `patch_bce_loss(min_elements=0)`, C = 112, 65 % "
                    f"training rows); `launch.BCE_PATCH_MIN_ELEMENTS` = {launch.BCE_PATCH_MIN_ELEMENTS} comes from this table.\n\n"
                    "| nodes | elements of out[train_idx] | aten | one-pass criterion | ratio |\n|---|---|---|---|---|\n")
            for n, t in sweep.items():
                f.write(f"| {n} | {int(0.65 * n) * 112} | {t['aten']:.4f} | {t['patched']:.4f} | {t['patched'] / t['aten']:.2f} |\n")
