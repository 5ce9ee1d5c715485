#!/usr/bin/env python
"""Timing of the three row passes of the attention from the un-projected input over fp32 storage — sgf_attn_h_fwd,
sgf_attn_h_bwd_apply, sgf_attn_h_bwd_reduce — under torch.set_float32_matmul_precision('highest') (the exact fp32 matrix
cores: k_attn_apply<float, DP, 4|5|6>, k_attn_reduce<float, DP, 3>) and 'high' (SGF_F32_BF16X3: csrc/attn_f32x.hip), at the
pokec node count and d = 256 / 128 / 64.

Both settings take turns inside every repetition of ONE process ('highest' launches the exact kernels unchanged, so it is
the baseline in the same call); HIP events around each call after warm-up; median and min..max over the repetitions; the
fraction of the 6.3 TB/s copy rate (scripts/kernel_roofline.py's yardstick) on the algorithmic bytes of the entry:
    fwd         read h, write out, den                    2 n d + n   floats
    bwd_apply   read g, out, h, den, write dh             4 n d + n   floats (the second launch's re-read of dh is not counted)
    bwd_reduce  read h, g, out, den                       3 n d + n   floats

    python scripts/attn_f32x_probe.py [--n 1632803] [--reps 7] [--md profiles/attn_f32x_high.md]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgformer_amd import ops  # noqa: E402

COPY = 6300.0   # GB/s, scripts/kernel_roofline.py

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1632803)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--md", default=None, help="also write the table to this markdown file")
args = ap.parse_args()

dev = torch.device("cuda:0")
K = ops.K


def once(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def measure(n, d):
    g_ = torch.Generator(device=dev).manual_seed(d)
    h = torch.randn(n, d, generator=g_, device=dev)
    g = torch.randn(n, d, generator=g_, device=dev)
    M = torch.randn(d, d, generator=g_, device=dev) / d ** 0.5
    D = torch.randn(d, d, generator=g_, device=dev) / d ** 0.5
    m, ds = torch.randn(d, generator=g_, device=dev), torch.randn(d, generator=g_, device=dev)
    w = 0.5 * torch.rand(d, generator=g_, device=dev) / d
    beta = torch.full((1,), 3.0, device=dev)
    o, den = K.attn_h_fwd(h, M, m, w, beta)
    entries = {
        "fwd": (lambda: K.attn_h_fwd(h, M, m, w, beta), 2 * n * d + n),
        "bwd_apply": (lambda: K.attn_h_bwd_apply(h, g, o, den, M, w, D, ds), 4 * n * d + n),
        "bwd_reduce": (lambda: K.attn_h_bwd_reduce(h, g, o, den), 3 * n * d + n),
    }
    times = {(e, p): [] for e in entries for p in ("highest", "high")}
    try:
        for rep in range(3 + args.reps):
            for e, (fn, _) in entries.items():
                for p in ("highest", "high"):
                    torch.set_float32_matmul_precision(p)
                    t = once(fn)
                    if rep >= 3:
                        times[(e, p)].append(t)
    finally:
        torch.set_float32_matmul_precision("highest")
    rows = {}
    for e, (_, floats) in entries.items():
        row = {"gbytes": 4e-9 * floats}
        for p in ("highest", "high"):
            v = sorted(times[(e, p)])
            row[p] = {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1],
                      "of_copy": 4e-9 * floats / (1e-3 * v[len(v) // 2]) / COPY}
        rows[e] = row
    return rows


result = {d: measure(args.n, d) for d in (256, 128, 64)}
print(json.dumps({"attn_f32x_probe": result, "n": args.n, "reps": args.reps, "device": torch.cuda.get_device_name(0)}))
if args.md:
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write("# Attention row passes over fp32 storage: 'highest' against 'high' (scripts/attn_f32x_probe.py)\n\n"
                f"One MI355X, n = {args.n}; HIP events, median (min .. max) of {args.reps} repetitions after 3 warm-up rounds, both "
                "settings interleaved in one process; ms.  `of copy`: algorithmic bytes of the entry over the median, as a "
                "fraction of the 6.3 TB/s a device copy reaches (scripts/kernel_roofline.py).  `bwd_apply` is two launches.\n\n"
                "| d | entry | GB | 'highest' ms | of copy | 'high' ms | of copy | highest / high |\n|---|---|---|---|---|---|---|---|\n")
        for d, rows in result.items():
            for e, r in rows.items():
                a, b = r["highest"], r["high"]
                f.write(f"| {d} | {e} | {r['gbytes']:.2f} | {a['median_ms']:.3f} ({a['min_ms']:.3f} .. {a['max_ms']:.3f}) | "
                        f"{a['of_copy']:.2f} | {b['median_ms']:.3f} ({b['min_ms']:.3f} .. {b['max_ms']:.3f}) | {b['of_copy']:.2f} | "
                        f"{a['median_ms'] / b['median_ms']:.2f} |\n")
