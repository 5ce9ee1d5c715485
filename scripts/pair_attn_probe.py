#!/usr/bin/env python
"""DIFFormer's sigmoid attention: the tiled kernels of csrc/pair_attn.hip (pair_attn.sigmoid_attention) against the dense
path (difformer._dense_attention: three einsums and an [n, l, H] fp32 score tensor), on one MI355X, in ONE process with the
two paths interleaved.  Sizes n = l in {2 708, 19 717, 50 000}, D = 64, H in {1, 4}, bf16 and fp32 storage.  Per cell, HIP
events around (a) the forward and (b) forward + backward, median (min .. max) of 7 repetitions after 3 warm-ups, the path
that goes first alternating; torch.cuda.max_memory_allocated of each path over the operands; the kernels' rate as
4 n l H D / t (forward) and 14 n l H D / t (backward = (b) - (a)).  A dense leg that runs out of memory is written as OOM.
Writes a markdown table (the worst error ratios of tests/test_gpu_pair_attn.py are appended from --ratios, the `PAIR_RATIO`
lines of a `pytest -s` run of that file) and prints one JSON line; --cells FILE rewrites the report from such a line.  One process, no retries: run it under one time limit,
    timeout -k 10 900 python scripts/pair_attn_probe.py [--out profiles/pair_attn_probe.md] [--ratios LOG]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgformer_amd import pair_attn  # noqa: E402
from sgformer_amd.difformer import _dense_attention  # noqa: E402

SIZES = (2708, 19717, 50000)
HEADS = (1, 4)
D = 64
WARM, REPS = 3, 7


def fmt(ms):
    return "OOM" if ms is None else f"{statistics.median(ms):.3f} ({min(ms):.3f} .. {max(ms):.3f})"


def run(path, q, k, v, g, backward):
    """one timed call: milliseconds between two events on the current stream"""
    ops = [t.detach().requires_grad_(backward) for t in (q, k, v)]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = pair_attn.sigmoid_attention(*ops) if path == "kernels" else _dense_attention(*ops, 'sigmoid', False)[0]
    if backward:
        out.backward(g)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def leg(path, q, k, v, g, backward):
    """(times or None on OOM, peak bytes over the operands)"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    try:
        t = run(path, q, k, v, g, backward)
    except torch.OutOfMemoryError:
        torch.cuda.empty_cache()
        return None, None
    return t, torch.cuda.max_memory_allocated() - base


def cell(n, h, dtype, dev):
    gen = torch.Generator().manual_seed(n + h)
    q, k = ((2.0 / D ** 0.5) * torch.randn(n, h, D, generator=gen) for _ in range(2))
    v, g = (torch.randn(n, h, D, generator=gen) for _ in range(2))
    q, k, v, g = (t.to(dev, dtype) for t in (q, k, v, g))
    res = {}
    for backward in (False, True):
        times = {"kernels": [], "dense": []}
        peak = {"kernels": 0, "dense": 0}
        for rep in range(WARM + REPS):
            order = ("kernels", "dense") if rep % 2 == 0 else ("dense", "kernels")
            for path in order:
                if times[path] is None:
                    continue
                t, mem = leg(path, q, k, v, g, backward)
                if t is None:
                    times[path] = None               # OOM: written as such, not retried
                    continue
                peak[path] = max(peak[path], mem)
                if rep >= WARM:
                    times[path].append(t)
        res["fwdbwd" if backward else "fwd"] = (times, peak)
    return res


def ratios(path):
    worst = {}
    if path and os.path.exists(path):
        for line in open(path):
            p = line.split()
            if len(p) == 3 and p[0] == "PAIR_RATIO":
                name = p[1]
                kind = name.split("[")[0] + "/" + ("bf16" if "bfloat16" in name else "fp32") + "/" + name.rsplit(".", 1)[-1]
                if float(p[2]) > worst.get(kind, (-1.0, ""))[0]:
                    worst[kind] = (float(p[2]), name)
    return worst


def ahead(c):
    """the kernels' slowest repetition beats the dense path's fastest one (or the dense path is OOM), both timings"""
    return all(c[d] is None or max(c[k]) < min(c[d]) for k, d in (("fwd_kernels", "fwd_dense"), ("fwdbwd_kernels", "fwdbwd_dense")))


def threshold(cells):
    """smallest probed n l H such that every cell of that size or larger is ahead; 0: every cell; None: not even the largest"""
    sizes = sorted({c["pairs"] for c in cells})
    behind = sorted({c["pairs"] for c in cells if not ahead(c)})
    if not behind:
        return 0, behind
    above = [s for s in sizes if s > behind[-1]]
    return (above[0] if above else None), behind


def report(cells, worst, out):
    mb = lambda x: "-" if not x else f"{x / 2 ** 20:.0f}"     # noqa: E731
    with open(out, "w") as f:
        f.write("# Sigmoid attention: tiled kernels against the dense path (scripts/pair_attn_probe.py)\n\n")
        f.write(f"One MI355X, one process, the two paths interleaved; HIP events; milliseconds as median (min .. max) of {REPS} "
                f"repetitions after {WARM} warm-ups.  n = l, D = {D}.  Peak = torch.cuda.max_memory_allocated over the operands "
                "in MiB (forward + backward).  TF/s: the kernels' 4 n l H D / t forward and 14 n l H D / (t_fwdbwd - t_fwd) "
                "backward.  Every leg starts from an emptied allocator cache, so a dense leg that needs gigabytes pays the "
                "device allocation in some repetitions (the large maxima, and the medians of the largest cells): its min is the "
                "steady figure, and the rule below compares against that min.  The dense path is difformer._dense_attention, "
                "unchanged from the parent commit.\n\n")
        f.write("| dtype | n | H | fwd kernels | fwd dense | fwd+bwd kernels | fwd+bwd dense | peak kernels | peak dense | "
                "TF/s fwd | TF/s bwd | ahead |\n|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for c in cells:
            f.write(f"| {c['dtype']} | {c['n']} | {c['heads']} | {fmt(c['fwd_kernels'])} | {fmt(c['fwd_dense'])} | "
                    f"{fmt(c['fwdbwd_kernels'])} | {fmt(c['fwdbwd_dense'])} | {mb(c['peak_kernels'])} | "
                    f"{mb(c['peak_dense']) if c['fwdbwd_dense'] else 'OOM'} | {c['tflops_fwd']:.1f} | {c['tflops_bwd']:.1f} | "
                    f"{'yes' if ahead(c) else 'NO'} |\n")
        f.write("\nYardstick (not a bar): a plain-HIP flash attention forward with a softmax reaches about 1000 TF/s in bf16 at "
                "D = 128 on this chip; these kernels are at D = 64, spend one exp and one rcp per score, and stage every tile "
                "without a prefetch.\n\n")
        f.write("## PAIR_MIN_PAIRS\n\nRule, per storage dtype: a cell is ahead when, for the forward and for forward + backward, "
                "the kernels' slowest repetition is faster than the dense path's fastest one (or the dense path is OOM).  The "
                "threshold is the smallest probed n l H such that every cell of that size or larger is ahead; 0 when every "
                "cell is.\n\n")
        res = {}
        for dt in sorted({c["dtype"] for c in cells}):
            t, behind = threshold([c for c in cells if c["dtype"] == dt])
            res[dt] = t
            f.write(f"* {dt}: cells NOT ahead at n l H = {behind if behind else 'none'}; threshold = {t}.\n")
        f.write("\n`pair_attn.PAIR_MIN_PAIRS` (fp32 storage) and `pair_attn.PAIR_MIN_PAIRS_BF16` hold these two numbers.\n\n")
        if worst:
            f.write("## Worst error / bar of tests/test_gpu_pair_attn.py\n\n| check | worst ratio | case |\n|---|---|---|\n")
            for kind in sorted(worst):
                f.write(f"| {kind} | {worst[kind][0]:.4f} | {worst[kind][1]} |\n")
            over = [k for k in worst if worst[k][0] > 0.5]
            f.write("\n" + (f"Above 0.5 of the bar: {', '.join(sorted(over))}.\n" if over else "No ratio exceeds 0.5.\n"))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_attn_probe.md"))
    ap.add_argument("--ratios", default=None, help="output of `pytest -s tests/test_gpu_pair_attn.py` (PAIR_RATIO lines)")
    ap.add_argument("--cells", default=None, help="the JSON line of an earlier run: rewrite the report, measure nothing")
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    args = ap.parse_args()
    if args.cells:
        cells = json.loads([ln for ln in open(args.cells) if ln.startswith("{")][-1])["cells"]
    else:
        dev = torch.device("cuda:0")
        os.environ["SGF_PAIR_ATTN"] = "1"
        cells = []
        for dtype in (torch.bfloat16, torch.float32):
            for n in (int(s) for s in args.sizes.split(",")):
                for h in HEADS:
                    r = cell(n, h, dtype, dev)
                    (tf, pf), (tb, pb) = r["fwd"], r["fwdbwd"]
                    kf, kb = statistics.median(tf["kernels"]), statistics.median(tb["kernels"])
                    pairs = n * n * h
                    cells.append(dict(dtype=str(dtype)[6:], n=n, heads=h, pairs=pairs,
                                      fwd_kernels=tf["kernels"], fwd_dense=tf["dense"], fwdbwd_kernels=tb["kernels"],
                                      fwdbwd_dense=tb["dense"], peak_kernels=pb["kernels"], peak_dense=pb["dense"],
                                      tflops_fwd=4 * pairs * D / (kf * 1e-3) / 1e12,
                                      tflops_bwd=14 * pairs * D / (max(kb - kf, 1e-6) * 1e-3) / 1e12))
                    print(f"{cells[-1]['dtype']} n={n} H={h}: fwd {fmt(tf['kernels'])} / {fmt(tf['dense'])}, fwd+bwd "
                          f"{fmt(tb['kernels'])} / {fmt(tb['dense'])}", flush=True)
    res = report(cells, ratios(args.ratios), args.out)
    print(json.dumps(dict(probe="pair_attn", thresholds=res, cells=cells)))


if __name__ == "__main__":
    main()
