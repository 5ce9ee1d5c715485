#!/usr/bin/env python
"""All-pair attention on fp32 tensors under torch.set_float32_matmul_precision('high'): the split-bf16 kernels (csrc/pair_attn.hip,
the sgf_pair_*_x3_* entries of block N9) against (a) the exact fp32 kernels of the same file (the same call under 'highest') and
(b) the dense path under 'high' (difformer._dense_attention / ours_soft._dense_attention: [n, l, H] scores and library GEMMs
that honour the same setting), on one MI355X, in ONE process with the three paths interleaved.  Both arms (sigmoid, softmax with
scale = 1), n = l in {5 000, 10 000, 20 000, 40 000}, H in {1, 2, 4}, D in {32, 64, 128}.  Per cell, HIP events around (a) the
forward and (b) forward + backward, median (min .. max) of 5 repetitions after 2 warm-ups, the order of the paths rotating.  A
dense leg that runs out of memory is written as OOM and not retried.  The allocator cache is emptied between cells, not between
repetitions.
Writes a markdown report (the register table from --resources, the compiler's kernel-resource-usage remarks; the worst error
ratios of tests/test_gpu_pair_x3.py from --ratios, the `X3_RATIO` lines of a `pytest -s` run of that file) and prints one JSON
line (also kept, cell by cell, in --json); --cells FILE rewrites the report from such a line.  One process, no retries: run it
under one time limit,
    timeout -k 10 1100 python scripts/pair_x3_probe.py [--out profiles/pair_x3_probe.md] [--ratios LOG] [--resources FILE]"""
import argparse
import json
import os
import re
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgformer_amd import difformer, ours_soft, pair_attn  # noqa: E402

SIZES = (5000, 10000, 20000, 40000)
HEADS = (1, 2, 4)
WIDTHS = (32, 64, 128)
ARMS = ("sigmoid", "softmax")
WARM, REPS = 2, 5
PATHS = ("x3", "exact", "dense")
PRECISION = {"x3": "high", "exact": "highest", "dense": "high"}


def fmt(ms):
    return "OOM" if ms is None else f"{statistics.median(ms):.3f} ({min(ms):.3f} .. {max(ms):.3f})"


def run(arm, path, q, k, v, g, backward):
    """one timed call: milliseconds between two events on the current stream"""
    ops = [t.detach().requires_grad_(backward) for t in (q, k, v)]
    torch.set_float32_matmul_precision(PRECISION[path])
    try:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if path == "dense":
            out = (difformer._dense_attention(*ops, 'sigmoid', False) if arm == "sigmoid" else
                   ours_soft._dense_attention(*ops, False, "keys"))[0]
        else:
            out = pair_attn.sigmoid_attention(*ops) if arm == "sigmoid" else pair_attn.softmax_attention(*ops)
        if backward:
            out.backward(g)
        b.record()
        b.synchronize()
    finally:
        torch.set_float32_matmul_precision("highest")
    return a.elapsed_time(b)


def leg(arm, path, q, k, v, g, backward):
    try:
        return run(arm, path, q, k, v, g, backward)
    except torch.OutOfMemoryError:
        torch.cuda.empty_cache()
        return None


def cell(arm, n, h, d, dev):
    gen = torch.Generator().manual_seed(n + h + d)
    q, k = ((2.0 / d ** 0.5) * torch.randn(n, h, d, generator=gen) for _ in range(2))
    v, g = (torch.randn(n, h, d, generator=gen) for _ in range(2))
    q, k, v, g = (t.to(dev) for t in (q, k, v, g))
    res = {}
    for backward in (False, True):
        torch.cuda.empty_cache()
        times = {p: [] for p in PATHS}
        for rep in range(WARM + REPS):
            for i in range(len(PATHS)):
                path = PATHS[(i + rep) % len(PATHS)]
                if times[path] is None:
                    continue
                t = leg(arm, path, q, k, v, g, backward)
                if t is None:
                    times[path] = None               # OOM: written as such, not retried
                elif rep >= WARM:
                    times[path].append(t)
        res["fwdbwd" if backward else "fwd"] = times
    return res


def launches(arm, dev):
    """the entries one forward + backward launches under 'high': the probe measures nothing if they are not the x3 ones"""
    names, launch = [], pair_attn._launch
    pair_attn._launch = lambda device, name, *a: (names.append(name), launch(device, name, *a))[1]
    try:
        q, k, v, g = (torch.randn(300, 2, 64, device=dev) for _ in range(4))
        run(arm, "x3", q, k, v, g, True)
    finally:
        pair_attn._launch = launch
    return names


def ratios(path):
    worst = {}
    if path and os.path.exists(path):
        for line in open(path):
            p = line[max(line.find("X3_RATIO "), 0):].split()       # (pytest -q -s puts its progress dots in front)
            if len(p) == 3 and p[0] == "X3_RATIO":
                name = p[1]
                arm = "softmax" if "softmax" in name else "sigmoid" if "sigmoid" in name else "-"
                kind = name.split("[")[0].split(".")[0] + "/" + arm + "/" + (name.rsplit(".", 1)[-1] if "[" in name else "parameters")
                if "logits" in name:
                    kind = name.split("[")[0].split(".")[0] + "/" + arm + "/logits"
                if float(p[2]) > worst.get(kind, (-1.0, ""))[0]:
                    worst[kind] = (float(p[2]), name)
    return worst


def resources(path):
    """[(kernel, VGPRs, AGPRs, spilled VGPRs, scratch bytes per lane, waves per SIMD, LDS bytes)] of the f32x3 kernels from the
    compiler's remarks (hipcc ... -Rpass-analysis=kernel-resource-usage -c sgformer_amd/csrc/pair_attn.hip 2> FILE)"""
    rows, seen = [], set()
    if path and os.path.exists(path):
        for block in re.split(r"remark: [^\n]*Function Name: ", open(path).read())[1:]:
            m = re.match(r"\S*?(k_pa_fwd|k_ps_fwd|k_pair_bwd_q|k_pair_bwd_kv)I\S*?f32x3ELi(\d+)E(\S*)", block)
            if m:
                score = "SoftmaxScore" if "SoftmaxScore" in m.group(3) else "SigmoidScore" if "SigmoidScore" in m.group(3) else ""
                name = f"{m.group(1)}<f32x3, {m.group(2)}{', ' + score if score else ''}>"
                if name in seen:
                    continue
                seen.add(name)
                get = lambda key: int(re.search(key + r": (\d+)", block).group(1))      # noqa: E731
                rows.append((name, get("VGPRs"), get("AGPRs"), get("VGPRs Spill"), get(r"ScratchSize \[bytes/lane\]"),
                             get(r"Occupancy \[waves/SIMD\]"), get(r"LDS Size \[bytes/block\]")))
    return rows


def ahead(c, other):
    """the split kernels' slowest repetition beats the other path's fastest one (or that path is OOM), both timings"""
    return all(c[o] is None or max(c[k]) < min(c[o]) for k, o in (("fwd_x3", "fwd_" + other), ("fwdbwd_x3", "fwdbwd_" + other)))


def threshold(cells):
    """smallest probed n l H such that every cell of that size or larger is ahead of the dense path; 0: every cell; None: not
    even the largest"""
    sizes = sorted({c["pairs"] for c in cells})
    behind = sorted({c["pairs"] for c in cells if not ahead(c, "dense")})
    if not behind:
        return 0, behind
    above = [s for s in sizes if s > behind[-1]]
    return (above[0] if above else None), behind


def report(cells, worst, out, regs=()):
    med = statistics.median
    with open(out, "w") as f:
        f.write("# All-pair attention under fp32 'high': split-bf16 kernels against the exact fp32 kernels and the dense path "
                "(scripts/pair_x3_probe.py)\n\n")
        f.write(f"One MI355X, one process, the three paths interleaved; HIP events; milliseconds as median (min .. max) of {REPS} "
                f"repetitions after {WARM} warm-ups.  fp32 tensors, n = l, softmax scale = 1.  x3: the sgf_pair_*_x3_* kernels "
                "(the call under 'high'); exact: the v_mfma_f32_32x32x2_f32 kernels (the same call under 'highest'; their code is "
                "instruction for instruction what it was before the split arm was added); dense: the [n, l, H] path under 'high'.  "
                "TF/s: the split kernels' 4 n l H D / t forward and 14 n l H D / (t_fwdbwd - t_fwd) backward.  exact / x3: the exact "
                "kernels' median over the split kernels' (forward; forward + backward).  `> exact`: the split kernels' slowest "
                "repetition beats the exact kernels' fastest one in both timings; `> dense`: the same against the dense path.\n\n")
        f.write("| arm | n | H | D | fwd x3 | fwd exact | fwd dense | fwd+bwd x3 | fwd+bwd exact | fwd+bwd dense | TF/s fwd | TF/s bwd | "
                "exact / x3 | > exact | > dense |\n" + "|---" * 15 + "|\n")
        for c in cells:
            xs = f"{med(c['fwd_exact']) / med(c['fwd_x3']):.2f}; {med(c['fwdbwd_exact']) / med(c['fwdbwd_x3']):.2f}"
            f.write(f"| {c['arm']} | {c['n']} | {c['heads']} | {c['d']} | {fmt(c['fwd_x3'])} | {fmt(c['fwd_exact'])} | "
                    f"{fmt(c['fwd_dense'])} | {fmt(c['fwdbwd_x3'])} | {fmt(c['fwdbwd_exact'])} | {fmt(c['fwdbwd_dense'])} | "
                    f"{c['tflops_fwd']:.1f} | {c['tflops_bwd']:.1f} | {xs} | {'yes' if ahead(c, 'exact') else 'NO'} | "
                    f"{'yes' if ahead(c, 'dense') else 'NO'} |\n")
        f.write("\n## Against the exact fp32 kernels\n\n")
        for arm in ARMS:
            rs = [(med(c["fwd_exact"]) / med(c["fwd_x3"]), med(c["fwdbwd_exact"]) / med(c["fwdbwd_x3"]), c) for c in cells if c["arm"] == arm]
            if not rs:
                continue
            f.write(f"* {arm}: forward {min(r[0] for r in rs):.2f} x to {max(r[0] for r in rs):.2f} x (median "
                    f"{med([r[0] for r in rs]):.2f} x); forward + backward {min(r[1] for r in rs):.2f} x to "
                    f"{max(r[1] for r in rs):.2f} x (median {med([r[1] for r in rs]):.2f} x).\n")
        notahead = [c for c in cells if not ahead(c, "exact")]
        f.write("\nCells in which the split kernels are NOT ahead of the exact kernels beyond the spread: " + (", ".join(
            f"{c['arm']} n = {c['n']} H = {c['heads']} D = {c['d']}" for c in notahead) if notahead else "none") + ".\n")
        f.write("\n## PAIR_MIN_PAIRS_X3 / SOFTMAX_MIN_PAIRS_X3\n\nRule (the rule of PAIR_MIN_PAIRS, profiles/pair_attn_probe.md), with "
                "the dense path under the same 'high' setting: a cell is ahead when, for the forward and for forward + backward, "
                "the split kernels' slowest repetition is faster than the dense path's fastest one (or the dense path is OOM).  The "
                "threshold is the smallest probed n l H such that every cell of that size or larger, at every probed head count and "
                "width, is ahead; 0 when every cell is.\n\n")
        res = {}
        for arm in ARMS:
            sub = [c for c in cells if c["arm"] == arm]
            if sub:
                t, behind = threshold(sub)
                res[arm] = t
                f.write(f"* {arm}: cells NOT ahead at n l H = {behind if behind else 'none'}; threshold = {t}.\n")
        f.write("\n`pair_attn.PAIR_MIN_PAIRS_X3` (sigmoid) and `pair_attn.SOFTMAX_MIN_PAIRS_X3` hold these two numbers.\n")
        if regs:
            f.write("\n## Registers (the compiler's resource summary, gfx950)\n\n| kernel | VGPRs | AGPRs | spilled | scratch B/lane | "
                    "waves/SIMD | LDS B |\n|---|---|---|---|---|---|---|\n")
            for r in regs:
                f.write("| " + " | ".join(str(x) for x in r) + " |\n")
            f.write("\n" + ("No instantiation spills: widths 32, 64 and 128 are all supported.\n" if not any(r[3] or r[4] for r in regs)
                           else "SPILLS: see the table.\n"))
        if worst:
            f.write("\n## Worst error / bar of tests/test_gpu_pair_x3.py\n\n| check | worst ratio | case |\n|---|---|---|\n")
            for kind in sorted(worst):
                f.write(f"| {kind} | {worst[kind][0]:.4f} | {worst[kind][1]} |\n")
            f.write("\nThe gradient rows of `large`, `moving32`, `moving64` and of the random cases at scale 1 are printed, not "
                    "asserted (those tests assert the forward bar and finite gradients); every other row is asserted at 1.\n")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_x3_probe.md"))
    ap.add_argument("--ratios", default=None, help="output of `pytest -s tests/test_gpu_pair_x3.py` (X3_RATIO lines)")
    ap.add_argument("--cells", default=None, help="the JSON line of an earlier run: rewrite the report, measure nothing")
    ap.add_argument("--resources", default=None, help="the compiler's kernel-resource-usage remarks for csrc/pair_attn.hip")
    ap.add_argument("--json", default=None, help="keep the cells measured so far in this file (rewritten after every cell)")
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--heads", default=",".join(str(s) for s in HEADS))
    ap.add_argument("--widths", default=",".join(str(s) for s in WIDTHS))
    args = ap.parse_args()
    if args.cells:
        cells = json.loads([ln for ln in open(args.cells) if ln.startswith("{")][-1])["cells"]
    else:
        dev = torch.device("cuda:0")
        os.environ["SGF_PAIR_ATTN"] = os.environ["SGF_PAIR_SOFTMAX"] = "1"
        for arm in ARMS:
            names = launches(arm, dev)
            assert names == [f"sgf_pair_{arm}_x3_{w}" for w in ("fwd", "bwd_q", "bwd_kv")], names
        cells = []
        for arm in ARMS:
            for n in (int(s) for s in args.sizes.split(",")):
                for h in (int(s) for s in args.heads.split(",")):
                    for d in (int(s) for s in args.widths.split(",")):
                        r = cell(arm, n, h, d, dev)
                        tf, tb = r["fwd"], r["fwdbwd"]
                        kf, kb = statistics.median(tf["x3"]), statistics.median(tb["x3"])
                        pairs = n * n * h
                        c = dict(arm=arm, n=n, heads=h, d=d, pairs=pairs, tflops_fwd=4 * pairs * d / (kf * 1e-3) / 1e12,
                                 tflops_bwd=14 * pairs * d / (max(kb - kf, 1e-6) * 1e-3) / 1e12)
                        for p in PATHS:
                            c["fwd_" + p], c["fwdbwd_" + p] = tf[p], tb[p]
                        cells.append(c)
                        print(f"{arm} n={n} H={h} D={d}: fwd {fmt(tf['x3'])} / {fmt(tf['exact'])} / {fmt(tf['dense'])}, "
                              f"fwd+bwd {fmt(tb['x3'])} / {fmt(tb['exact'])} / {fmt(tb['dense'])}", flush=True)
                        if args.json:
                            with open(args.json, "w") as f:
                                f.write(json.dumps(dict(probe="pair_x3", cells=cells)) + "\n")
    res = report(cells, ratios(args.ratios), args.out, resources(args.resources))
    print(json.dumps(dict(probe="pair_x3", thresholds=res, cells=cells)))


if __name__ == "__main__":
    main()
