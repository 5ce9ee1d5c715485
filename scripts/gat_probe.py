"""Timing probe of the edge-softmax kernels (csrc/gat.hip) -> profiles/gat_probe.md.

    python scripts/gat_probe.py [--nodes 100000 1000000] [--reps 7] [--out gat_probe.json]

Per graph (the uniform and the community synthetic graphs of benchlib/workloads.py, average degree 16, plus the self-loops
GATConv adds), shape (H, C) and storage dtype, on one GPU, each figure the median (min .. max) of `--reps` timed repetitions
after 3 warm-up ones, in milliseconds between two stream events:
    per kernel   sgf_gat_scores / _fwd / _bwd_dst / _bwd_src, and the ATen column sums of datt_l, datt_r, dbias
    per layer    gat.gat_aggregate forward and forward + backward, against (a) gat.edge_list_aggregate on the same device and
                 (b) sgf_spmm on the same CSR at d = H C (the floor of the gathering kernels), with (c) the peak memory over the
                 operands of both paths
One process per run; run it several times for the spread between processes."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sgformer_amd import gat, ops, synth  # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return [statistics.median(ms), min(ms), max(ms)]


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for n in args.nodes:
        for kind, gen in (("uniform", synth.synthetic_graph), ("community", synth.synthetic_graph_community)):
            ei = gat._with_self_loops(gen(n, 16.0, seed=1, device=dev), n)
            graph = ops.CSRGraph(ei, n)
            graph.transposed()
            for h, c in ((8, 64), (1, 64)):
                for dtype in (torch.float32, torch.bfloat16):
                    torch.manual_seed(0)
                    xw = torch.randn(n, h * c, device=dev).to(dtype).requires_grad_(True)
                    att_l = (torch.randn(1, h, c, device=dev) * 0.3).requires_grad_(True)
                    att_r = (torch.randn(1, h, c, device=dev) * 0.3).requires_grad_(True)
                    bias = torch.zeros(h * c, device=dev, requires_grad=True)
                    g = torch.randn(n, h * c, device=dev).to(dtype)
                    t = gat._Hip
                    wl, wr = att_l.detach().reshape(-1), att_r.detach().reshape(-1)
                    x = xw.detach()
                    al, ar = t.gat_scores(x, wl, wr, h)
                    out, lse, norm = t.gat_fwd(graph.rowptr, graph.colind, x, al, ar, bias.detach(), h, False, 0.2, 0.0, 0)
                    delta, dar = t.gat_bwd_dst(graph.rowptr, graph.colind, g, x, al, ar, norm, h, False, 0.2, 0.0, 0)
                    tr, tc = graph.transposed()[:2]
                    dal, _ = t.gat_bwd_src(tr, tc, g, x, al, ar, norm, delta, dar, wl, wr, h, False, 0.2, 0.0, 0)
                    x3 = x.view(n, h, c).float()
                    r = dict(nodes=n, graph=kind, nnz=graph.nnz, heads=h, c=c, dtype=str(dtype).split(".")[1])
                    r["scores"] = timed(lambda: t.gat_scores(x, wl, wr, h), args.reps)
                    r["fwd"] = timed(lambda: t.gat_fwd(graph.rowptr, graph.colind, x, al, ar, bias.detach(), h, False, 0.2, 0.0, 0),
                                     args.reps)
                    r["fwd_drop"] = timed(lambda: t.gat_fwd(graph.rowptr, graph.colind, x, al, ar, bias.detach(), h, False, 0.2,
                                                            0.5, 12345), args.reps)
                    r["bwd_dst"] = timed(lambda: t.gat_bwd_dst(graph.rowptr, graph.colind, g, x, al, ar, norm, h, False, 0.2, 0.0,
                                                               0), args.reps)
                    r["bwd_src"] = timed(lambda: t.gat_bwd_src(tr, tc, g, x, al, ar, norm, delta, dar, wl, wr, h, False, 0.2, 0.0,
                                                               0), args.reps)
                    r["aten_param_grads"] = timed(lambda: (torch.einsum("nh,nhc->hc", dal, x3), torch.einsum("nh,nhc->hc", dar, x3),
                                                           g.float().sum(0)), args.reps)
                    r["spmm"] = timed(lambda: ops.spmm(graph, x), args.reps)

                    def layer(fn, backward):
                        def run():
                            o = fn()
                            if backward:
                                torch.autograd.grad(o, (xw, att_l, att_r, bias), g)
                        return run
                    kern = lambda: gat.gat_aggregate(graph, xw, att_l, att_r, bias=bias)
                    edge = lambda: gat.edge_list_aggregate(ei, n, xw, att_l.to(dtype), att_r.to(dtype), bias=bias)
                    r["layer_fwd"], r["layer_fwd_bwd"] = timed(layer(kern, False), args.reps), timed(layer(kern, True), args.reps)
                    r["layer_mib"] = peak(layer(kern, True))
                    try:
                        r["edge_fwd"], r["edge_fwd_bwd"] = timed(layer(edge, False), args.reps), timed(layer(edge, True), args.reps)
                        r["edge_mib"] = peak(layer(edge, True))
                    except torch.cuda.OutOfMemoryError:
                        r["edge_fwd"] = r["edge_fwd_bwd"] = r["edge_mib"] = None
                        torch.cuda.empty_cache()
                    print(json.dumps(r), flush=True)
                    rows.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f)


if __name__ == "__main__":
    main()
