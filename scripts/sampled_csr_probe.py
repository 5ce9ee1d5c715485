#!/usr/bin/env python
"""What the sampled batch's CSR costs, old path against new, on the batches of the 100M recipe (100M/nb-sample.py: 1000 seeds,
num_neighbors [15, 10, 5]; also [25, 10]) drawn from the graph of scripts/sampler_probe.py (synth.SHAPES['papers100M-shard8'],
uniform random).  Per fan-out list, on the SAME batches in the SAME process, legs alternating batch by batch, HIP events:
  (a)  K.csr_build + K.csr_transpose on the batch edge list (sgf_csr_build / sgf_csr_transpose: the path SGF_SAMPLED_CSR=0
       keeps) — with the `.item()` of the symmetry flag and without it;
  (b)  K.sampled_csr_build + K.sampled_csr_transpose (sgf_sampled_csr_*) on the capacity-sized buffers the sampler hands over;
and the eager training step of sampler_probe.py (sample, gather, forward, loss, backward, Adam) with SGF_SAMPLED_CSR=1 and =0,
on the same batches (fixed seeds and batch ids), the two legs alternating in order from pass to pass.  Every figure is a median with the min and max over the timed batches (the run-to-run spread).  Before
timing, the two legs' arrays are compared bit for bit on every timed batch.  Writes a markdown report and prints one JSON line.
One process, no retries: run it under one time limit, e.g.
    timeout -k 10 1100 python scripts/sampled_csr_probe.py [--nodes N] [--batches 24] [--out profiles/sampled_csr_probe.md]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgformer_amd import _lib, ops, synth  # noqa: E402
from sgformer_amd.kernels import HipKernels as K, _ptr, _stream  # noqa: E402
from sgformer_amd.ours_100m import SGFormer  # noqa: E402
from sgformer_amd.sampling import NeighborLoader, NeighborSampler  # noqa: E402


def old_transpose_no_read(ei, n, deg, rowptr, colind):
    """K.csr_transpose without the host read of its symmetry flag (the flag stays on the device)."""
    dev, nnz = ei.device, int(ei.shape[1])
    t_rowptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    t_colind = torch.empty(nnz, dtype=torch.int32, device=dev)
    t_val = torch.empty(nnz, dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(_lib.load().sgf_csr_workspace_bytes(nnz, n), 256), dtype=torch.uint8, device=dev)
    _lib.call("sgf_csr_transpose", _ptr(ei), nnz, n, _ptr(deg), _ptr(rowptr), _ptr(colind), _ptr(t_rowptr), _ptr(t_colind),
              _ptr(t_val), _ptr(flag), _ptr(ws), ws.numel(), _stream(dev))
    return t_rowptr, t_colind, t_val, flag


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "n": len(ms)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    return a, b, out


def csr_legs(sampler, seeds_of, batches, warmup, dev):
    fan = sampler.fanouts
    lib = _lib.load()
    ncap, ecap = ctypes.c_int64(0), ctypes.c_int64(0)
    fan_host = (ctypes.c_int32 * len(fan))(*fan)
    lib.sgf_neighbor_sample_batch_workspace_bytes(len(seeds_of(0)), fan_host, len(fan), ctypes.byref(ncap), ctypes.byref(ecap))
    ncap, ecap = ncap.value, ecap.value
    legs = {"a_with_item": [], "a_without_item": [], "b_new": []}
    nodes = edges = 0
    for b in range(warmup + batches):
        n_id, e, _ = sampler.sample(seeds_of(b), batch_id=b)
        nn, ne = int(n_id.numel()), int(e.shape[1])
        # what the sampler hands sgf_sampled_csr_build: capacity-sized int32 edge arrays and the device counts
        e_src = torch.zeros(max(ecap, 1), dtype=torch.int32, device=dev)
        e_dst = torch.zeros(max(ecap, 1), dtype=torch.int32, device=dev)
        e_src[:ne], e_dst[:ne] = e[0], e[1]
        counts = torch.tensor([nn, ne], dtype=torch.int64, device=dev)
        e = e.clone()                                    # (a plain edge list: no attributes)

        def leg_a(read):
            rowptr, colind, val, deg = K.csr_build(e, nn)
            if read:
                return (rowptr, colind, val, deg) + K.csr_transpose(e, nn, deg, rowptr, colind)[:3]
            return (rowptr, colind, val, deg) + old_transpose_no_read(e, nn, deg, rowptr, colind)[:3]

        def leg_b():
            rowptr_b, colind_b, val_b, deg_b = K.sampled_csr_build(e_src, e_dst, counts, ncap, ecap, max(fan))
            rp, ci, va = rowptr_b[:nn + 1], colind_b[:ne], val_b[:ne]
            return (rp, ci, va, deg_b[:nn]) + K.sampled_csr_transpose(rp, ci, va, nn)

        torch.cuda.synchronize()
        evs = []
        order = [("a_with_item", lambda: leg_a(True)), ("b_new", leg_b), ("a_without_item", lambda: leg_a(False))]
        for name, fn in order[b % 3:] + order[:b % 3]:   # the legs take turns at going first
            s, t, out = timed(fn)
            evs.append((name, s, t, out))
        torch.cuda.synchronize()
        want = next(out for name, _, _, out in evs if name == "a_with_item")
        for name, _, _, out in evs:                      # same results, at the size that is timed
            for x, y in zip(out, want):
                if not torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                   y.view(torch.int32) if y.dtype == torch.float32 else y):
                    raise SystemExit(f"leg {name} differs from sgf_csr_build / sgf_csr_transpose on batch {b}")
        if b >= warmup:
            for name, s, t, _ in evs:
                legs[name].append(s.elapsed_time(t))
            nodes += nn
            edges += ne
    return {k: stats(v) for k, v in legs.items()}, nodes / batches, edges / batches, ncap, ecap


def step_legs(data, fan, a, dev, dt, f, c, d, seeds_of):
    """The eager training step of sampler_probe.py — sample, gather, forward, loss, backward, Adam — on the SAME batches with
    the switch on and off: fixed seed sets and batch ids (the draw is a hash of seed / batch / hop / node), so that pass after
    pass every step sees the batch it saw before; the order of the two legs alternates from pass to pass."""
    loader = NeighborLoader(data, input_nodes=torch.arange(0, a.batch), num_neighbors=fan, batch_size=a.batch,
                            shuffle=False, seed=7, feature_dtype=dt)
    model = SGFormer(f, d, c, trans_dropout=0.0, gnn_dropout=0.0, compute_dtype=dt, **synth.RECIPES["papers100M-shard8"]).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    loss_fn = torch.nn.CrossEntropyLoss()
    res = {"on": [], "off": []}
    wall = {"on": [], "off": []}
    for rnd in range(5):                                 # pass 0: warm-up of both paths
        for flag in (("on", "off") if rnd % 2 == 0 else ("off", "on")):
            os.environ["SGF_SAMPLED_CSR"] = "1" if flag == "on" else "0"
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(a.batches + 1)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            evs[0].record()
            for b in range(a.batches):
                n_id, ei_b, bs = loader.sampler.sample(seeds_of(a.warmup + b), batch_id=a.warmup + b)
                x_b, y_b = ops.gather_rows(loader.x, n_id), loader.y[n_id]
                out = model(x_b, ei_b)[:bs]
                loss = loss_fn(out.float(), y_b[:bs])
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
                evs[b + 1].record()
            torch.cuda.synchronize()
            if rnd > 0:
                wall[flag].append((time.perf_counter() - t0) / a.batches * 1e3)
                res[flag] += [evs[i].elapsed_time(evs[i + 1]) for i in range(a.batches)]
    os.environ.pop("SGF_SAMPLED_CSR", None)
    return {k: stats(v) for k, v in res.items()}, {k: [round(x, 3) for x in v] for k, v in wall.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=0)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--batches", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampled_csr_probe.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampled_csr_probe: needs the GPU (no timing without one)")
    if a.batches < 20:
        raise SystemExit("sampled_csr_probe: at least 20 timed batches")
    dev = torch.device("cuda:0")
    n, deg, f, c, d = synth.SHAPES["papers100M-shard8"]
    n = a.nodes or n
    ei = synth.synthetic_graph(n, deg, seed=123, device=dev)
    x, y, _ = synth.synthetic_task(n, f, c, seed=123, device=dev)
    dt = None if a.dtype == "f32" else torch.bfloat16

    class Data:
        pass
    data = Data()
    data.x, data.y, data.edge_index = x, y, ei
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(n, generator=g)[: a.batch * (a.batches + a.warmup)].to(dev)
    report = {"graph": f"uniform random, {n} nodes, {int(ei.shape[1])} stored entries", "seeds_per_batch": a.batch,
              "timed_batches": a.batches, "dtype": a.dtype, "device": torch.cuda.get_device_name(0), "fanouts": {}}
    for fan in ([15, 10, 5], [25, 10]):
        sampler = NeighborSampler(ei, n, fan, seed=7, device=dev)
        os.environ["SGF_SAMPLED_CSR"] = "0"              # the timed legs build their own arrays
        legs, nn, ne, ncap, ecap = csr_legs(sampler, lambda b: perm[b * a.batch:(b + 1) * a.batch], a.batches, a.warmup, dev)
        os.environ.pop("SGF_SAMPLED_CSR", None)
        ops.graph_cache.clear()
        step, wall = step_legs(data, fan, a, dev, dt, f, c, d, lambda b: perm[b * a.batch:(b + 1) * a.batch])
        lower = legs["b_new"]["max"] < min(legs["a_with_item"]["min"], legs["a_without_item"]["min"])
        report["fanouts"][str(fan)] = {"nodes_per_batch": round(nn), "edges_per_batch": round(ne), "node_cap": ncap, "edge_cap": ecap,
                                       "csr_ms": legs, "step_ms": step, "step_wall_ms_per_batch_by_pass": wall,
                                       "b_lower_than_a_beyond_the_spread": bool(lower)}
    lines = ["# Sampled batches: the CSR and its transpose, old path against new (scripts/sampled_csr_probe.py)", "",
             f"{report['device']}; {report['graph']}; {a.batch} seeds per batch; {a.batches} timed batches after {a.warmup} of "
             f"warm-up; model storage {a.dtype}.  HIP events, the legs alternating batch by batch on the same batches in one "
             "process (CSR legs: the order rotates batch by batch; steps: fixed seed sets and batch ids, four timed passes per leg, the "
             "order alternating); every cell is `median (min .. max)` in ms over the timed batches.  The arrays of all legs were compared "
             "bit for bit on every batch before a time was kept.", ""]
    for fan, r in report["fanouts"].items():
        cell = lambda s: f"{s['median']:.3f} ({s['min']:.3f} .. {s['max']:.3f})"      # noqa: E731
        lines += [f"## num_neighbors = {fan}", "",
                  f"{r['nodes_per_batch']} nodes and {r['edges_per_batch']} edges per batch (capacities {r['node_cap']} / {r['edge_cap']}).", "",
                  "| leg | ms per batch |", "|---|---|",
                  f"| (a) `sgf_csr_build` + `sgf_csr_transpose`, with the `.item()` of the symmetry flag | {cell(r['csr_ms']['a_with_item'])} |",
                  f"| (a) the same without the `.item()` | {cell(r['csr_ms']['a_without_item'])} |",
                  f"| (b) `sgf_sampled_csr_build` + `sgf_sampled_csr_transpose` | {cell(r['csr_ms']['b_new'])} |",
                  f"| eager training step, `SGF_SAMPLED_CSR=1` | {cell(r['step_ms']['on'])} |",
                  f"| eager training step, `SGF_SAMPLED_CSR=0` | {cell(r['step_ms']['off'])} |", "",
                  f"Host clock per batch, pass by pass (on / off alternating): on {r['step_wall_ms_per_batch_by_pass']['on']}, "
                  f"off {r['step_wall_ms_per_batch_by_pass']['off']}.", "",
                  "(b) is lower than (a) by more than the spread (max of (b) below min of (a)): "
                  + ("**yes**" if r["b_lower_than_a_beyond_the_spread"] else "**no**") + ".", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print(json.dumps(report))


if __name__ == "__main__":
    main()
