#!/usr/bin/env python
"""Dropout under hipGraph replay, measured (profiles/graphed_dropout_probe.md).  One leg per fresh process, one JSON line each:

  --leg kernel            sgf_dropout (seed as a launch argument) against sgf_dropout_dev (seed read from device memory) on
                          [100000, 256] rows with a residual, bf16 and fp32, calls alternating, device events per call
  --leg eager  --drop T,G a main-batch.py-shaped training step (100 k-node induced batches of a 400 k-node graph, the
  --leg replay --drop T,G ogbn-products recipe, d = 256, bf16, Adam) with trans_dropout T / gnn_dropout G, issued launch by
                          launch (SGF_GRAPH_DROPOUT=0) or replayed; host clock around each step, ending in a synchronise,
                          and around windows of 10 steps with one synchronise behind the last (as the trainer issues them)

  --report FILE           the markdown tables of profiles/graphed_dropout_probe.md from the legs' JSON lines
                          (profiles/graphed_dropout_probe.jsonl); the reading below the tables is written by hand

The eager leg imports nothing newer than sgformer_amd.graphed.counters, so the same file times a checkout of an earlier
commit (where active dropout always meant eager).  Medians with (min .. max) over the timed steps after the warm-up."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "count": len(xs)}


def kernel_leg(args):
    import torch
    from sgformer_amd import ops
    K = ops.K
    dev = torch.device("cuda:0")
    n, d, p, seed = 100000, 256, 0.5, 2 ** 40 + 12345
    out = {"leg": "kernel", "n": n, "d": d, "p": p, "device": torch.cuda.get_device_name(0)}
    seeds = torch.tensor([1, seed, 3, 4], dtype=torch.int64, device=dev)
    for name, dtype in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        g = torch.Generator().manual_seed(0)
        x = torch.randn(n, d, generator=g).to(dtype).to(dev)
        res = torch.randn(n, d, generator=g).to(dtype).to(dev)
        calls = {"imm": lambda: K.dropout(x, res, p, seed), "dev": lambda: K.dropout_dev(x, res, p, seeds, 1)}
        assert torch.equal(calls["imm"](), calls["dev"]())
        times = {k: [] for k in calls}
        for it in range(args.warmup + args.steps):
            for k in (("imm", "dev") if it % 2 == 0 else ("dev", "imm")):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                calls[k]()
                b.record()
                b.synchronize()
                if it >= args.warmup:
                    times[k].append(a.elapsed_time(b) * 1e3)
        nbytes = 3 * n * d * x.element_size()
        out[name] = {k: dict(_summary(v), unit="us", tb_per_s=nbytes / (statistics.median(v) * 1e-6) / 1e12) for k, v in times.items()}
    print(json.dumps(out), flush=True)


def step_leg(args):
    replay = args.leg == "replay"
    pt, pg = (float(v) for v in args.drop.split(","))
    # eager with active dropout: what every earlier commit does by itself; with dropout 0 / 0 (the reference pair of legs:
    # replay as it was before dropout could be captured) the eager leg has to switch the replays off
    os.environ["SGF_BATCH_GRAPH"] = "1" if (replay or pt > 0 or pg > 0) else "0"
    os.environ["SGF_GRAPH_DROPOUT"] = "1" if replay else "0"
    import torch
    import torch.nn.functional as F
    from sgformer_amd import batching, graphed, launch, synth
    from sgformer_amd.ours import SGFormer
    dev = torch.device("cuda:0")
    n, f, c, d, m = 400000, 100, 47, 256, 100000
    ei = synth.synthetic_graph(n, 51.5, seed=1, device=dev)
    x, y, _ = synth.synthetic_task(n, f, c, seed=1)
    x, y = x.to(dev), y.to(dev)
    torch.manual_seed(0)
    model = SGFormer(f, d, c, trans_dropout=pt, gnn_dropout=pg, compute_dtype=torch.bfloat16, **synth.RECIPES["ogbn-products"]).to(dev)
    model.logits_dtype = torch.float32
    launch.patch_adam()
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    gen = torch.Generator().manual_seed(3)
    batches = []
    for _ in range(6):
        idx = torch.randperm(n, generator=gen)[:m].to(dev)
        ei_i, _ = batching.subgraph(idx, ei, num_nodes=n, relabel_nodes=True)
        batches.append((x[idx], ei_i, y[idx]))
    before = dict(graphed.counters)
    it = 0

    def step():
        nonlocal it
        xi, ei_i, yi = batches[it % len(batches)]
        it += 1
        model.train()
        opt.zero_grad()
        out = model(xi, ei_i)
        loss = F.nll_loss(F.log_softmax(out.float(), dim=1), yi)
        loss.backward()
        opt.step()
        return loss

    # (1) every step on its own: host clock from its first call to the synchronise behind its optimizer step
    times = []
    for k in range(args.warmup + args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        if k >= args.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    # (2) as the trainer runs them: WINDOW steps back to back, one synchronise behind the last (the host issues ahead)
    windows, loss = [], None
    for k in range(args.steps // args.window):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.window):
            loss = step()
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) * 1e3 / args.window)
    used = {k: graphed.counters[k] - before[k] for k in before}
    assert (used["replays"] > 0) == replay, used
    s, w = _summary(times), _summary(windows)
    print(json.dumps({"leg": args.leg, "drop": [pt, pg], "root": ROOT, "nodes": m, "d": d, "step_ms": s,
                      "window": args.window, "window_ms_per_step": w, "nodes_per_s": m / (w["median"] * 1e-3),
                      "overlap": os.environ.get("SGF_OVERLAP", "1"), "counters": used, "loss": float(loss.detach()),
                      "device": torch.cuda.get_device_name(0)}), flush=True)


def report(args):
    """Markdown from the legs' JSON lines (the file kept next to the report), every process a row of its own."""
    rows = [json.loads(line) for line in open(args.report) if line.startswith("{")]
    f = lambda s, nd=2: f"{s['median']:.{nd}f} ({s['min']:.{nd}f} .. {s['max']:.{nd}f})"
    out = ["# Dropout under hipGraph replay: kernel and step (scripts/graphed_dropout_probe.py)", "",
           f"{rows[0]['device']} (MI355X, gfx950).  One fresh process per row, the legs alternating; every cell is "
           "`median (min .. max)`.", "", "## (a) `sgf_dropout` against `sgf_dropout_dev`", "",
           "[100000, 256] rows with a residual, p = 0.5; device events around each call, the two entries alternating call by "
           "call in one process, 300 timed calls each after 30 of warm-up; outputs compared bit for bit first.  TB/s on "
           "3 n d element bytes at the median.", "",
           "| process | dtype | `sgf_dropout` (seed as a launch argument), us | TB/s | `sgf_dropout_dev` (seed read from device memory), us | TB/s |",
           "|---|---|---|---|---|---|"]
    for i, r in enumerate(r for r in rows if r["leg"] == "kernel"):
        for dt in ("bf16", "f32"):
            out.append(f"| {i + 1} | {dt} | {f(r[dt]['imm'], 1)} | {r[dt]['imm']['tb_per_s']:.2f} | {f(r[dt]['dev'], 1)} | {r[dt]['dev']['tb_per_s']:.2f} |")
    out += ["", "## (b) The training step", "",
            "100 000-node induced batches of a 400 000-node uniform graph (6 batches in turn), ogbn-products recipe, d = 256, "
            "bf16, Adam.  `step`: host clock around ONE step, a synchronise on both sides (60 steps after 10 of warm-up).  "
            "`window`: 10 steps back to back with one synchronise behind the last, per step (6 windows) — how the trainer "
            "issues them.  `parent`: the same script on a checkout of the commit before `sgf_dropout_dev`.  The final loss is the "
            "same number in every row of one dropout pair.", "",
            "| dropout (trans, gnn) | leg | tree | step, ms | window, ms per step | nodes/s (window) | captures / replays |",
            "|---|---|---|---|---|---|---|"]
    for r in rows:
        if r["leg"] == "kernel":
            continue
        leg = {"eager": "eager", "replay": "replayed"}[r["leg"]] + (", `SGF_OVERLAP=0` (one stream)" if r["overlap"] == "0" else "")
        tree = "parent" if os.path.basename(r["root"]) == "parent" else "this"
        out.append(f"| {r['drop'][0]:g}, {r['drop'][1]:g} | {leg} | {tree} | {f(r['step_ms'])} | {f(r['window_ms_per_step'])} | "
                   f"{r['nodes_per_s'] / 1e6:.1f} M | {r['counters']['captures']} / {r['counters']['replays']} |")
    print("\n".join(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--report", help="JSON lines of earlier legs: print the markdown report instead of measuring")
    ap.add_argument("--leg", choices=["kernel", "eager", "replay"])
    ap.add_argument("--drop", default="0.5,0.2")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--window", type=int, default=10)
    a = ap.parse_args()
    if a.report:
        report(a)
    elif a.leg is None:
        ap.error("--leg or --report")
    else:
        (kernel_leg if a.leg == "kernel" else step_leg)(a)
