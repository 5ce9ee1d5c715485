#!/usr/bin/env python
"""What the head on the seed rows buys the neighbour-sampled step (100M/nb-sample.py: 1000 seeds, num_neighbors [15, 10, 5];
also [25, 10]) on the graph of scripts/sampled_csr_probe.py (synth.SHAPES['papers100M-shard8'], uniform random), the 100M
recipe with its dropout, d = 128, C = 172, bf16 storage.  The trainer's lines as they are written —
    output = model(graph.x, graph.edge_index)[:batch_size];  loss = nn.CrossEntropyLoss()(output, graph.y[:batch_size])
— with launch.patch_ce_loss() installed, per fan-out list on the SAME batches in the SAME process, HIP events:
  (a)  SGF_SEED_HEAD=0: the full head, ATen's slice and loss;
  (b)  SGF_SEED_HEAD=1: the lazy head, sgf_head_rows_fwd / _bwd on the seed rows.
Each batch is sampled once; then, before any time is kept, both legs run forward + backward from the same parameters and the
same torch seed (the same dropout masks) and their loss and parameter gradients are compared; then each leg runs one timed
training step (forward, loss, backward, Adam step) and one timed evaluation forward (eval mode, no_grad, `[:k].argmax(-1) ==
y[:k]`), the leg that goes first alternating batch by batch.  Every figure is `median (min .. max)` over the timed batches.
The launches of one step per leg are counted afterwards with torch.profiler, in a pass of its own.  Writes a markdown report
and prints one JSON line.  One process, no retries: run it under one time limit, e.g.
    timeout -k 10 900 python scripts/seed_head_probe.py [--nodes N] [--batches 20] [--out profiles/seed_head_probe.md]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgformer_amd import launch, ops, synth  # noqa: E402
from sgformer_amd.ours_100m import SGFormer  # noqa: E402
from sgformer_amd.sampling import NeighborLoader  # noqa: E402

LEGS = (("a", "0"), ("b", "1"))
# NOT the bound of the model test (tests/test_gpu_head_rows.py: each leg against the fp64 oracle, new <= 2 x old + 1e-6 gmax):
# there is no oracle at 756 000 nodes, so the legs are compared with each other, under a LOOSER bound of this script's own.
# Per tensor: 8 bf16 roundings (2^-9 each) of |g|, times the batch's largest logit where that exceeds 1, plus one bf16
# rounding of the largest gradient norm — the floor for tensors whose exact gradient is zero (a Linear bias in front of a
# BatchNorm), where both legs hold rounding noise only.  It catches a wrong row, label or scale, not a last-digit difference.
PARITY_REL, PARITY_ABS = 8 * 2.0 ** -9, 2.0 ** -9


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "n": len(ms)}


def trainer_lines(model, x, ei, y, bs, loss_fn):
    output = model(x, ei)[:bs]
    return loss_fn(output, y[:bs])


def parity(model, x, ei, y, bs, loss_fn, b):
    got = {}
    scale = 1.0
    for name, flag in LEGS:
        os.environ["SGF_SEED_HEAD"] = flag
        torch.manual_seed(1000 + b)
        model.zero_grad(set_to_none=True)
        output = model(x, ei)[:bs]
        loss = loss_fn(output, y[:bs])
        loss.backward()
        got[name] = (loss.detach().float(), {k: p.grad.detach().float().clone() for k, p in model.named_parameters() if p.grad is not None})
        if name == "b":                  # a rounding of a logit is relative to the logit: the bound scales with the largest one
            scale = max(1.0, float(output.detach().float().abs().max()))
    (la, ga), (lb, gb) = got["a"], got["b"]
    if not abs(float(la) - float(lb)) <= PARITY_REL * scale * max(1.0, abs(float(la))):
        raise SystemExit(f"batch {b}: loss (a) {float(la)} against (b) {float(lb)} (largest logit {scale})")
    gmax = max(float(g.norm()) for g in ga.values())
    worst = 0.0
    for k, g in ga.items():
        diff = float((gb[k] - g).norm())
        if not diff <= PARITY_REL * scale * float(g.norm()) + PARITY_ABS * gmax:
            raise SystemExit(f"batch {b}: gradient of {k} differs by {diff} (norm {float(g.norm())}, gmax {gmax}, largest logit {scale})")
        if float(g.norm()) > 1e-3 * gmax:
            worst = max(worst, diff / float(g.norm()))
    return abs(float(la) - float(lb)), worst


def count_launches(fn):
    """(kernels, memsets and copies) the device ran for one call of fn, or None where the profiler gives nothing."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
        other = [e for e in dev if e.name.lower().startswith(("memset", "memcpy"))]
        return (len(dev) - len(other), len(other)) if dev else None
    except Exception as e:  # noqa: BLE001  (a profiler that is not there must not cost the timings)
        print(f"seed_head_probe: launch count not measured ({type(e).__name__}: {e})", file=sys.stderr)
        return None


def run_fanout(data, fan, a, dev, f, c, d, seeds_of):
    loader = NeighborLoader(data, input_nodes=torch.arange(0, a.batch), num_neighbors=fan, batch_size=a.batch, shuffle=False,
                            seed=7, feature_dtype=torch.bfloat16)
    p_trans, p_gnn = synth.RECIPE_DROPOUT["papers100M-shard8"]
    torch.manual_seed(0)
    model = SGFormer(f, d, c, trans_dropout=p_trans, gnn_dropout=p_gnn, compute_dtype=torch.bfloat16,
                     **synth.RECIPES["papers100M-shard8"]).to(dev)
    model.logits_dtype = torch.float32
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    loss_fn = torch.nn.CrossEntropyLoss()
    step_ms, eval_ms = {"a": [], "b": []}, {"a": [], "b": []}
    nodes, dl_max, dg_max, hits = 0, 0.0, 0.0, {"a": 0, "b": 0}
    last = None
    for b in range(a.warmup + a.batches):
        n_id, ei, bs = loader.sampler.sample(seeds_of(b), batch_id=b)
        x, y = ops.gather_rows(loader.x, n_id), loader.y[n_id]
        model.train()
        dl, dg = parity(model, x, ei, y, bs, loss_fn, b)
        order = LEGS if b % 2 == 0 else LEGS[::-1]
        evs = {}
        model.train()
        for name, flag in order:
            os.environ["SGF_SEED_HEAD"] = flag
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            loss = trainer_lines(model, x, ei, y, bs, loss_fn)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            s1.record()
            evs[name] = [s0, s1]
        model.eval()                     # both evaluation legs see the same parameters: their hit counts can be compared
        with torch.no_grad():
            for name, flag in order:
                os.environ["SGF_SEED_HEAD"] = flag
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = model(x, ei)[:bs]
                n_hit = (out.argmax(dim=-1) == y[:bs]).sum()
                e1.record()
                evs[name] += [e0, e1, n_hit]
        torch.cuda.synchronize()
        if b >= a.warmup:
            for name, (s0, s1, e0, e1, n_hit) in evs.items():
                step_ms[name].append(s0.elapsed_time(s1))
                eval_ms[name].append(e0.elapsed_time(e1))
                hits[name] += int(n_hit)
            nodes += int(n_id.numel())
            dl_max, dg_max = max(dl_max, dl), max(dg_max, dg)
        last = (x, ei, y, bs)
    launches = {}
    x, ei, y, bs = last
    model.train()
    for name, flag in LEGS:
        os.environ["SGF_SEED_HEAD"] = flag

        def one_step():
            loss = trainer_lines(model, x, ei, y, bs, loss_fn)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        one_step()
        launches[name] = count_launches(one_step)
    os.environ.pop("SGF_SEED_HEAD", None)
    return {"nodes_per_batch": round(nodes / a.batches), "step_ms": {k: stats(v) for k, v in step_ms.items()},
            "eval_ms": {k: stats(v) for k, v in eval_ms.items()}, "launches": launches, "eval_hits": hits,
            "parity_max_loss_diff": dl_max, "parity_max_rel_grad_diff": dg_max,
            "b_below_a_beyond_the_spread": bool(max(step_ms["b"]) < min(step_ms["a"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=0)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seed_head_probe.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seed_head_probe: needs the GPU (no timing without one)")
    if a.batches < 20:
        raise SystemExit("seed_head_probe: at least 20 timed batches")
    dev = torch.device("cuda:0")
    n, deg, f, c, d = synth.SHAPES["papers100M-shard8"]
    n = a.nodes or n
    ei = synth.synthetic_graph(n, deg, seed=123, device=dev)
    x, y, _ = synth.synthetic_task(n, f, c, seed=123, device=dev)

    class Data:
        pass
    data = Data()
    data.x, data.y, data.edge_index = x, y, ei
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))[: a.batch * (a.batches + a.warmup)].to(dev)
    launch.patch_ce_loss()
    report = {"graph": f"uniform random, {n} nodes, {int(ei.shape[1])} stored entries", "seeds_per_batch": a.batch,
              "timed_batches": a.batches, "device": torch.cuda.get_device_name(0), "fanouts": {}}
    for fan in ([15, 10, 5], [25, 10]):
        ops.graph_cache.clear()
        report["fanouts"][str(fan)] = run_fanout(data, fan, a, dev, f, c, d, lambda b: perm[b * a.batch:(b + 1) * a.batch])
    launch.unpatch_ce_loss()
    on = all(r["b_below_a_beyond_the_spread"] for r in report["fanouts"].values())
    report["default"] = "1" if on else "0"
    cell = lambda s: f"{s['median']:.3f} ({s['min']:.3f} .. {s['max']:.3f})"      # noqa: E731
    count = lambda v: "not measured" if v is None else f"{v[0]} kernels + {v[1]} memsets / copies"      # noqa: E731
    lines = ["# Sampled batches: the head on the seed rows, switch off against switch on (scripts/seed_head_probe.py)", "",
             f"{report['device']}; {report['graph']}; {a.batch} seeds per batch; {a.batches} timed batches after {a.warmup} of "
             f"warm-up; the 100M recipe with its dropout, d = {d}, C = {c}, bf16 storage, fp32 logits.  HIP events; each batch is "
             "sampled once and both legs run on it in the same process, the leg that goes first alternating batch by batch; every "
             "cell is `median (min .. max)` in ms over the timed batches.  The training step is forward, loss, backward and the Adam "
             "step on the sampled batch (sampling and the feature gather are the same for both legs and are not in it); the "
             "evaluation forward is `model.eval()`, `no_grad`, `[:k].argmax(-1) == y[:k]`.  Before a time was kept, loss and every "
             f"parameter gradient of the two legs were compared with each other on every batch, from the same parameters and dropout "
             f"masks.  This is not the bound of the model test (each leg against the fp64 oracle, new <= 2 x old + 1e-6 gmax): no "
             f"oracle runs at this size, and the bound used here is a different, looser one — per tensor {PARITY_REL:.4f} max(1, "
             f"largest logit) |g| + {PARITY_ABS:g} gmax; the largest differences seen are given under each table.  Launches: one training step per leg under torch.profiler, "
             "in a pass of its own.", ""]
    for fan, r in report["fanouts"].items():
        lines += [f"## num_neighbors = {fan}", "", f"{r['nodes_per_batch']} nodes per batch.", "",
                  "| leg | training step, ms | evaluation forward, ms | launches per training step |", "|---|---|---|---|",
                  f"| (a) `SGF_SEED_HEAD=0` | {cell(r['step_ms']['a'])} | {cell(r['eval_ms']['a'])} | {count(r['launches']['a'])} |",
                  f"| (b) `SGF_SEED_HEAD=1` | {cell(r['step_ms']['b'])} | {cell(r['eval_ms']['b'])} | {count(r['launches']['b'])} |", "",
                  f"Largest difference between the legs over the timed batches: loss {r['parity_max_loss_diff']:.3e}, parameter "
                  f"gradients {r['parity_max_rel_grad_diff']:.3e} of their norm (tensors above 1e-3 gmax).  Evaluation hits over the timed batches: "
                  f"(a) {r['eval_hits']['a']}, (b) {r['eval_hits']['b']} of {a.batch * a.batches} (the same parameters for both; (a) rounds its "
                  "logits to bf16, (b) keeps them in fp32, so a near-tie can fall either way).", "",
                  "The training step of (b) is below (a) by more than the spread (max of (b) below min of (a)): "
                  + ("**yes**" if r["b_below_a_beyond_the_spread"] else "**no**") + ".", ""]
    lines += ["## Default", "",
              "The rule: `SGF_SEED_HEAD` is on by default if the max of (b) is below the min of (a) on both fan-out lists, otherwise "
              f"off.  By these tables the default is **{'on (1)' if on else 'off (0)'}**.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print(json.dumps(report))


if __name__ == "__main__":
    main()
