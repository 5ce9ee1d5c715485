"""The reference side of the live-reference pins of tests/test_oracle.py and tests/test_host.py, and the fixtures that keep
them running where the reference is not mounted (run in the build container only):

    python oracle/live_golden.py          # -> tests/golden/live/*.npz

Each `record_*` executes the reference's model files unchanged (oracle/ref_shim.py) on the inputs the test defines and
returns what the test compares against: inputs, state_dicts and outputs in float64.  The tests check the oracle against
the stored fixture always and against a fresh recording as well when the reference is mounted.
(tests/golden/*.npz, oracle/make_golden.py, are the other, per-recipe fixtures.)
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_shim, sgformer_oracle as O  # noqa: E402

LIVE_DIR = os.path.join(ROOT, "tests", "golden", "live")

# the parametrisations of the tests (their ids are cfg0, cfg1, ... in this order)
LARGE_CFGS = [
    dict(trans_num_layers=1, gnn_num_layers=2, gnn_use_init=True, graph_weight=0.5, trans_use_act=False),
    dict(trans_num_layers=2, trans_num_heads=2, gnn_num_layers=1, aggregate="cat"),
    dict(trans_use_weight=False, trans_num_heads=2, gnn_use_weight=False, gnn_use_bn=False, trans_use_bn=False),
    dict(use_graph=False),
]
MEDIUM_CASES = [(dict(num_layers=1, alpha=0.5, graph_weight=0.8), 4),
                (dict(num_layers=2, num_heads=2, use_weight=False, aggregate="cat"), 2),
                (dict(num_layers=1, use_bn=False, use_residual=False), 3)]
DIFFORMER_CFGS = [dict(num_layers=2, num_heads=1),
                  dict(num_layers=1, num_heads=2, use_weight=False, graph_weight=0.3, use_source=True),
                  dict(num_layers=2, num_heads=2, use_graph=False, use_bn=False, use_residual=False)]


class _Data:
    def __init__(self, x, ei):
        self.graph = {"node_feat": x, "edge_index": ei}


def _sd(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _f64(fn):
    def run(*a, **k):
        torch.set_default_dtype(torch.float64)
        try:
            return fn(*a, **k)
        finally:
            torch.set_default_dtype(torch.float32)
    return run


@_f64
def record_large(cfg):
    """large/ours.py SGFormer: a training-mode and an eval-mode forward, each with the state_dict it ran on."""
    ref = ref_shim.load_reference("large")
    torch.manual_seed(3)
    n, f, d, c = 211, 18, 16, 5
    m = ref.SGFormer(f, d, c, trans_dropout=0.0, gnn_dropout=0.0, **cfg).double()
    x = torch.randn(n, f)
    ei = O.synthetic_graph(n, 6.0, seed=8)
    out = {"x": x, "edge_index": ei, "state/train": _sd(m)}
    m.train()
    out["out/train"] = m(x, ei).detach()
    m.eval()
    out["state/eval"] = _sd(m)
    out["out/eval"] = m(x, ei).detach()
    return out


@_f64
def record_medium(cfg, gcn_layers):
    """medium/ours.py SGFormer over medium/models.py GCN, training and eval mode."""
    ref = ref_shim.load_reference("medium")
    torch.manual_seed(5)
    n, f, d, c = 160, 22, 16, 6
    gnn = ref.models.GCN(f, d, d, num_layers=gcn_layers, dropout=0.0)
    m = ref.SGFormer(f, d, c, dropout=0.0, gnn=gnn, **cfg).double()
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k.endswith("bias"):
                v.normal_(0, 0.1)
    x = torch.randn(n, f)
    ei = O.synthetic_graph(n, 5.0, seed=9)[:, :-n]
    out = {"x": x, "edge_index": ei}
    for mode, training in (("train", True), ("eval", False)):
        m.train(training)
        out[f"state/{mode}"] = _sd(m)
        with torch.no_grad():
            out[f"out/{mode}"] = m(_Data(x, ei))
    return out


@_f64
def record_difformer(cfg):
    """medium/difformer.py DIFFormer (kernel='simple'), training mode."""
    ref = ref_shim.load_reference("difformer")
    torch.manual_seed(0)
    n, f, d, c = 150, 20, 16, 5
    m = ref.DIFFormer(f, d, c, dropout=0.0, **cfg).double()
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k.endswith("bias"):
                v.normal_(0, 0.1)
    x = torch.randn(n, f)
    ei = O.synthetic_graph(n, 5.0, seed=3)
    m.train()
    out = {"x": x, "edge_index": ei, "state/train": _sd(m)}
    with torch.no_grad():
        out["out/train"] = m(_Data(x, ei))
    return out


def record_state_dict(variant):
    """The freshly initialised state_dict (torch.manual_seed(0)) of the modules tests/test_host.py compares key for key."""
    torch.manual_seed(0)
    if variant == "medium":
        ref = ref_shim.load_reference("medium")
        m = ref.SGFormer(30, 16, 4, num_layers=1, gnn=ref.models.GCN(30, 16, 16, num_layers=4))
    else:
        ref = ref_shim.load_reference("difformer")
        m = ref.DIFFormer(30, 16, 4, num_layers=2, num_heads=2)
    return {"state": _sd(m)}


def path(name):
    return os.path.join(LIVE_DIR, name + ".npz")


def save(name, rec):
    """Nested dicts of tensors -> one .npz; the state_dict keys' order is kept in `meta`."""
    arrays, order = {}, {}
    for k, v in rec.items():
        if isinstance(v, dict):
            order[k] = list(v)
            for kk, t in v.items():
                arrays[f"{k}/{kk}"] = t.numpy()
        else:
            arrays[k] = v.numpy()
    arrays["meta"] = np.array(json.dumps(order))
    os.makedirs(LIVE_DIR, exist_ok=True)
    np.savez_compressed(path(name), **arrays)


def load(name):
    z = np.load(path(name), allow_pickle=False)
    order = json.loads(str(z["meta"]))
    rec = {k: torch.from_numpy(z[k]) for k in z.files if k != "meta" and k.split("/")[0] not in order}
    for k, keys in order.items():
        rec[k] = {kk: torch.from_numpy(z[f"{k}/{kk}"]) for kk in keys}
    return rec


def records(name, record, *args):
    """The stored fixture, and a fresh recording too when the reference is mounted."""
    out = [load(name)]
    if ref_shim.reference_available():
        out.append(record(*args))
    return out


def main():
    if not ref_shim.reference_available():
        raise SystemExit("reference not mounted: live fixtures can only be generated in the build container")
    for i, cfg in enumerate(LARGE_CFGS):
        save(f"large_cfg{i}", record_large(cfg))
    for i, (cfg, layers) in enumerate(MEDIUM_CASES):
        save(f"medium_cfg{i}", record_medium(cfg, layers))
    for i, cfg in enumerate(DIFFORMER_CFGS):
        save(f"difformer_cfg{i}", record_difformer(cfg))
    for variant in ("medium", "difformer"):
        save(f"state_dict_{variant}", record_state_dict(variant))
    for f in sorted(os.listdir(LIVE_DIR)):
        print(f"{os.path.join(LIVE_DIR, f)}: {os.path.getsize(os.path.join(LIVE_DIR, f)) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
