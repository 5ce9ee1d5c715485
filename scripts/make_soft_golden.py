"""Write tests/golden/soft/soft_cfg{0,1}.npz: a seeded state_dict, inputs, and the logits and parameter gradients of the LIVE
reference's SGFormerSOFT (medium/ablation/oursSOFT.py) for them.  Run where the reference is mounted (SGF_REFERENCE_ROOT,
oracle/ref_shim.py):

    python scripts/make_soft_golden.py

oursSOFT.py and medium/models.py are imported unchanged over the stand-ins the other fixtures use (oracle.ref_shim).  The
model runs in fp64, in train mode with dropout 0, under the mean cross-entropy of seeded labels.  A subdirectory: the model
tests take every tests/golden/*.npz for a model fixture.  Tests read only the fixtures.

Each file holds two recordings of the same model on the same inputs:
  * `logits`, `grad/<parameter>`: the reference exactly as shipped.  Its softmax_attention calls F.softmax(scores, dim=-1) on
    scores of shape [N, L, H]: the weights are normalised over the HEADS.
  * `logits_keys`, `grad_keys/<parameter>`: the same unchanged code run while torch.nn.functional.softmax is wrapped so that
    this one call (a 3-D input with dim=-1) is taken over dim=1, the KEYS — the softmax attention of the paper's ablation and
    of include/sgf.h block N8.
`state/<key>` is the state_dict before the step (fp32 values), `x`, `edge_index`, `y` the inputs, `meta` a JSON string."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden", "soft")
N, F_IN, HIDDEN, CLASSES = 203, 24, 64, 5
CONFIGS = [
    dict(num_layers=2, num_heads=1, use_weight=True, use_graph=False, gcn_layers=0),
    dict(num_layers=1, num_heads=2, use_weight=False, use_graph=True, gcn_layers=2),
]


def _exec(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_soft():
    """(oursSOFT, models) of the reference, executed unchanged; oursSOFT.py:9 does `from models import GCN`."""
    ref_shim.install_stand_ins()
    saved = sys.modules.get("models")
    models = _exec(os.path.join(ref_shim.REFERENCE_ROOT, "medium", "models.py"), "_sgf_reference_medium_models")
    sys.modules["models"] = models
    try:
        return _exec(os.path.join(ref_shim.REFERENCE_ROOT, "medium", "ablation", "oursSOFT.py"), "_sgf_reference_soft"), models
    finally:
        if saved is None:
            del sys.modules["models"]
        else:
            sys.modules["models"] = saved


class _Data:
    def __init__(self, x, ei):
        self.graph = {"node_feat": x, "edge_index": ei}


class _softmax_over_keys:
    """While active, F.softmax(3-D tensor, dim=-1) — the one call of oursSOFT.softmax_attention — runs over dim=1."""

    def __enter__(self):
        self.orig = torch.nn.functional.softmax

        def softmax(input, dim=None, *args, **kwargs):
            if input.dim() == 3 and dim == -1:
                dim = 1
            return self.orig(input, dim, *args, **kwargs)
        torch.nn.functional.softmax = softmax

    def __exit__(self, *exc):
        torch.nn.functional.softmax = self.orig


def _graph(n, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (4 * n,), generator=g)
    dst = torch.randint(0, n, (4 * n,), generator=g)
    keep = src != dst
    return torch.stack([torch.cat([src[keep], dst[keep]]), torch.cat([dst[keep], src[keep]])])


def _step(soft, models, cfg, state, x, ei, y):
    gnn = models.GCN(F_IN, HIDDEN, HIDDEN, num_layers=cfg["gcn_layers"], dropout=0.0) if cfg["use_graph"] else None
    m = soft.SGFormerSOFT(F_IN, HIDDEN, CLASSES, num_layers=cfg["num_layers"], num_heads=cfg["num_heads"], dropout=0.0,
                          use_weight=cfg["use_weight"], use_graph=cfg["use_graph"], gnn=gnn).double()
    if state is None:
        return {k: v.detach().clone() for k, v in m.float().state_dict().items()}
    m.load_state_dict(state)
    m.train()
    logits = m(_Data(x.double(), ei))
    torch.nn.functional.cross_entropy(logits, y).backward()
    return logits.detach(), {k: p.grad.detach() for k, p in m.named_parameters() if p.grad is not None}


def main():
    soft, models = reference_soft()
    os.makedirs(OUT_DIR, exist_ok=True)
    for i, cfg in enumerate(CONFIGS):
        torch.manual_seed(1000 + i)
        state = _step(soft, models, cfg, None, None, None, None)
        g = torch.Generator().manual_seed(2000 + i)
        x = torch.randn(N, F_IN, generator=g)
        y = torch.randint(0, CLASSES, (N,), generator=g)
        ei = _graph(N, 3000 + i)
        logits, grads = _step(soft, models, cfg, state, x, ei, y)
        with _softmax_over_keys():
            logits_k, grads_k = _step(soft, models, cfg, state, x, ei, y)
        assert set(grads) == set(grads_k)
        blob = {"x": x.numpy(), "edge_index": ei.numpy(), "y": y.numpy(), "logits": logits.numpy(),
                "logits_keys": logits_k.numpy()}
        for k, v in state.items():
            blob["state/" + k] = v.numpy()
        for k in grads:
            blob["grad/" + k] = grads[k].float().numpy()
            blob["grad_keys/" + k] = grads_k[k].float().numpy()
        blob["meta"] = np.array(json.dumps(dict(
            cfg, n=N, in_channels=F_IN, hidden_channels=HIDDEN, out_channels=CLASSES, dropout=0.0, loss="cross_entropy(mean)",
            source="medium/ablation/oursSOFT.py, fp64, train mode", grad_dtype="float32 (rounded from fp64)")))
        path = os.path.join(OUT_DIR, f"soft_cfg{i}.npz")
        np.savez_compressed(path, **blob)
        print(f"cfg{i}: {len(state)} state entries, {len(grads)} gradients, |logits - logits_keys| max "
              f"{float((logits - logits_k).abs().max()):.3e}; wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
