"""bench.py --dump-outputs: what the timed path handed its caller in its last timed step, as .npy files, so that two builds
of the project can be compared output for output on identical inputs (every input of bench.py is seeded)."""
from __future__ import annotations

import os

import numpy as np
import torch

MAX_BYTES = 64 << 20        # the whole dump
LOGIT_ROWS = 65536          # rows of the logits kept (a fixed, seeded sample when the graph has more)
SAMPLE_SEED = 0


def step_outputs(model, logits, loss) -> dict:
    """loss, the logits (all rows, or a fixed sample of them with their row ids), and the model's state after the step:
    parameters, their gradients and floating-point buffers (BatchNorm running statistics) — float32, the loss float64."""
    out = {"loss": np.asarray(float(loss.detach()), dtype=np.float64)}
    for name, p in model.named_parameters():
        out[f"param.{name}"] = p.detach().float().cpu().numpy()
        if p.grad is not None:
            out[f"grad.{name}"] = p.grad.detach().float().cpu().numpy()
    for name, b in model.named_buffers():
        if b.is_floating_point():
            out[f"buffer.{name}"] = b.detach().float().cpu().numpy()
    lg = logits.detach()
    n, c = lg.shape
    budget = MAX_BYTES - sum(a.nbytes for a in out.values())
    k = min(n, LOGIT_ROWS, max(budget // (4 * c + 8), 0))
    if k == n:
        out["logits"] = lg.float().cpu().numpy()
    else:
        rows = torch.randperm(n, generator=torch.Generator().manual_seed(SAMPLE_SEED))[:k].sort().values
        out["logits_sample"] = lg[rows.to(lg.device)].float().cpu().numpy()
        out["logits_sample_rows"] = rows.double().numpy()
    return out


def write_outputs(path: str, arrays: dict) -> None:
    os.makedirs(path, exist_ok=True)
    total = sum(a.nbytes for a in arrays.values())
    if total > MAX_BYTES:
        raise RuntimeError(f"--dump-outputs: {total} bytes, more than the {MAX_BYTES} allowed")
    for name, a in arrays.items():
        if a.dtype not in (np.float32, np.float64):
            raise TypeError(f"--dump-outputs: {name} is {a.dtype}, not float32 / float64")
        np.save(os.path.join(path, f"{name}.npy"), a)
