#!/usr/bin/env python
"""Bit-identity of the pair-attention entries (csrc/pair_attn.hip, blocks N7 and N8) between two builds: for each arm, fwd, bwd_q
with and without dq, and bwd_kv through pair_attn._Hip on seeded operands, and a SHA-256 of every output tensor (out, rowsum / lse,
delta, delta of the dq-less launch, dq, dk, dv).  The grid: fp32 and bf16 storage, D in {32, 64, 128}, (H, Hv) in {(1, 1), (3, 1),
(3, 3)}, (n, l) in {(1, 1), (31, 33), (33, 31), (70, 193), (257, 255)}, for the softmax arm scale 1 and 0.125, and per arm and dtype
one case whose operands sit in buffers wider than their rows.  Every gradient of these kernels is a fixed-order sum, so two builds
that compute the same thing agree in every bit.  One process, a few seconds:
    timeout -k 10 120 python scripts/pair_digest.py --out A.json [--root OTHER_CHECKOUT]      (once per build)
    python scripts/pair_digest.py --compare A.json B.json                                    (no GPU; exit status 1 on a difference)"""
import argparse
import hashlib
import json
import os
import sys

import torch

SHAPES = ((1, 1), (31, 33), (33, 31), (70, 193), (257, 255))
HEADS = ((1, 1), (3, 1), (3, 3))
WIDTHS = (32, 64, 128)
WIDE = dict(d=64, heads=(3, 1), shape=(70, 193), pad=8)      # pad: elements past the row, 16 bytes or more in both dtypes


def sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy().tobytes()).hexdigest()


def widen(t, pad):
    """the same [rows, H, D] values in a buffer whose rows are `pad` elements longer"""
    rows, h, d = t.shape
    buf = torch.zeros(rows, h * d + pad, dtype=t.dtype, device=t.device)
    buf[:, :h * d] = t.reshape(rows, h * d)
    return buf[:, :h * d].unflatten(1, (h, d))


def case(hip, arm, dtype, d, h, hv, n, l, scale, pad, dev):
    gen = torch.Generator().manual_seed(1000 * n + 10 * l + d + h + hv)
    q, g = ((2.0 / d ** 0.5) * torch.randn(n, h, d, generator=gen), torch.randn(n, h, d, generator=gen))
    k, v = ((2.0 / d ** 0.5) * torch.randn(l, h, d, generator=gen), torch.randn(l, hv, d, generator=gen))
    q, k, v, g = (t.to(dev, dtype) for t in (q, k, v, g))
    if pad:
        q, k, v, g = (widen(t, pad) for t in (q, k, v, g))
    extra = () if arm == "sigmoid" else (scale,)
    fwd, bwd_q, bwd_kv = (getattr(hip, f"pair_{arm}_{e}") for e in ("fwd", "bwd_q", "bwd_kv"))
    out, saved = fwd(q, k, v, *extra)
    o = widen(out, pad) if pad else out
    dq, delta = bwd_q(g, o, saved, q, k, v, *extra)
    none, delta_only = bwd_q(g, o, saved, q, k, v, *extra, want_dq=False)
    assert none is None
    dk, dv = bwd_kv(g, saved, delta, q, k, v, *extra)
    return dict(out=sha(out), saved=sha(saved), delta=sha(delta), delta_only=sha(delta_only), dq=sha(dq), dk=sha(dk), dv=sha(dv))


def compare(a, b):
    ca, cb = (json.load(open(p))["cases"] for p in (a, b))
    bad = sorted(set(ca) ^ set(cb)) + [f"{key}: {name}" for key in sorted(set(ca) & set(cb)) for name in ca[key]
                                       if ca[key][name] != cb[key].get(name)]
    kinds = {}
    for key in ca:
        for name in ca[key]:
            kinds[name] = kinds.get(name, 0) + 1
    print(json.dumps(dict(probe="pair_digest_compare", cases=len(ca), digests=kinds, different=bad)))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="keep the JSON line in this file")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose sgformer_amd (and library) is loaded; default: this one")
    ap.add_argument("--compare", nargs=2, default=None, metavar="JSON", help="compare two --out files, measure nothing")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    sys.path.insert(0, os.path.abspath(args.root))
    from sgformer_amd import _lib, pair_attn
    dev = torch.device("cuda:0")
    cases = {}
    for arm in ("sigmoid", "softmax"):
        for dtype in (torch.float32, torch.bfloat16):
            grid = [(d, h, hv, n, l, 0) for d in WIDTHS for h, hv in HEADS for n, l in SHAPES]
            grid.append((WIDE["d"], *WIDE["heads"], *WIDE["shape"], WIDE["pad"]))
            for d, h, hv, n, l, pad in grid:
                for scale in ((1.0,) if arm == "sigmoid" else (1.0, 0.125)):
                    key = f"{arm}/{str(dtype)[6:]}/D{d}/H{h}.{hv}/n{n}.l{l}/scale{scale}" + ("/wide" if pad else "")
                    cases[key] = case(pair_attn._Hip, arm, dtype, d, h, hv, n, l, scale, pad, dev)
    torch.cuda.synchronize()
    line = json.dumps(dict(probe="pair_digest", library=_lib.LIB_PATH, cases=cases))
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(json.dumps(dict(probe="pair_digest", library=_lib.LIB_PATH, cases=len(cases),
                          all=hashlib.sha256(json.dumps(cases, sort_keys=True).encode()).hexdigest())))


if __name__ == "__main__":
    main()
