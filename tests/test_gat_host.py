"""The GAT branch (csrc/gat.hip block N10, sgformer_amd/gat.py) without a GPU: the argument checks of the sgf_gat_* entries
through ctypes (every rejection happens on the host before the first HIP call; pointers are dummy, suitably aligned addresses
that are never dereferenced), the host queries, GATConv / GAT on a CPU kernel table that has the entries
(tests/cpu_kernels_gat.py) AND on the module's plain-PyTorch edge-list path against the dense fp64 restatement of
tests/gat_reference.py, the parameter surface, the Philox keep convention, and the launcher's patch."""
import math
import os
import re
import subprocess
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import gat_reference as R  # noqa: E402
from tests.cpu_kernels import CpuKernels  # noqa: E402
from tests.cpu_kernels_gat import CpuKernelsGat, gat_keep  # noqa: E402

SGF_OK, SGF_E_INVALID, SGF_E_UNSUPPORTED = 0, -1, -4
F32, BF16, F32X = 0, 1, 2
A = 0x10000
F64 = torch.float64

SIGS = {
    "sgf_gat_scores": "xw ldx att_l att_r n heads c dtype al ar stream",
    "sgf_gat_fwd": "rowptr colind xw ldx al ar bias n_rows n_src heads c dtype mean_heads negative_slope p_drop seed out ldo lse "
                   "norm stream",
    "sgf_gat_bwd_dst": "rowptr colind g ldg xw ldx al ar norm n_rows n_src heads c dtype mean_heads negative_slope p_drop seed "
                       "delta dar stream",
    "sgf_gat_bwd_src": "t_rowptr t_colind g ldg xw ldx al ar norm delta dar att_l att_r n_rows n_src heads c dtype mean_heads "
                       "negative_slope p_drop seed dal dxw lddx stream",
}
SCALARS = dict(n=1000, n_rows=1000, n_src=900, heads=8, c=64, dtype=F32, mean_heads=0, negative_slope=0.2, p_drop=0.0, seed=7,
               stream=None)
LD = 8 * 64
# (pointer, leading dimension) of the row operands; the plain arrays that must not be null; the pointers that may be
ROWS = {"sgf_gat_scores": "xw:ldx", "sgf_gat_fwd": "xw:ldx out:ldo", "sgf_gat_bwd_dst": "g:ldg xw:ldx",
        "sgf_gat_bwd_src": "g:ldg xw:ldx dxw:lddx"}
NARROW = {"sgf_gat_fwd": "out:ldo", "sgf_gat_bwd_dst": "g:ldg", "sgf_gat_bwd_src": "g:ldg"}      # c wide under mean_heads
ARRAYS = {"sgf_gat_scores": "att_l att_r al ar", "sgf_gat_fwd": "rowptr colind al ar lse norm",
          "sgf_gat_bwd_dst": "rowptr colind al ar norm delta dar", "sgf_gat_bwd_src": "t_rowptr t_colind al ar norm delta dal"}
OPTIONAL = {"sgf_gat_scores": "", "sgf_gat_fwd": "bias", "sgf_gat_bwd_dst": "", "sgf_gat_bwd_src": "att_l att_r"}
ENTRIES = sorted(SIGS)


@pytest.fixture(scope="module")
def lib():
    from sgformer_amd import _lib
    if not _lib.available():
        pytest.skip("libsgf.so not built (run `make`)")
    return _lib.load()


def _call(lib, entry, **kw):
    names = SIGS[entry].split()
    assert set(kw) <= set(names), (entry, sorted(set(kw) - set(names)))
    args = [kw[a] if a in kw else SCALARS[a] if a in SCALARS else LD if a.startswith("ld") else A for a in names]
    return getattr(lib, entry)(*args)


def _rejected(lib, entry, code, **kw):
    assert _call(lib, entry, **kw) == code, (kw, lib.sgf_last_error())
    assert lib.sgf_last_error().startswith(entry.encode() + b":"), lib.sgf_last_error()


def _rows(entry):
    return [tuple(t.split(":")) for t in ROWS[entry].split()]


def _size(entry):          # the size whose zero makes the launch a no-op
    return {"sgf_gat_scores": "n", "sgf_gat_bwd_src": "n_src"}.get(entry, "n_rows")


# ---- the header, the signatures and the queries ---------------------------------------------------------------------------
def test_every_export_is_declared_and_typed():
    from sgformer_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgf.h")).read(), flags=re.S)
    for name in ENTRIES + ["sgf_gat_supported", "sgf_gat_lap_rows"]:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m is not None, f"{name} not declared in include/sgf.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
    for entry in ENTRIES:                                     # this file's argument names are the header's, in order
        m = re.search(r"\b" + entry + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == SIGS[entry].split(), entry
    assert int(re.search(r"#define\s+SGF_VERSION\s+(\d+)", src).group(1)) >= 670


def test_supported_table(lib):
    for h in range(0, 10):
        for c in (0, 2, 4, 7, 8, 64, 128, 132):
            for dtype in (F32, BF16, F32X, 7):
                want = int(1 <= h <= 8 and c >= 4 and c % 4 == 0 and h * c <= 1024 and dtype in (F32, BF16))
                assert lib.sgf_gat_supported(h, c, dtype) == want, (h, c, dtype)
    assert lib.sgf_gat_supported(1, 1024, F32) == 1 and lib.sgf_gat_supported(1, 1028, F32) == 0
    assert lib.sgf_gat_supported(5, 204, BF16) == 1 and lib.sgf_gat_supported(5, 208, BF16) == 0


def test_lap_rows(lib):
    lap = lib.sgf_gat_lap_rows
    for h, c in ((1, 4), (1, 64), (2, 32), (8, 8), (8, 32), (8, 64), (8, 128), (3, 12), (5, 204), (1, 1024)):
        for dtype in (F32, BF16):
            rows = [lap(h, c, dtype, which) for which in range(4)]
            # a capped grid of 256-thread workgroups, 8 per CU on 256 CUs, a row per group of 8 .. 64 lanes
            assert all(r in (2048 * 4, 2048 * 8, 2048 * 16, 2048 * 32) for r in rows), (h, c, rows)
            assert len(set(rows)) == 1                       # the four kernels share the geometry
    assert lap(8, 64, F32, 0) == 2048 * 4 and lap(1, 64, F32, 1) == 2048 * 16 and lap(1, 4, BF16, 3) == 2048 * 32
    for bad in ((8, 64, F32, 4), (8, 64, F32, -1), (9, 64, F32, 0), (8, 6, F32, 0), (8, 64, F32X, 0)):
        assert lap(*bad) == -1
        assert lib.sgf_last_error().startswith(b"sgf_gat_lap_rows:")


# ---- the launches' checks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_shapes_and_dtype_codes(lib, entry):
    ptr = _rows(entry)[0][0]
    for kw in (dict(heads=0), dict(heads=9), dict(c=0), dict(c=2), dict(c=7), dict(c=132), dict(heads=1, c=1028), dict(dtype=F32X),
               dict(dtype=7)):
        _rejected(lib, entry, SGF_E_UNSUPPORTED, **kw)
        _rejected(lib, entry, SGF_E_UNSUPPORTED, **{ptr: None}, **kw)             # before the pointers
        _rejected(lib, entry, SGF_E_UNSUPPORTED, **{_size(entry): 0}, **kw)       # and for an empty problem too
    sizes = ["n"] if entry == "sgf_gat_scores" else ["n_rows", "n_src"]
    for s in sizes:
        _rejected(lib, entry, SGF_E_INVALID, **{s: -1})
        _rejected(lib, entry, SGF_E_UNSUPPORTED, **{s: 2 ** 31})
        assert b"2^31" in lib.sgf_last_error()
        _rejected(lib, entry, SGF_E_UNSUPPORTED, **{s: 2 ** 31, ptr: None})       # before the pointers


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e != "sgf_gat_scores"])
def test_slope_and_dropout_probability(lib, entry):
    ptr = _rows(entry)[0][0]
    for kw in (dict(negative_slope=float("inf")), dict(negative_slope=float("nan")), dict(p_drop=-0.1), dict(p_drop=1.5),
               dict(p_drop=float("nan"))):
        _rejected(lib, entry, SGF_E_INVALID, **kw)
        _rejected(lib, entry, SGF_E_INVALID, **{ptr: None}, **kw)                 # before the pointers
        _rejected(lib, entry, SGF_E_INVALID, **{_size(entry): 0}, **kw)           # and for an empty problem too
    for kw in (dict(p_drop=0.0), dict(p_drop=1.0), dict(negative_slope=0.0), dict(negative_slope=-1.0)):
        assert _call(lib, entry, **{_size(entry): 0}, **kw) == SGF_OK, lib.sgf_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_problems(lib, entry):
    names = SIGS[entry].split()
    nothing = {a: (0 if a.startswith("ld") else None) for a in names if a not in SCALARS}
    for dtype in (F32, BF16):
        assert _call(lib, entry, dtype=dtype, **{_size(entry): 0}, **nothing) == SGF_OK, lib.sgf_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_pointers(lib, entry):
    for dtype in (F32, BF16):
        for ptr, ld in _rows(entry):
            _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **{ptr: None})
            assert b"null pointer" in lib.sgf_last_error() and ptr.encode() in lib.sgf_last_error(), lib.sgf_last_error()
            _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **{ptr: None, ld: 8})                # before the widths
            assert b"null pointer" in lib.sgf_last_error(), lib.sgf_last_error()
        for ptr in ARRAYS[entry].split():
            _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **{ptr: None})
            assert b"null pointer" in lib.sgf_last_error() and ptr.encode() in lib.sgf_last_error(), lib.sgf_last_error()
    if entry == "sgf_gat_bwd_src":
        _rejected(lib, entry, SGF_E_INVALID, dar=None)                  # dar goes with att_r
        assert b"dar" in lib.sgf_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_leading_dimensions_and_alignment(lib, entry):
    for dtype, nbytes in ((BF16, 8), (F32, 16)):
        for ptr, ld in _rows(entry):
            _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **{ld: LD - 4})
            assert b"leading dimension smaller than the width" in lib.sgf_last_error(), lib.sgf_last_error()
            _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **{ld: LD - 4, ptr: A + 2})          # before the alignment
            assert b"leading dimension smaller than the width" in lib.sgf_last_error(), lib.sgf_last_error()
            for kw in ({ptr: A + nbytes // 2}, {ptr: A + 2}, {ld: LD + 2}, {ld: LD + 1}):
                _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **kw)
                assert b"-byte aligned" in lib.sgf_last_error(), (kw, lib.sgf_last_error())
        for ptr in OPTIONAL[entry].split() + (["att_l", "att_r"] if entry == "sgf_gat_scores" else []):
            _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **{ptr: A + 8})
            assert b"16-byte aligned" in lib.sgf_last_error(), lib.sgf_last_error()
    # mean over the heads: out / g are c wide, not heads * c
    for tok in NARROW.get(entry, "").split():
        ptr, ld = tok.split(":")
        _rejected(lib, entry, SGF_E_INVALID, mean_heads=1, **{ld: 60})
        assert b"leading dimension smaller than the width" in lib.sgf_last_error()
        _rejected(lib, entry, SGF_E_INVALID, mean_heads=1, **{ld: 64, "xw": None})       # the narrow row passes: the next speaks
        assert b"null pointer" in lib.sgf_last_error()
        _rejected(lib, entry, SGF_E_INVALID, mean_heads=0, **{ld: 64})


# ---- the modules on a CPU kernel table and on the edge-list path, against the dense restatement ------------------------------
@pytest.fixture
def table():
    from sgformer_amd import ops
    CpuKernelsGat.calls = {}
    prev = ops.set_kernels(CpuKernelsGat())
    yield CpuKernelsGat
    ops.set_kernels(prev)


def _graph(n=23, seed=0):
    """sources -> targets with parallel edges (3 <- 5 twice, 0 <- 1 three times), existing self-loops (2, 7; 7 twice) and a
    node (n - 1) that is nobody's target"""
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (4 * n,), generator=gen)
    dst = torch.randint(0, n - 1, (4 * n,), generator=gen)
    extra = torch.tensor([[5, 5, 1, 1, 1, 2, 7, 7], [3, 3, 0, 0, 0, 2, 7, 7]])
    ei = torch.cat([torch.stack([src, dst]), extra], 1)
    return ei[:, ei[1] != n - 1]


def _reference_conv(conv, x, ei, g):
    """logits and parameter gradients of one GATConv by tests/gat_reference.py in fp64"""
    n, h, c = x.shape[0], conv.heads, conv.out_channels
    w = conv.lin_l.weight.detach().to(F64).requires_grad_(True)
    al = conv.att_l.detach().to(F64).requires_grad_(True)
    ar = conv.att_r.detach().to(F64).requires_grad_(True)
    b = conv.bias.detach().to(F64).requires_grad_(True)
    xx = x.detach().to(F64).requires_grad_(True)
    out, _ = R.dense((xx @ w.t()).view(n, h, c), al[0], ar[0], R.multiplicity(ei, n, conv.add_self_loops),
                     conv.negative_slope, concat=conv.concat, bias=b)
    out.backward(g.to(F64))
    return out.detach(), dict(x=xx.grad, w=w.grad, att_l=al.grad, att_r=ar.grad, bias=b.grad)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


CONV_CASES = [dict(heads=2, c=8, concat=True, loops=True), dict(heads=2, c=8, concat=False, loops=True),
              dict(heads=3, c=4, concat=True, loops=False), dict(heads=1, c=12, concat=False, loops=False),
              dict(heads=2, c=7, concat=True, loops=True), dict(heads=1, c=7, concat=False, loops=False)]


def _run_conv(case, path, monkeypatch):
    from sgformer_amd import gat
    torch.manual_seed(11)
    n, d_in = 23, 10
    ei = _graph(n)
    conv = gat.GATConv(d_in, case["c"], heads=case["heads"], concat=case["concat"], negative_slope=0.3,
                       add_self_loops=case["loops"])
    with torch.no_grad():
        conv.bias.uniform_(-1, 1)
        conv.att_l.mul_(4), conv.att_r.mul_(4)
    dtype = F64 if path == "edge_list64" else torch.float32
    conv = conv.to(dtype)
    x = torch.randn(n, d_in, dtype=dtype, requires_grad=True)
    g = torch.randn(n, case["heads"] * case["c"] if case["concat"] else case["c"], dtype=dtype)
    if path != "table":
        monkeypatch.setenv("SGF_GAT", "0")
    out = conv(x, ei)
    out.backward(g)
    ref, grads = _reference_conv(conv, x, ei, g)
    tol = 1e-12 if dtype == F64 else 2e-5
    assert out.shape == ref.shape and _rel(out.detach(), ref) <= tol
    if not case["loops"]:                                  # the node that is nobody's target: bias alone, exactly
        assert torch.equal(out[n - 1].detach(), conv.bias.detach().view(-1, case["c"]).mean(0) if not case["concat"]
                           else conv.bias.detach())
    got = dict(x=x.grad, w=conv.lin_l.weight.grad, att_l=conv.att_l.grad, att_r=conv.att_r.grad, bias=conv.bias.grad)
    for k, v in grads.items():
        assert got[k].shape == v.shape and _rel(got[k], v) <= tol, k


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "h{heads}c{c}{}{}".format("cat" if c["concat"] else "mean",
                                                                                      "+loops" if c["loops"] else "", **c))
def test_conv_on_the_cpu_table(table, case, monkeypatch):
    monkeypatch.setenv("SGF_GAT", "1")
    _run_conv(case, "table", monkeypatch)
    assert sorted(table.calls) == ["gat_bwd_dst", "gat_bwd_src", "gat_fwd", "gat_scores"], table.calls
    assert table.calls["gat_fwd"] == [23] and table.calls["gat_bwd_src"] == [23]


@pytest.mark.parametrize("path", ["edge_list", "edge_list64"])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "h{heads}c{c}{}{}".format("cat" if c["concat"] else "mean",
                                                                                      "+loops" if c["loops"] else "", **c))
def test_conv_on_the_edge_list_path(table, case, path, monkeypatch):
    _run_conv(case, path, monkeypatch)
    assert table.calls == {}                               # SGF_GAT=0: no entry ran


def test_closed_backward_formulas_agree_with_autograd():
    """tests/gat_reference.backward (what the GPU tests compare delta, dar, dal with) against fp64 autograd of dense()"""
    torch.manual_seed(2)
    n, h, c = 17, 3, 4
    ei = _graph(n)
    mult = R.multiplicity(ei, n, True)
    keep = torch.rand(n, n, h) >= 0.4
    for concat in (True, False):
        xw = torch.randn(n, h, c, dtype=F64, requires_grad=True)
        att_l, att_r = (torch.randn(h, c, dtype=F64, requires_grad=True) for _ in range(2))
        bias = torch.zeros(h * c if concat else c, dtype=F64, requires_grad=True)
        g = torch.randn(n, h * c if concat else c, dtype=F64)
        out, _ = R.dense(xw, att_l, att_r, mult, 0.2, keep, 0.4, concat, bias)
        out.backward(g)
        b = R.backward(xw.detach(), att_l.detach(), att_r.detach(), mult, g, 0.2, keep, 0.4, concat)
        assert _rel(b["dxw"], xw.grad) <= 1e-12 and _rel(b["datt_l"], att_l.grad) <= 1e-12
        assert _rel(b["datt_r"], att_r.grad) <= 1e-12 and _rel(b["dbias"], bias.grad) <= 1e-12


@pytest.mark.parametrize("layers,use_bn", [(2, False), (3, True)])
def test_gat_model_on_both_paths(table, layers, use_bn, monkeypatch):
    from sgformer_amd import gat
    torch.manual_seed(5)
    n = 23
    ei = _graph(n)
    model = gat.GAT(10, 8, 7, num_layers=layers, dropout=0.0, use_bn=use_bn, heads=2, out_heads=1)
    data = types.SimpleNamespace(graph={"node_feat": torch.randn(n, 10), "edge_index": ei})
    outs, grads = [], []
    for switch in ("1", "0"):
        monkeypatch.setenv("SGF_GAT", switch)
        model.zero_grad()
        out = model(data)
        out.square().sum().backward()
        outs.append(out.detach().clone())
        grads.append([p.grad.clone() for p in model.parameters() if p.grad is not None])     # (use_bn=False: the BatchNorms are unused)
    assert outs[0].shape == (n, 7) and table.calls["gat_fwd"] == [n] * layers
    assert _rel(outs[0], outs[1]) <= 2e-5
    gmax = max(float(b.abs().max()) for b in grads[1])
    for a, b in zip(*grads):             # (a conv bias ahead of a BatchNorm has a gradient of rounding noise alone)
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()) + 1e-6 * gmax


# ---- the parameter surface -------------------------------------------------------------------------------------------------
def test_state_dict_and_initialisation():
    from sgformer_amd import gat
    torch.manual_seed(0)
    conv = gat.GATConv(40, 16, heads=8)
    assert conv.lin_r is conv.lin_l
    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == {
        "lin_l.weight": (128, 40), "lin_r.weight": (128, 40), "att_l": (1, 8, 16), "att_r": (1, 8, 16), "bias": (128,)}
    assert len(list(conv.parameters())) == 4                 # the shared weight counts once
    assert tuple(gat.GATConv(40, 16, heads=8, concat=False).bias.shape) == (16,)
    assert gat.GATConv(40, 16, bias=False).bias is None
    a_w, a_att = math.sqrt(6.0 / (40 + 128)), math.sqrt(6.0 / (8 + 16))
    for t, a in ((conv.lin_l.weight.detach(), a_w), (conv.att_l.detach(), a_att), (conv.att_r.detach(), a_att)):
        assert float(t.abs().max()) <= a and float(t.abs().max()) >= 0.9 * a and abs(float(t.mean())) < 0.1 * a
    assert float(conv.bias.abs().max()) == 0.0
    other = gat.GATConv(40, 16, heads=8)
    other.load_state_dict(conv.state_dict())
    assert torch.equal(other.lin_r.weight, conv.lin_l.weight)
    model = gat.GAT(40, 16, 7, num_layers=3, heads=8, out_heads=1, use_bn=True)
    keys = set(model.state_dict())
    assert {"convs.0.lin_l.weight", "convs.0.lin_r.weight", "convs.0.att_l", "convs.0.att_r", "convs.0.bias",
            "convs.2.att_r", "bns.1.running_mean"} <= keys
    assert model.convs[1].in_channels == 128 and model.convs[2].concat is False and model.convs[2].heads == 1


def test_supported_and_the_switch(table, monkeypatch):
    from sgformer_amd import gat, ops
    monkeypatch.delenv("SGF_GAT", raising=False)
    xw = torch.randn(10, 64)
    assert gat.supported(xw, 8, 8) and gat.supported(xw.bfloat16(), 1, 64) and gat.supported(xw, 2, 32)
    assert not gat.supported(xw.double(), 8, 8) and not gat.supported(xw, 8, 4) and not gat.supported(xw[:, :14], 2, 7)
    assert not gat.supported(xw[:0], 8, 8) and not gat.supported(torch.randn(4, 9 * 4), 9, 4)
    assert gat.use_kernels(xw, 8, 8) == gat.GAT_DEFAULT_ON
    monkeypatch.setenv("SGF_GAT", "1")
    assert gat.use_kernels(xw, 8, 8)
    monkeypatch.setenv("SGF_GAT", "0")
    assert not gat.use_kernels(xw, 8, 8)
    monkeypatch.setenv("SGF_GAT", "1")
    prev = ops.set_kernels(CpuKernels())                     # the stock CPU table has no gat_*: the edge-list path
    try:
        assert not gat.supported(xw, 8, 8) and not gat.use_kernels(xw, 8, 8)
        with pytest.raises(RuntimeError, match="unsupported operands"):
            gat.gat_aggregate(types.SimpleNamespace(n=10), xw, torch.zeros(1, 8, 8), torch.zeros(1, 8, 8))
    finally:
        ops.set_kernels(prev)
    conv = gat.GATConv(4, 8)
    conv._shard = object()
    with pytest.raises(NotImplementedError, match="node-sharded"):
        conv(torch.randn(5, 4), torch.zeros(2, 0, dtype=torch.int64))


# ---- dropout ---------------------------------------------------------------------------------------------------------------
def test_keep_mask_is_a_function_of_target_source_and_head(table):
    """the same decisions from the forward CSR and from its transpose, and for parallel entries"""
    from sgformer_amd import ops
    n, h = 23, 8
    ei = _graph(n)
    g = ops.CSRGraph(ei, n)
    tgt = torch.repeat_interleave(torch.arange(n), g.rowptr[1:] - g.rowptr[:-1])
    fwd = gat_keep(1234567891011, tgt, g.colind.long(), h, 0.5)
    t_rowptr, t_colind = g.transposed()[:2]
    src_t = torch.repeat_interleave(torch.arange(n), t_rowptr[1:] - t_rowptr[:-1])
    bwd = gat_keep(1234567891011, t_colind.long(), src_t, h, 0.5)
    dense_f = torch.zeros(n, n, h, dtype=torch.int64)
    dense_b = torch.zeros(n, n, h, dtype=torch.int64)
    dense_f[tgt, g.colind.long()] = fwd.long() + 1
    dense_b[t_colind.long(), src_t] = bwd.long() + 1
    assert torch.equal(dense_f, dense_b) and int((dense_f > 0).sum()) > 0
    pair = (tgt == 0) & (g.colind.long() == 1)               # 0 <- 1 is stored three times: one draw
    assert int(pair.sum()) == 3 and bool((fwd[pair] == fwd[pair][0]).all())
    assert not torch.equal(gat_keep(5, tgt, g.colind.long(), h, 0.5), fwd)                        # another seed
    assert not torch.equal(fwd[:, 0], fwd[:, 4])                                                  # another head group
    assert not torch.equal(fwd[:, 0], fwd[:, 1])                                                  # another word


def test_philox_known_answers():
    """tests/philox_host.py against the three known-answer vectors of the Philox4x32-10 paper, and against the integer Philox the
    sgf_dropout tests use (tests/test_gpu_ew_laps.py): one generator on both sides of the library's two dropouts"""
    from tests import test_gpu_ew_laps as G
    from tests.philox_host import philox4x32_10
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        got = philox4x32_10(tuple(torch.tensor([v], dtype=torch.int64) for v in ctr), key)
        assert tuple(int(w) for w in got) == want, (ctr, [hex(int(w)) for w in got])
    gen = torch.Generator().manual_seed(1)
    ctr = tuple(torch.randint(0, 2 ** 32, (1000,), generator=gen, dtype=torch.int64) for _ in range(4))
    for a, b in zip(philox4x32_10(ctr, (0x12345678, 0x9ABCDEF0)), G.philox4x32_10(ctr, (0x12345678, 0x9ABCDEF0))):
        assert torch.equal(a, b)


@pytest.mark.parametrize("p", [0.25, 0.5, 0.9])
def test_kept_share(p):
    i = torch.arange(12500)
    keep = gat_keep(987654321, i % 500, i // 500 + 3 * (i % 7), 8, p)         # 10^5 draws
    sigma = math.sqrt(p * (1 - p) / keep.numel())
    assert abs(float(keep.float().mean()) - (1 - p)) <= 4 * sigma


def test_dropout_follows_the_philox_mask_and_eval_ignores_it(table, monkeypatch):
    from sgformer_amd import gat, ops
    monkeypatch.setenv("SGF_GAT", "1")
    n, h, c, p = 23, 2, 8, 0.5
    ei = _graph(n)
    conv = gat.GATConv(10, c, heads=h, dropout=p)
    x = torch.randn(n, 10)
    conv.eval()
    quiet = conv(x, ei)
    conv.dropout = 0.0
    assert torch.equal(conv(x, ei), quiet)                   # eval mode ignores p
    conv.dropout = p
    conv.train()
    torch.manual_seed(77)
    seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64))          # the draw gat_aggregate makes
    torch.manual_seed(77)
    out = conv(x, ei)
    mult = R.multiplicity(ei, n, True)
    ii, jj = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
    keep = gat_keep(seed, ii.reshape(-1), jj.reshape(-1), h, p).view(n, n, h)
    ref, _ = R.dense((x.double() @ conv.lin_l.weight.double().t()).view(n, h, c), conv.att_l[0], conv.att_r[0], mult, 0.2, keep, p,
                     True, conv.bias)
    assert _rel(out.detach(), ref.detach()) <= 2e-5
    assert _rel(out.detach(), quiet.detach()) > 1e-2         # and it did drop


# ---- the model around it, and the launcher ------------------------------------------------------------------------------------
def test_sgformer_with_a_gat_branch_trains(table, monkeypatch):
    from sgformer_amd import gat, ours_medium
    monkeypatch.setenv("SGF_GAT", "1")
    torch.manual_seed(3)
    n, d_in, hidden, classes = 40, 12, 16, 4
    ei = _graph(n, seed=4)
    x = torch.randn(n, d_in)
    y = torch.randint(0, classes, (n,))
    gnn = gat.GAT(d_in, hidden // 2, hidden, num_layers=2, dropout=0.0, heads=2, out_heads=1)
    model = ours_medium.SGFormer(d_in, hidden, classes, num_layers=1, dropout=0.0, use_bn=True, use_graph=True, gnn=gnn)
    data = types.SimpleNamespace(graph={"node_feat": x, "edge_index": ei})
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(data), y)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(math.isfinite(v) for v in losses) and losses[2] < losses[1] < losses[0], losses
    assert len(table.calls["gat_fwd"]) == 6 and len(table.calls["gat_bwd_src"]) == 6
    assert {id(p) for p in gnn.parameters()} <= {id(p) for p in model.params2}


def test_patch_medium_gat(monkeypatch):
    from sgformer_amd import gat, launch
    fake = types.ModuleType("models")
    fake.GAT, fake.GCN = object, object
    monkeypatch.setitem(sys.modules, "models", fake)
    assert launch.patch_medium_gat() is fake
    assert fake.GAT is gat.GAT and fake.GCN is object


CORA_GAT = ("--backbone gat --gat_heads 2 --dataset cora --lr 0.01 --num_layers 2 --hidden_channels 32 --weight_decay 5e-4 "
            "--dropout 0. --method ours --ours_layers 1 --use_graph --graph_weight 0.8 --ours_dropout 0. --use_residual --alpha 0.5 "
            "--ours_weight_decay 0.001 --rand_split_class --valid_num 100 --test_num 150 --no_feat_norm --seed 123 --runs 1 "
            "--epochs 4 --display_step 1 --cpu").split()


@pytest.mark.skipif(not ref_shim.reference_available(), reason="the reference is not mounted")
def test_medium_trainer_with_the_gat_backbone(tmp_path):
    """medium/main.py --backbone gat (the CORA line of tests/test_trainer_unchanged.py with another backbone), unchanged, under
    sgformer_amd.launch: models.GAT is sgformer_amd.gat.GAT (on the stock CPU table: its edge-list path) and the run prints its
    epochs with finite losses.  There is no side-by-side: the reference's own GAT needs torch_geometric's GATConv, which does not
    exist here (tests/standins/torch_geometric/nn holds a placeholder)."""
    env = {**os.environ, "PYTHONHASHSEED": "0"}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "run_trainer.py"), "ours",
                        os.path.join(ref_shim.REFERENCE_ROOT, "medium", "main.py")] + CORA_GAT + ["--data_dir", str(tmp_path) + "/"],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    rows = re.findall(r"Epoch: (\d+), Loss: ([\d.]+), Train: ([\d.]+)%, Valid: ([\d.]+)%, Test: ([\d.]+)%", p.stdout)
    assert len(rows) >= 4 and all(math.isfinite(float(r[1])) for r in rows), p.stdout[-2000:]
    assert "SGF_OURS_MODULE sgformer_amd.ours_medium" in p.stdout
