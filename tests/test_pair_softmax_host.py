"""All-pair softmax attention (csrc/pair_attn.hip block N8, sgformer_amd/pair_attn.py) without a GPU: the argument checks of
the sgf_pair_softmax_* entries through ctypes (every rejection happens on the host before the first HIP call; pointers are
dummy, suitably aligned addresses that are never dereferenced), the autograd wiring of pair_attn.softmax_attention on a CPU
kernel table that has the entries (tests/cpu_kernels_pair_softmax.py) against torch.autograd of the dense formula, and the
supported / switch logic."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.cpu_kernels import CpuKernels  # noqa: E402
from tests.cpu_kernels_pair_softmax import CpuKernelsPairSoftmax  # noqa: E402

SGF_OK, SGF_E_INVALID, SGF_E_WORKSPACE, SGF_E_UNSUPPORTED = 0, -1, -2, -4
F32, BF16, F32X = 0, 1, 2
A = 0x10000
BIG = 1 << 40

SIGS = {
    "sgf_pair_softmax_fwd": "q ldq k ldk v ldv n l heads v_heads d dtype scale out ldo lse stream",
    "sgf_pair_softmax_bwd_q": "g ldg out ldo lse q ldq k ldk v ldv n l heads v_heads d dtype scale dq lddq workspace "
                              "workspace_bytes stream",
    "sgf_pair_softmax_bwd_kv": "g ldg lse q ldq k ldk v ldv n l heads v_heads d dtype scale dk lddk dv lddv workspace "
                               "workspace_bytes stream",
}
SCALARS = dict(n=1000, l=900, heads=2, v_heads=2, d=64, dtype=BF16, scale=0.125, workspace_bytes=BIG, stream=None)
LD = 2 * 64              # heads * d of the default call
# (pointer, its leading dimension) of the row operands; dq of bwd_q may be null (delta only)
ROWS = {
    "sgf_pair_softmax_fwd": "q:ldq k:ldk v:ldv out:ldo",
    "sgf_pair_softmax_bwd_q": "g:ldg out:ldo q:ldq k:ldk v:ldv dq:lddq",
    "sgf_pair_softmax_bwd_kv": "g:ldg q:ldq k:ldk v:ldv dk:lddk dv:lddv",
}
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


# ---- the header, the signatures and the queries ---------------------------------------------------------------------------
def test_every_export_is_declared_and_typed():
    import re
    from sgformer_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgf.h")).read(), flags=re.S)
    names = ENTRIES + ["sgf_pair_softmax_supported", "sgf_pair_softmax_workspace_bytes", "sgf_pair_softmax_lap_rows"]
    for name in names:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m is not None, f"{name} not declared in include/sgf.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
    for entry in ENTRIES:                                     # this file's argument names are the header's, in order
        m = re.search(r"\b" + entry + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == SIGS[entry].split(), entry


def test_supported_table(lib):
    for d in (16, 32, 48, 64, 128, 256):
        for h in (0, 1, 8, 9):
            for hv in (0, 1, 2, h):
                for dtype in (F32, BF16, F32X):
                    want = int(d in (32, 64, 128) and 1 <= h <= 8 and hv in (1, h) and dtype in (F32, BF16))
                    assert lib.sgf_pair_softmax_supported(h, hv, d, dtype) == want, (h, hv, d, dtype)


def test_workspace_is_linear_in_the_rows(lib):
    ws = lib.sgf_pair_softmax_workspace_bytes
    for h in (1, 3, 8):
        for n, l in ((1, 1), (1000, 10), (10, 1000), (40009, 40009)):
            assert ws(n, l, h) <= 4 * h * (n + l)                        # O((n + l) H): nothing of size n x l
            assert ws(2 * n, 2 * l, h) == 2 * ws(n, l, h)
        assert ws(1000, 900, h) == 4 * 1000 * h                          # delta fp32 [n, H]
    assert ws(0, 0, 2) == 0


def test_lap_rows_is_monotone_in_laps(lib):
    lap = lib.sgf_pair_softmax_lap_rows
    for which in (0, 1, 2):
        for d in (32, 64, 128):
            for dtype in (F32, BF16):
                rows = [lap(which, 2, d, dtype, laps) for laps in (1, 2, 3, 5)]
                assert all(r >= 0 for r in rows) and rows == sorted(rows), (which, d, dtype, rows)
    assert lap(3, 2, 64, BF16, 1) == -1 and lap(0, 2, 48, BF16, 1) == -1 and lap(0, 2, 64, F32X, 1) == -1
    assert lap(0, 2, 64, BF16, 0) == -1
    assert lib.sgf_last_error().startswith(b"sgf_pair_softmax_lap_rows:")


# ---- the launches' checks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_shapes_and_dtype_codes(lib, entry):
    for kw in (dict(d=16), dict(d=48), dict(d=256), dict(heads=0, v_heads=0), dict(heads=9, v_heads=9), dict(dtype=F32X),
               dict(dtype=7)):
        _rejected(lib, entry, SGF_E_UNSUPPORTED, **kw)
        _rejected(lib, entry, SGF_E_UNSUPPORTED, q=None, **kw)             # before the pointers
        _rejected(lib, entry, SGF_E_UNSUPPORTED, n=0, **kw)                # and for an empty problem too
        _rejected(lib, entry, SGF_E_UNSUPPORTED, scale=0.0, **kw)          # and before the scale
    for kw in (dict(v_heads=3), dict(v_heads=0), dict(heads=4, v_heads=2)):
        _rejected(lib, entry, SGF_E_INVALID, **kw)
        assert b"v_heads" in lib.sgf_last_error()
    _rejected(lib, entry, SGF_E_INVALID, n=-1)
    _rejected(lib, entry, SGF_E_INVALID, l=-1)


@pytest.mark.parametrize("entry", ENTRIES)
def test_scale_must_be_finite_and_positive(lib, entry):
    for dtype in (F32, BF16):
        for scale in (0.0, -0.0, -1.0, float("inf"), -float("inf"), float("nan")):
            _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, scale=scale)
            assert b"scale" in lib.sgf_last_error(), lib.sgf_last_error()
            _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, scale=scale, q=None)       # before the pointers
            assert b"scale" in lib.sgf_last_error(), lib.sgf_last_error()
            _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, scale=scale, n=0)          # and for an empty problem too
        for scale in (1.0, 0.125, 1e-30, 3e38):
            assert _call(lib, entry, dtype=dtype, scale=scale, n=0) == SGF_OK, lib.sgf_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_problems(lib, entry):
    names = SIGS[entry].split()
    nothing = {a: (0 if a.startswith("ld") or a.endswith("_bytes") else None) for a in names if a not in SCALARS or a.endswith("_bytes")}
    for dtype in (F32, BF16):
        assert _call(lib, entry, n=0, dtype=dtype, **nothing) == SGF_OK, lib.sgf_last_error()     # no rows: nothing to launch
        assert _call(lib, entry, n=0, l=0, dtype=dtype, **nothing) == SGF_OK, lib.sgf_last_error()
        _rejected(lib, entry, SGF_E_INVALID, l=0, dtype=dtype)                                     # rows, and no key to sum
        assert b"l == 0" in lib.sgf_last_error()
        _rejected(lib, entry, SGF_E_INVALID, l=0, dtype=dtype, **nothing)                          # before the pointers


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_pointers(lib, entry):
    for dtype in (F32, BF16):
        for ptr, ld in _rows(entry) + [("lse", None)]:
            if ptr == "dq":
                continue
            _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **{ptr: None})
            assert b"null pointer" in lib.sgf_last_error(), lib.sgf_last_error()
            if ld is not None:
                _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **{ptr: None, ld: 8})            # before the widths
                assert b"null pointer" in lib.sgf_last_error(), lib.sgf_last_error()
    if entry != "sgf_pair_softmax_fwd":
        _rejected(lib, entry, SGF_E_WORKSPACE, workspace=None)
        _rejected(lib, entry, SGF_E_WORKSPACE, workspace_bytes=4 * 1000 * 2 - 1)
    if entry == "sgf_pair_softmax_bwd_q":
        _rejected(lib, entry, SGF_E_WORKSPACE, dq=None, lddq=0, workspace=None)                    # dq is optional: delta only


@pytest.mark.parametrize("entry", ENTRIES)
def test_leading_dimensions_and_alignment(lib, entry):
    for dtype, per16 in ((BF16, 8), (F32, 4)):
        for ptr, ld in _rows(entry):
            _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **{ld: LD - per16})
            assert b"leading dimension smaller than the width" in lib.sgf_last_error(), lib.sgf_last_error()
            _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **{ld: LD - per16, ptr: A + 2})      # before the alignment
            assert b"leading dimension smaller than the width" in lib.sgf_last_error(), lib.sgf_last_error()
            for kw in ({ptr: A + 8 if dtype == BF16 else A + 4}, {ptr: A + 2}, {ld: LD + per16 // 2}, {ld: LD + 1}):
                _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **kw)
                assert b"rows must be 16-byte aligned" in lib.sgf_last_error(), (kw, lib.sgf_last_error())
    # one shared value head: v and dv are d wide, not heads * d
    kw = dict(v_heads=1, ldv=64)
    if entry == "sgf_pair_softmax_bwd_kv":
        kw["lddv"] = 64
    assert _call(lib, entry, n=0, **kw) == SGF_OK
    _rejected(lib, entry, SGF_E_INVALID, v_heads=1, ldv=56)
    _rejected(lib, entry, SGF_E_INVALID, **{**kw, "q": None})             # the narrow v passes: the next check speaks
    assert b"null pointer" in lib.sgf_last_error()


# ---- wiring on a CPU kernel table -----------------------------------------------------------------------------------------
@pytest.fixture
def table():
    from sgformer_amd import ops
    CpuKernelsPairSoftmax.calls = {}
    prev = ops.set_kernels(CpuKernelsPairSoftmax())
    yield CpuKernelsPairSoftmax
    ops.set_kernels(prev)


def _dense(q, k, v, scale):
    w = torch.softmax(scale * torch.einsum("nhd,lhd->nlh", q, k), dim=1)
    return torch.einsum("nlh,lhd->nhd", w, v.expand(-1, q.shape[1], -1))


def _relnorm(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


@pytest.mark.parametrize("h,hv", [(1, 1), (2, 2), (3, 1)])
@pytest.mark.parametrize("scale", [1.0, 0.125])
def test_autograd_matches_the_dense_formula(table, h, hv, scale):
    from sgformer_amd import pair_attn
    gen = torch.Generator().manual_seed(7 + h + hv)
    q, k, v = torch.randn(40, h, 32, generator=gen), torch.randn(23, h, 32, generator=gen), torch.randn(23, hv, 32, generator=gen)
    g = torch.randn(40, h, 32, generator=gen)
    a = [t.clone().requires_grad_(True) for t in (q, k, v)]
    b = [t.clone().double().requires_grad_(True) for t in (q, k, v)]
    out = pair_attn.softmax_attention(*a, scale=scale)
    assert type(out.grad_fn).__name__.startswith("_SoftmaxAttention")
    out.backward(g)
    ref = _dense(*b, scale)
    ref.backward(g.double())
    assert table.calls == {"pair_softmax_fwd": [40], "pair_softmax_bwd_q": [40], "pair_softmax_bwd_kv": [40]}
    assert _relnorm(out.detach(), ref.detach()) <= 1e-6
    for x, y in zip(a, b):
        assert x.grad.shape == y.grad.shape and _relnorm(x.grad, y.grad) <= 1e-5


def test_partial_gradients_and_views(table, monkeypatch):
    """A backward that asks for dv only runs bwd_q for delta (no dq) and bwd_kv; operands sliced out of one wider buffer
    (the module's [Q | K | V]) go to the entries as they are."""
    from sgformer_amd import pair_attn
    torch.manual_seed(3)
    qkv = torch.randn(40, 3 * 2 * 32)
    q, k, v = (qkv[:, i * 64:(i + 1) * 64].reshape(40, 2, 32) for i in range(3))
    vg = v.clone().requires_grad_(True)
    pair_attn.softmax_attention(q, k, vg).square().sum().backward()
    assert table.calls == {"pair_softmax_fwd": [40], "pair_softmax_bwd_q": [40], "pair_softmax_bwd_kv": [40]}
    vr = v.clone().requires_grad_(True)
    _dense(q, k, vr, 1.0).square().sum().backward()
    assert _relnorm(vg.grad, vr.grad) <= 1e-5
    seen = {}
    fwd = table.pair_softmax_fwd
    monkeypatch.setattr(table, "pair_softmax_fwd",
                        staticmethod(lambda q, k, v, scale=1.0: (seen.update(ld=q.stride(0)), fwd(q, k, v, scale))[1]))
    pair_attn.softmax_attention(q, k, v)
    assert seen["ld"] == 192                                         # no copy: the view's leading dimension


def test_once_differentiable_and_argument_errors(table):
    from sgformer_amd import pair_attn
    torch.manual_seed(4)
    q, k, v = (torch.randn(9, 2, 32, requires_grad=True) for _ in range(3))
    out = pair_attn.softmax_attention(q, k, v)
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(out.sum(), q, create_graph=True)
    with pytest.raises(RuntimeError, match="unsupported operands"):
        pair_attn.softmax_attention(q, k[:0], v[:0])
    for scale in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="scale"):
            pair_attn.softmax_attention(q, k, v, scale=scale)


def test_supported_and_the_switch(table, monkeypatch):
    from sgformer_amd import ops, pair_attn
    q, k, v = torch.randn(40, 2, 32), torch.randn(23, 2, 32), torch.randn(23, 2, 32)
    assert pair_attn.softmax_supported(q, k, v) and pair_attn.softmax_supported(q, k, v[:, :1])
    assert pair_attn.softmax_supported(q.bfloat16(), k.bfloat16(), v.bfloat16())
    assert not pair_attn.softmax_supported(q, k, v[:, :, :16]) and not pair_attn.softmax_supported(q.double(), k.double(), v.double())
    assert not pair_attn.softmax_supported(q, k[:0], v[:0]) and not pair_attn.softmax_supported(q[:, :, ::2], k[:, :, ::2], v[:, :, ::2])
    assert not pair_attn.softmax_supported(q, k.bfloat16(), v) and not pair_attn.softmax_supported(q, k[:, :1], v[:, :1])
    assert not pair_attn.supported(q, k, v)                           # this table has no pair_sigmoid_*: the families are apart
    monkeypatch.setenv("SGF_PAIR_SOFTMAX", "1")
    assert pair_attn.use_softmax_kernels(q, k, v)
    monkeypatch.setenv("SGF_PAIR_ATTN", "0")                          # the sigmoid switch is another switch
    assert pair_attn.use_softmax_kernels(q, k, v)
    monkeypatch.setenv("SGF_PAIR_SOFTMAX", "0")
    assert not pair_attn.use_softmax_kernels(q, k, v)
    monkeypatch.delenv("SGF_PAIR_SOFTMAX")                            # unset: the size thresholds decide, per dtype
    monkeypatch.setattr(pair_attn, "SOFTMAX_MIN_PAIRS", 40 * 23 * 2 + 1)
    monkeypatch.setattr(pair_attn, "SOFTMAX_MIN_PAIRS_BF16", 40 * 23 * 2)
    assert not pair_attn.use_softmax_kernels(q, k, v)
    assert pair_attn.use_softmax_kernels(q.bfloat16(), k.bfloat16(), v.bfloat16())
    monkeypatch.setattr(pair_attn, "SOFTMAX_MIN_PAIRS", 40 * 23 * 2)
    assert pair_attn.use_softmax_kernels(q, k, v)
    monkeypatch.setenv("SGF_PAIR_SOFTMAX", "1")
    prev = ops.set_kernels(CpuKernels())                              # the stock CPU table has no pair_softmax_*
    try:
        assert not pair_attn.softmax_supported(q, k, v) and not pair_attn.use_softmax_kernels(q, k, v)
    finally:
        ops.set_kernels(prev)
    assert table.calls == {}
