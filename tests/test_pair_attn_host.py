"""All-pair sigmoid attention (csrc/pair_attn.hip, sgformer_amd/pair_attn.py) without a GPU: the argument checks of the
sgf_pair_sigmoid_* entries through ctypes (every rejection happens on the host before the first HIP call; pointers are dummy,
suitably aligned addresses that are never dereferenced), and the wiring of DIFFormer(kernel='sigmoid') on a CPU kernel table
that has the entries (tests/cpu_kernels_pair_attn.py) against the same module on the dense path."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.cpu_kernels import CpuKernels  # noqa: E402
from tests.cpu_kernels_pair_attn import CpuKernelsPairAttn  # noqa: E402

SGF_OK, SGF_E_INVALID, SGF_E_WORKSPACE, SGF_E_UNSUPPORTED = 0, -1, -2, -4
F32, BF16, F32X = 0, 1, 2
A = 0x10000
BIG = 1 << 40

SIGS = {
    "sgf_pair_sigmoid_fwd": "q ldq k ldk v ldv n l heads v_heads d dtype out ldo rowsum stream",
    "sgf_pair_sigmoid_bwd_q": "g ldg out ldo rowsum q ldq k ldk v ldv n l heads v_heads d dtype dq lddq workspace "
                              "workspace_bytes stream",
    "sgf_pair_sigmoid_bwd_kv": "g ldg rowsum q ldq k ldk v ldv n l heads v_heads d dtype dk lddk dv lddv workspace "
                               "workspace_bytes stream",
}
SCALARS = dict(n=1000, l=900, heads=2, v_heads=2, d=64, dtype=BF16, workspace_bytes=BIG, stream=None)
LD = 2 * 64              # heads * d of the default call
# (pointer, its leading dimension) of the row operands; dq of bwd_q may be null (delta only)
ROWS = {
    "sgf_pair_sigmoid_fwd": "q:ldq k:ldk v:ldv out:ldo",
    "sgf_pair_sigmoid_bwd_q": "g:ldg out:ldo q:ldq k:ldk v:ldv dq:lddq",
    "sgf_pair_sigmoid_bwd_kv": "g:ldg q:ldq k:ldk v:ldv dk:lddk dv:lddv",
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


# ---- the queries --------------------------------------------------------------------------------------------------------------
def test_supported_table(lib):
    for d in (16, 32, 48, 64, 128, 256):
        for h in (0, 1, 8, 9):
            for hv in (0, 1, 2, h):
                for dtype in (F32, BF16, F32X):
                    want = int(d in (32, 64, 128) and 1 <= h <= 8 and hv in (1, h) and dtype in (F32, BF16))
                    assert lib.sgf_pair_sigmoid_supported(h, hv, d, dtype) == want, (h, hv, d, dtype)


def test_workspace_is_linear_in_the_rows(lib):
    ws = lib.sgf_pair_sigmoid_workspace_bytes
    for h in (1, 3, 8):
        for n, l in ((1, 1), (1000, 10), (10, 1000), (40009, 40009)):
            assert ws(n, l, h) <= 4 * h * (n + l)                        # O((n + l) H): nothing of size n x l
            assert ws(2 * n, 2 * l, h) == 2 * ws(n, l, h)
            assert ws(n + 7, l + 7, h) - ws(n, l, h) == ws(7, 7, h)
        assert ws(1000, 900, h) == 4 * 1000 * h                          # delta fp32 [n, H]
    assert ws(0, 0, 2) == 0


def test_lap_rows_is_monotone_in_laps(lib):
    lap = lib.sgf_pair_sigmoid_lap_rows
    for which in (0, 1, 2):
        for d in (32, 64, 128):
            for dtype in (F32, BF16):
                rows = [lap(which, 2, d, dtype, laps) for laps in (1, 2, 3, 5)]
                assert all(r >= 0 for r in rows) and rows == sorted(rows), (which, d, dtype, rows)
    assert lap(3, 2, 64, BF16, 1) == -1 and lap(0, 2, 48, BF16, 1) == -1 and lap(0, 2, 64, F32X, 1) == -1
    assert lap(0, 2, 64, BF16, 0) == -1
    assert lib.sgf_last_error().startswith(b"sgf_pair_sigmoid_lap_rows:")


# ---- the launches' checks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_shapes_and_dtype_codes(lib, entry):
    for kw in (dict(d=16), dict(d=48), dict(d=256), dict(heads=0, v_heads=0), dict(heads=9, v_heads=9), dict(dtype=F32X),
               dict(dtype=7)):
        _rejected(lib, entry, SGF_E_UNSUPPORTED, **kw)
        _rejected(lib, entry, SGF_E_UNSUPPORTED, q=None, **kw)             # before the pointers
        _rejected(lib, entry, SGF_E_UNSUPPORTED, n=0, **kw)                # and for an empty problem too
    for kw in (dict(v_heads=3), dict(v_heads=0), dict(heads=4, v_heads=2)):
        _rejected(lib, entry, SGF_E_INVALID, **kw)
        assert b"v_heads" in lib.sgf_last_error()
    _rejected(lib, entry, SGF_E_INVALID, n=-1)
    _rejected(lib, entry, SGF_E_INVALID, l=-1)


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
        for ptr, ld in _rows(entry) + [("rowsum", None)]:
            if ptr == "dq":
                continue
            _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **{ptr: None})
            assert b"null pointer" in lib.sgf_last_error(), lib.sgf_last_error()
            if ld is not None:
                _rejected(lib, entry, SGF_E_INVALID, dtype=dtype, **{ptr: None, ld: 8})            # before the widths
                assert b"null pointer" in lib.sgf_last_error(), lib.sgf_last_error()
    if entry != "sgf_pair_sigmoid_fwd":
        _rejected(lib, entry, SGF_E_WORKSPACE, workspace=None)
        _rejected(lib, entry, SGF_E_WORKSPACE, workspace_bytes=4 * 1000 * 2 - 1)
    if entry == "sgf_pair_sigmoid_bwd_q":
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
    if entry == "sgf_pair_sigmoid_bwd_kv":
        kw["lddv"] = 64
    assert _call(lib, entry, n=0, **kw) == SGF_OK
    _rejected(lib, entry, SGF_E_INVALID, v_heads=1, ldv=56)
    _rejected(lib, entry, SGF_E_INVALID, **{**kw, "q": None})             # the narrow v passes: the next check speaks
    assert b"null pointer" in lib.sgf_last_error()


# ---- wiring on a CPU kernel table ---------------------------------------------------------------------------------------------
class _Data:
    def __init__(self, x, ei):
        self.graph = {"node_feat": x, "edge_index": ei}


@pytest.fixture
def table():
    from sgformer_amd import ops
    CpuKernelsPairAttn.calls = {}
    prev = ops.set_kernels(CpuKernelsPairAttn())
    yield CpuKernelsPairAttn
    ops.set_kernels(prev)


def _graph(n, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (4 * n,), generator=g)
    dst = torch.randint(0, n, (4 * n,), generator=g)
    keep = src != dst
    return torch.stack([torch.cat([src[keep], dst[keep]]), torch.cat([dst[keep], src[keep]])])


def _run(heads, use_weight, layers=2, output_attn=False):
    """(logits, {parameter: gradient}) of DIFFormer(kernel='sigmoid') at n = 97, d = 32, same seed every time"""
    from sgformer_amd import difformer as M
    n, f, d, c = 97, 32, 32, 5
    torch.manual_seed(11)
    m = M.DIFFormer(f, d, c, num_layers=layers, num_heads=heads, kernel='sigmoid', dropout=0.0, use_weight=use_weight)
    x = torch.randn(n, f)
    ei = _graph(n, 12)
    y = torch.randint(0, c, (n,))
    m.train()
    if output_attn:
        with torch.no_grad():
            return m.get_attentions(torch.randn(n, d)), None
    logits = m(_Data(x, ei))
    torch.nn.functional.cross_entropy(logits, y).backward()
    return logits.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def _relnorm(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


@pytest.mark.parametrize("heads,use_weight", [(1, True), (2, True), (2, False)])
def test_module_takes_the_kernels_and_matches_the_dense_path(table, monkeypatch, heads, use_weight):
    layers = 2
    monkeypatch.setenv("SGF_PAIR_ATTN", "0")
    ref_logits, ref_grads = _run(heads, use_weight, layers)
    assert table.calls == {}
    monkeypatch.setenv("SGF_PAIR_ATTN", "1")
    logits, grads = _run(heads, use_weight, layers)
    assert table.calls == {"pair_sigmoid_fwd": [97] * layers, "pair_sigmoid_bwd_q": [97] * layers,
                           "pair_sigmoid_bwd_kv": [97] * layers}
    assert _relnorm(logits, ref_logits) <= 1e-5
    assert set(grads) == set(ref_grads)
    for k in ref_grads:
        assert _relnorm(grads[k], ref_grads[k]) <= 1e-5, k


def test_paths_that_stay_dense(table, monkeypatch):
    from sgformer_amd import ops, pair_attn
    monkeypatch.setenv("SGF_PAIR_ATTN", "1")
    att, _ = _run(2, True, output_attn=True)                          # the attention maps
    assert att.shape == (2, 97, 97, 2) and table.calls == {}
    prev = ops.set_kernels(CpuKernels())                              # the stock CPU table has no pair_sigmoid_* on purpose
    try:
        _run(2, True)
    finally:
        ops.set_kernels(prev)
    assert table.calls == {}
    monkeypatch.delenv("SGF_PAIR_ATTN")                               # unset: the size threshold decides
    monkeypatch.setattr(pair_attn, "PAIR_MIN_PAIRS", 97 * 97 * 2 + 1)
    _run(2, True)
    assert table.calls == {}
    monkeypatch.setattr(pair_attn, "PAIR_MIN_PAIRS", 97 * 97 * 2)
    _run(2, True)
    assert table.calls["pair_sigmoid_fwd"] == [97, 97]


def test_free_function_and_partial_gradients(table, monkeypatch):
    """full_attention_conv with n != l; a backward that asks for dv only runs bwd_q for delta and skips nothing it needs."""
    from sgformer_amd import difformer as M, pair_attn
    torch.manual_seed(3)
    q, k, v = torch.randn(40, 2, 32), torch.randn(23, 2, 32), torch.randn(23, 2, 32)
    monkeypatch.setenv("SGF_PAIR_ATTN", "0")
    ref = M.full_attention_conv(q, k, v, 'sigmoid')
    assert table.calls == {}
    monkeypatch.setenv("SGF_PAIR_ATTN", "1")
    out = M.full_attention_conv(q, k, v, 'sigmoid')
    assert table.calls == {"pair_sigmoid_fwd": [40]} and _relnorm(out, ref) <= 1e-5
    out2, attn = M.full_attention_conv(q, k, v, 'sigmoid', output_attn=True)       # the maps: dense
    assert attn.shape == (40, 23, 2) and table.calls == {"pair_sigmoid_fwd": [40]}
    assert not pair_attn.supported(q, k, v[:, :, :16]) and not pair_attn.supported(q.double(), k.double(), v.double())
    assert not pair_attn.supported(q, k[:0], v[:0]) and not pair_attn.supported(q[:, :, ::2], k[:, :, ::2], v[:, :, ::2])
    with pytest.raises(RuntimeError, match="unsupported operands"):
        pair_attn.sigmoid_attention(q, k[:0], v[:0])
    table.calls = {}
    vg = v.clone().requires_grad_(True)
    pair_attn.sigmoid_attention(q, k, vg).square().sum().backward()
    assert table.calls == {"pair_sigmoid_fwd": [40], "pair_sigmoid_bwd_q": [40], "pair_sigmoid_bwd_kv": [40]}
    vr = v.clone().requires_grad_(True)
    M._dense_attention(q, k, vr, 'sigmoid', False)[0].square().sum().backward()
    assert _relnorm(vg.grad, vr.grad) <= 1e-5
