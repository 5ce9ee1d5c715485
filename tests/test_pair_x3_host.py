"""The split-bf16 arm of the all-pair attention (csrc/pair_attn.hip, include/sgf.h block N9) without a GPU.

1. The argument checks of the ten sgf_pair_sigmoid_x3_* / sgf_pair_softmax_x3_* entries through ctypes: the checks
   tests/test_pair_attn_host.py and tests/test_pair_softmax_host.py make of the exact entries, with the dtype rule turned
   round (SGF_F32_BF16X3 only).
2. The wiring: which entry and dtype code sgformer_amd/pair_attn.py launches under which float32 matmul precision.
3. An emulation of the arm's arithmetic in fp64 (every product as hi.hi + hi.lo + lo.hi of operands split as the kernels
   split them; everything else exact), held to HALF of the bars tests/test_gpu_pair_x3.py holds the kernels to, on the
   cases that file runs (which it imports from here), and shown to miss the cross-term cases when one term is dropped.

The bars (the GPU file asserts them; W: the fp64 attention weights, dz_ij = 2^-14 scale (|q| |k|^T)_ij: the bound of one split
product, tests/test_gpu_attn_f32x.py BOUND):
  out, per element:   1e-4 max|v| + 2 sum_j W_ij |v_j - out_i| dz_ij + 2^-14 sum_j W_ij |v_j|
                      (the exact fp32 arm's bar; twice the first-order response of out to a score error, d out_i / d z_ij =
                      W_ij (v_j - out_i) for the softmax and no larger for the sigmoid; the second product)
  lse (softmax):      1e-5 max(1, |lse|) + max_j dz_ij
  rowsum (sigmoid):   1e-5 r + sum_j dz_ij / 4                          (|d sigmoid / dz| <= 1 / 4)
  gradients:          ||err|| <= 2e-4 (||ref|| + 1e-2 gmax) on the cases whose scores are moderate (scale 0.125): three
                      chained products at 3 * 2^-16 each; a dropped lo term is a 2^-9 operand error, ten times the bar."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SGF_OK, SGF_E_INVALID, SGF_E_WORKSPACE, SGF_E_UNSUPPORTED = 0, -1, -2, -4
F32, BF16, F32X = 0, 1, 2
A = 0x10000
BIG = 1 << 40
ARMS = ("sigmoid", "softmax")
WIDTHS = (32, 64, 128)             # the widths of the x3 families (none was dropped: no kernel of any width spills)


def _sigs(arm):
    s = " scale" if arm == "softmax" else ""
    saved = "lse" if arm == "softmax" else "rowsum"
    p = f"sgf_pair_{arm}_x3_"
    return {
        p + "fwd": f"q ldq k ldk v ldv n l heads v_heads d dtype{s} out ldo {saved} stream",
        p + "bwd_q": f"g ldg out ldo {saved} q ldq k ldk v ldv n l heads v_heads d dtype{s} dq lddq workspace workspace_bytes stream",
        p + "bwd_kv": f"g ldg {saved} q ldq k ldk v ldv n l heads v_heads d dtype{s} dk lddk dv lddv workspace workspace_bytes "
                      "stream",
    }


SIGS = {**_sigs("sigmoid"), **_sigs("softmax")}
SCALARS = dict(n=1000, l=900, heads=2, v_heads=2, d=64, dtype=F32X, scale=0.125, workspace_bytes=BIG, stream=None)
LD = 2 * 64              # heads * d of the default call
ROWS = {"fwd": "q:ldq k:ldk v:ldv out:ldo", "bwd_q": "g:ldg out:ldo q:ldq k:ldk v:ldv dq:lddq",
        "bwd_kv": "g:ldg q:ldq k:ldk v:ldv dk:lddk dv:lddv"}
ENTRIES = sorted(SIGS)


@pytest.fixture(scope="module")
def lib():
    from sgformer_amd import _lib
    if not _lib.available():
        pytest.skip("libsgf.so not built (run `make`)")
    return _lib.load()


def _call(lib, entry, **kw):
    names = SIGS[entry].split()
    kw = {a: b for a, b in kw.items() if a != "scale" or "scale" in names}
    assert set(kw) <= set(names), (entry, sorted(set(kw) - set(names)))
    args = [kw[a] if a in kw else SCALARS[a] if a in SCALARS else LD if a.startswith("ld") else A for a in names]
    return getattr(lib, entry)(*args)


def _rejected(lib, entry, code, **kw):
    assert _call(lib, entry, **kw) == code, (kw, lib.sgf_last_error())
    assert lib.sgf_last_error().startswith(entry.encode() + b":"), lib.sgf_last_error()


def _rows(entry):
    return [tuple(t.split(":")) for t in ROWS[entry.split("_x3_")[1]].split()]


def _saved(entry):
    return "lse" if "softmax" in entry else "rowsum"


# ---- the header, the signatures and the queries -----------------------------------------------------------------------------
def test_every_export_is_declared_and_typed():
    from sgformer_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgf.h")).read(), flags=re.S)
    assert int(re.search(r"#define\s+SGF_VERSION\s+(\d+)", src).group(1)) >= 669
    names = ENTRIES + [f"sgf_pair_{a}_x3_{w}" for a in ARMS for w in ("supported", "lap_rows")]
    assert len(names) == 10
    for name in names:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m is not None, f"{name} not declared in include/sgf.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
        exact = name.replace("_x3_", "_")                    # argument lists identical to the exact counterparts
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[exact], name
    for entry in ENTRIES:                                     # this file's argument names are the header's, in order
        m = re.search(r"\b" + entry + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == SIGS[entry].split(), entry


@pytest.mark.parametrize("arm", ARMS)
def test_supported_table(lib, arm):
    sup = getattr(lib, f"sgf_pair_{arm}_x3_supported")
    for d in (16, 32, 48, 64, 128, 256):
        for h in (0, 1, 8, 9):
            for hv in (0, 1, 2, h):
                for dtype in (F32, BF16, F32X, 3, 7):
                    want = int(d in WIDTHS and 1 <= h <= 8 and hv in (1, h) and dtype == F32X)
                    assert sup(h, hv, d, dtype) == want, (h, hv, d, dtype)


@pytest.mark.parametrize("arm", ARMS)
def test_lap_rows_is_monotone_in_laps(lib, arm):
    lap = getattr(lib, f"sgf_pair_{arm}_x3_lap_rows")
    for which in (0, 1, 2):
        for d in WIDTHS:
            rows = [lap(which, 2, d, F32X, laps) for laps in (1, 2, 3, 5)]
            assert all(r >= 0 for r in rows) and rows == sorted(rows), (which, d, rows)
    assert lap(3, 2, 64, F32X, 1) == -1 and lap(0, 2, 48, F32X, 1) == -1
    assert lap(0, 2, 64, F32, 1) == -1 and lap(0, 2, 64, BF16, 1) == -1
    assert lap(0, 2, 64, F32X, 0) == -1
    assert lib.sgf_last_error().startswith(f"sgf_pair_{arm}_x3_lap_rows:".encode())


def test_the_exact_entries_still_reject_the_code(lib):
    for arm in ARMS:
        assert getattr(lib, f"sgf_pair_{arm}_supported")(2, 2, 64, F32X) == 0
        assert getattr(lib, f"sgf_pair_{arm}_lap_rows")(0, 2, 64, F32X, 1) == -1
    for entry in ENTRIES:
        exact = entry.replace("_x3_", "_")
        names = SIGS[entry].split()
        args = [SCALARS[a] if a in SCALARS else LD if a.startswith("ld") else A for a in names]
        assert getattr(lib, exact)(*args) == SGF_E_UNSUPPORTED
        assert lib.sgf_last_error().startswith(exact.encode() + b":")


# ---- the launches' checks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_shapes_and_dtype_codes(lib, entry):
    for kw in (dict(d=16), dict(d=48), dict(d=256), dict(heads=0, v_heads=0), dict(heads=9, v_heads=9), dict(dtype=F32),
               dict(dtype=BF16), dict(dtype=3), dict(dtype=7)):
        _rejected(lib, entry, SGF_E_UNSUPPORTED, **kw)
        _rejected(lib, entry, SGF_E_UNSUPPORTED, q=None, **kw)             # before the pointers
        _rejected(lib, entry, SGF_E_UNSUPPORTED, n=0, **kw)                # and for an empty problem too
        _rejected(lib, entry, SGF_E_UNSUPPORTED, scale=0.0, **kw)          # and before the scale (softmax)
    for kw in (dict(v_heads=3), dict(v_heads=0), dict(heads=4, v_heads=2)):
        _rejected(lib, entry, SGF_E_INVALID, **kw)
        assert b"v_heads" in lib.sgf_last_error()
    _rejected(lib, entry, SGF_E_INVALID, n=-1)
    _rejected(lib, entry, SGF_E_INVALID, l=-1)
    for d in WIDTHS:
        assert _call(lib, entry, n=0, d=d, **{ld: 2 * d for _, ld in _rows(entry)}) == SGF_OK, lib.sgf_last_error()


@pytest.mark.parametrize("entry", [e for e in ENTRIES if "softmax" in e])
def test_scale_must_be_finite_and_positive(lib, entry):
    for scale in (0.0, -0.0, -1.0, float("inf"), -float("inf"), float("nan")):
        _rejected(lib, entry, SGF_E_INVALID, scale=scale)
        assert b"scale" in lib.sgf_last_error(), lib.sgf_last_error()
        _rejected(lib, entry, SGF_E_INVALID, scale=scale, q=None)       # before the pointers
        assert b"scale" in lib.sgf_last_error(), lib.sgf_last_error()
        _rejected(lib, entry, SGF_E_INVALID, scale=scale, n=0)          # and for an empty problem too
    for scale in (1.0, 0.125, 1e-30, 3e38):
        assert _call(lib, entry, scale=scale, n=0) == SGF_OK, lib.sgf_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_problems(lib, entry):
    names = SIGS[entry].split()
    nothing = {a: (0 if a.startswith("ld") or a.endswith("_bytes") else None) for a in names if a not in SCALARS or a.endswith("_bytes")}
    assert _call(lib, entry, n=0, **nothing) == SGF_OK, lib.sgf_last_error()              # no rows: nothing to launch
    assert _call(lib, entry, n=0, l=0, **nothing) == SGF_OK, lib.sgf_last_error()
    _rejected(lib, entry, SGF_E_INVALID, l=0)                                              # rows, and no key to sum
    assert b"l == 0" in lib.sgf_last_error()
    _rejected(lib, entry, SGF_E_INVALID, l=0, **nothing)                                   # before the pointers


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_pointers(lib, entry):
    for ptr, ld in _rows(entry) + [(_saved(entry), None)]:
        if ptr == "dq":
            continue
        _rejected(lib, entry, SGF_E_INVALID, **{ptr: None})
        assert b"null pointer" in lib.sgf_last_error(), lib.sgf_last_error()
        if ld is not None:
            _rejected(lib, entry, SGF_E_INVALID, **{ptr: None, ld: 8})                     # before the widths
            assert b"null pointer" in lib.sgf_last_error(), lib.sgf_last_error()
    if not entry.endswith("_fwd"):
        _rejected(lib, entry, SGF_E_WORKSPACE, workspace=None)
        _rejected(lib, entry, SGF_E_WORKSPACE, workspace_bytes=4 * 1000 * 2 - 1)          # the exact families' workspace query
        assert getattr(lib, entry.split("_x3_")[0] + "_workspace_bytes")(1000, 900, 2) == 4 * 1000 * 2
    if entry.endswith("_bwd_q"):
        _rejected(lib, entry, SGF_E_WORKSPACE, dq=None, lddq=0, workspace=None)            # dq is optional: delta only


@pytest.mark.parametrize("entry", ENTRIES)
def test_leading_dimensions_and_alignment(lib, entry):
    per16 = 4                                                                              # fp32 storage
    for ptr, ld in _rows(entry):
        _rejected(lib, entry, SGF_E_INVALID, **{ld: LD - per16})
        assert b"leading dimension smaller than the width" in lib.sgf_last_error(), lib.sgf_last_error()
        _rejected(lib, entry, SGF_E_INVALID, **{ld: LD - per16, ptr: A + 2})               # before the alignment
        assert b"leading dimension smaller than the width" in lib.sgf_last_error(), lib.sgf_last_error()
        for kw in ({ptr: A + 4}, {ptr: A + 8}, {ptr: A + 2}, {ld: LD + per16 // 2}, {ld: LD + 1}):
            _rejected(lib, entry, SGF_E_INVALID, **kw)
            assert b"rows must be 16-byte aligned" in lib.sgf_last_error(), (kw, lib.sgf_last_error())
        assert _call(lib, entry, n=0, **{ld: LD + per16, ptr: A + 16}) == SGF_OK
    kw = dict(v_heads=1, ldv=64)                              # one shared value head: v and dv are d wide, not heads * d
    if entry.endswith("_bwd_kv"):
        kw["lddv"] = 64
    assert _call(lib, entry, n=0, **kw) == SGF_OK
    _rejected(lib, entry, SGF_E_INVALID, v_heads=1, ldv=60)
    _rejected(lib, entry, SGF_E_INVALID, **{**kw, "q": None})             # the narrow v passes: the next check speaks
    assert b"null pointer" in lib.sgf_last_error()


# ---- wiring: which entry a launch takes ---------------------------------------------------------------------------------------
class precision:
    """torch.set_float32_matmul_precision(p) for a block; always back to 'highest'"""

    def __init__(self, p):
        self.p = p

    def __enter__(self):
        torch.set_float32_matmul_precision(self.p)

    def __exit__(self, *exc):
        torch.set_float32_matmul_precision("highest")


def _recorded(monkeypatch):
    from sgformer_amd import pair_attn
    calls = []

    def record(device, name, *args):
        from sgformer_amd import _lib
        argn = SIGS.get(name, SIGS.get(name.replace("sgf_pair_sigmoid_", "sgf_pair_sigmoid_x3_").replace(
            "sgf_pair_softmax_", "sgf_pair_softmax_x3_"))).split()
        assert len(args) == len(argn) - 1 == len(_lib.SIGNATURES[name][1]) - 1, name       # (the stream goes last)
        kw = dict(zip(argn, args))
        if "scale" in kw:
            assert kw["scale"] == 0.25
        calls.append((name, kw["dtype"]))
    monkeypatch.setattr(pair_attn, "_launch", record)
    return calls


def _launch_all(dtype):
    from sgformer_amd.pair_attn import _Hip
    q, k, v, g = (torch.zeros(5, 2, 64, dtype=dtype), torch.zeros(7, 2, 64, dtype=dtype), torch.zeros(7, 1, 64, dtype=dtype),
                  torch.zeros(5, 2, 64, dtype=dtype))
    out, rs = _Hip.pair_sigmoid_fwd(q, k, v)
    _, delta = _Hip.pair_sigmoid_bwd_q(g, out, rs, q, k, v)
    _Hip.pair_sigmoid_bwd_kv(g, rs, delta, q, k, v)
    out, lse = _Hip.pair_softmax_fwd(q, k, v, 0.25)
    _, delta = _Hip.pair_softmax_bwd_q(g, out, lse, q, k, v, 0.25)
    _Hip.pair_softmax_bwd_kv(g, lse, delta, q, k, v, 0.25)


def _names(x3, code):
    return [(f"sgf_pair_{arm}_{'x3_' if x3 else ''}{w}", code) for arm in ARMS for w in ("fwd", "bwd_q", "bwd_kv")]


def test_the_precision_setting_picks_the_entry(lib, monkeypatch):
    from sgformer_amd import kernels
    calls = _recorded(monkeypatch)
    try:
        torch.set_float32_matmul_precision("highest")
        _launch_all(torch.float32)
        assert calls == _names(False, F32)
        del calls[:]
        torch.set_float32_matmul_precision("high")
        _launch_all(torch.float32)
        assert calls == _names(True, F32X)
        del calls[:]
        _launch_all(torch.bfloat16)                                          # bf16 storage: untouched
        assert calls == _names(False, BF16)
        del calls[:]
        # a library that does not take the shape on the split kernels: exactly the exact call
        monkeypatch.setattr(kernels, "_x3_cache", {(f"sgf_pair_{arm}_x3_supported", 2, 1, 64): False for arm in ARMS})
        _launch_all(torch.float32)
        assert calls == _names(False, F32)
        del calls[:]
        torch.set_float32_matmul_precision("highest")
        _launch_all(torch.float32)
        assert calls == _names(False, F32)
    finally:
        torch.set_float32_matmul_precision("highest")


def test_third_threshold(lib, monkeypatch):
    """unset switch: fp32 under 'high' on the HIP table is held to the *_X3 threshold, everything else to what it was"""
    from sgformer_amd import pair_attn
    assert pair_attn.PAIR_MIN_PAIRS_X3 > 0 and pair_attn.SOFTMAX_MIN_PAIRS_X3 > 0
    monkeypatch.delenv("SGF_PAIR_ATTN", raising=False)
    monkeypatch.delenv("SGF_PAIR_SOFTMAX", raising=False)
    monkeypatch.setattr(pair_attn, "_supported", lambda q, k, v, family: True)
    monkeypatch.setattr(pair_attn, "_table", lambda entry="": pair_attn._Hip)
    q, k, v = torch.zeros(10, 2, 64), torch.zeros(10, 2, 64), torch.zeros(10, 2, 64)
    for fam, use, lo, x3 in (("pair_sigmoid", pair_attn.use_kernels, "PAIR_MIN_PAIRS", "PAIR_MIN_PAIRS_X3"),
                             ("pair_softmax", pair_attn.use_softmax_kernels, "SOFTMAX_MIN_PAIRS", "SOFTMAX_MIN_PAIRS_X3")):
        try:
            monkeypatch.setattr(pair_attn, lo, 201)
            monkeypatch.setattr(pair_attn, x3, 200)
            assert not use(q, k, v)                                          # 'highest': 200 entries < 201
            torch.set_float32_matmul_precision("high")
            assert use(q, k, v)                                              # 'high': 200 >= 200
            assert not use(q[:9], k, v)
            monkeypatch.setattr(pair_attn, lo, 0)
            monkeypatch.setattr(pair_attn, x3, 201)
            assert not use(q, k, v)
            torch.set_float32_matmul_precision("highest")
            assert use(q, k, v)
        finally:
            torch.set_float32_matmul_precision("highest")


# ---- the cases of tests/test_gpu_pair_x3.py, their fp64 references and their bars ------------------------------------------------
SHAPES = [(1, 1), (31, 33), (33, 31), (70, 193), (257, 255), (1031, 1031)]
HEADS = [(1, 1), (3, 1), (3, 3)]
BOUND = 2.0 ** -14                 # one split product: |error| <= BOUND |a| . |b| (tests/test_gpu_attn_f32x.py)
GRAD_TOL_X3 = 2e-4


def dense64(arm, q, k, v, g, scale=1.0):
    """(out, saved, dq, dk, dv, W) of the dense formula in fp64; saved: lse (softmax) / rowsum (sigmoid); W [n, l, h]"""
    h = q.shape[1]
    ops = [t.clone().requires_grad_(True) for t in (q, k, v)]
    z = scale * torch.einsum("nhd,lhd->nlh", ops[0], ops[1])
    if arm == "softmax":
        w = torch.softmax(z, dim=1)
        saved = torch.logsumexp(z.detach(), dim=1)
    else:
        s = torch.sigmoid(z)
        saved = s.detach().sum(1)
        w = s / s.sum(1, keepdim=True)
    out = torch.einsum("nlh,lhd->nhd", w, ops[2].expand(-1, h, -1))
    out.backward(g)
    return out.detach(), saved, ops[0].grad, ops[1].grad, ops[2].grad, w.detach()


def bars(arm, q, k, v, scale, ref):
    """(out bar [n, h, d], saved bar [n, h]) of the docstring, from the fp64 reference"""
    out, saved, w = ref[0], ref[1], ref[5]
    n, h, d = q.shape
    ve = v.expand(-1, h, -1)
    dz = BOUND * scale * torch.einsum("nhd,lhd->nlh", q.abs(), k.abs())
    wdz = (w * dz).float()
    resp = torch.empty(n, h, d, dtype=torch.float64)
    step = max(1, (1 << 24) // max(1, k.shape[0] * d))
    for t in range(h):                                            # sum_j W_ij dz_ij |v_j - out_i|, in row chunks
        vt = ve[:, t].float()
        for i0 in range(0, n, step):
            o = out[i0:i0 + step, t].float()
            resp[i0:i0 + step, t] = torch.einsum("nl,nld->nd", wdz[i0:i0 + step, :, t], (vt[None] - o[:, None]).abs()).double()
    out_bar = 1e-4 * float(v.abs().max()) + 2.0 * resp + BOUND * torch.einsum("nlh,lhd->nhd", w, ve.abs())
    if arm == "softmax":
        saved_bar = 1e-5 * saved.abs().clamp_min(1.0) + dz.max(1).values
    else:
        saved_bar = 1e-5 * saved + 0.25 * dz.sum(1)
    return out_bar, saved_bar


_cases = {}


def _cached(key, make):
    if key not in _cases:
        arm, q, k, v, g, scale = make()
        ref = dense64(arm, q, k, v, g, scale)
        _cases[key] = (arm, q, k, v, g, scale, ref[:5], bars(arm, q, k, v, scale, ref))
    return _cases[key]


def random_case(arm, n, l, h, hv, d, scale, zmax=None):
    """fp32 operands that bf16 does not hold (as fp64 tensors), the fp64 reference and the bars.  `scale`: the softmax's score
    scale; the sigmoid arm has none, there it multiplies q."""
    def make():
        gen = torch.Generator().manual_seed(11 + n + 3 * l + 5 * h + 7 * hv + 13 * d)

        def rnd(*shape, s=1.0):
            return (s * torch.randn(*shape, generator=gen)).float().double()
        q, k = rnd(n, h, d, s=2.0 / d ** 0.5), rnd(l, h, d, s=2.0 / d ** 0.5)
        if zmax is not None:
            q = (q * (zmax / float(torch.einsum("nhd,lhd->nlh", q, k).abs().max()))).float().double()
        v, g = rnd(l, hv, d), rnd(n, h, d)
        if arm == "sigmoid":
            return arm, (scale * q).float().double(), k, v, g, 1.0
        return arm, q, k, v, g, scale
    return _cached(("random", arm, n, l, h, hv, d, scale, zmax), make)


def moving_case(arm, block):
    """n = 130, l = 1031, H = 2, Hv = 1, D = 64: feature 0 lifts the scores by 40 per `block` keys (64: to 640, 32: to 1280) over
    a random part of a few units, the construction of tests/test_gpu_pair_softmax.py::_moving_case('rising') on operands that
    bf16 does not hold (feature 0 itself is exact: q = 64, k = 0.625 b)."""
    def make():
        n, l, h, hv, d = 130, 1031, 2, 1, 64
        gen = torch.Generator().manual_seed(177 + block)

        def rnd(*shape, s=1.0):
            return (s * torch.randn(*shape, generator=gen)).float().double()
        q, k = rnd(n, h, d, s=2.0 / d ** 0.5), rnd(l, h, d, s=2.0 / d ** 0.5)
        q[:, :, 0] = 64.0
        k[:, :, 0] = (0.625 * (torch.arange(l) // block).double())[:, None]
        return arm, q, k, rnd(l, hv, d), rnd(n, h, d), 1.0
    return _cached(("moving", arm, block), make)


def _table(rows, cols, shift):
    """the asymmetric table of tests/test_gpu_pair_attn.py::_exact_case: B[r][m] = (7 r' + 3 m + (r' >> 3)) mod 5 < 2, r' = r + shift"""
    r = torch.arange(rows)[:, None] + shift
    return ((7 * r + 3 * torch.arange(cols)[None, :] + (r >> 3)) % 5) < 2


def cross_case(kind, n, l, h, hv, d):
    """(q, k, v, g, count [n, h], out_ref, dv_ref): z is exactly 32 or -128 through ONE of the three products of z.
    'q_lo': k_j[2m] = a_jm, k_j[2m+1] = -a_jm with a in {2^14, -2^16}; q_i[2m] = 1 + e_im, q_i[2m+1] = 1 - e_im with e = 2^-10 at
    m = (i + 3 t) mod D/2 (head t) and 0 elsewhere: hi_q = 1, hi_q . k_j = 0, z_ij = lo_q . k_j = 2^-9 a_j,m(i).  'k_lo': the
    roles of q and k exchanged.  A row the table leaves without a key keeps key i mod l, as in _exact_case."""
    key = ("cross", kind, n, l, h, hv, d)
    if key not in _cases:
        gen = torch.Generator().manual_seed(n * 137 + l * 11 + h * 3 + hv + d)
        half = d // 2
        q, k = torch.zeros(n, h, d, dtype=torch.float64), torch.zeros(l, h, d, dtype=torch.float64)
        mask = torch.empty(h, n, l, dtype=torch.float64)
        i, j = torch.arange(n), torch.arange(l)
        for t in range(h):
            if kind == "q_lo":
                b = _table(l, half, 3 * t)                            # [l, half]: a_jm
                c = (i + 3 * t) % half
                empty = (b[:, c].sum(0) == 0).nonzero().view(-1)
                b[empty % l, c[empty]] = True
                a = torch.where(b, 2.0 ** 14, -2.0 ** 16)
                k[:, t, 0::2], k[:, t, 1::2] = a, -a
                e = torch.zeros(n, half, dtype=torch.float64)
                e[i, c] = 2.0 ** -10
                q[:, t, 0::2], q[:, t, 1::2] = 1.0 + e, 1.0 - e
                mask[t] = b[:, c].t().double()
            else:
                b = _table(n, half, 3 * t)                            # [n, half]: a_im
                c = (j + 3 * t) % half
                empty = (b[:, c].sum(1) == 0).nonzero().view(-1)
                b[empty, c[empty % l]] = True
                a = torch.where(b, 2.0 ** 14, -2.0 ** 16)
                q[:, t, 0::2], q[:, t, 1::2] = a, -a
                e = torch.zeros(l, half, dtype=torch.float64)
                e[j, c] = 2.0 ** -10
                k[:, t, 0::2], k[:, t, 1::2] = 1.0 + e, 1.0 - e
                mask[t] = b[:, c].double()
        z = torch.einsum("nhd,lhd->nlh", q, k)
        assert torch.equal(z, torch.where(mask.permute(1, 2, 0) > 0, 32.0, -128.0).double())
        v = torch.randint(-3, 4, (l, hv, d), generator=gen).double()
        g = torch.randint(-2, 3, (n, h, d), generator=gen).double()
        count = mask.sum(2)
        assert float(count.min()) >= 1
        ve = v.expand(-1, h, -1)
        out = torch.stack([mask[t] @ ve[:, t] / count[t][:, None] for t in range(h)], 1)
        dv = torch.stack([(mask[t] / count[t][:, None]).t() @ g[:, t] for t in range(h)], 1)
        if hv == 1:
            dv = dv.sum(1, keepdim=True)
        _cases[key] = (q, k, v, g, count.t().contiguous(), out, dv)
    return _cases[key]


def v_lo_case(n, l, h, hv, d):
    """q = 0: every score is equal; v_j[f] = (-1)^j + t_jf 2^-10 with t in {0, 1}: hi_v = +-1 cancels over the l keys (l a power of
    two), out = 2^-10 mean_j t_jf exactly, carried by P_hi . V_lo alone.  (q, k, v, g, count, out_ref, dv_ref) as cross_case."""
    key = ("v_lo", n, l, h, hv, d)
    if key not in _cases:
        assert l >= 256 and l & (l - 1) == 0
        gen = torch.Generator().manual_seed(n * 139 + l * 13 + h * 3 + hv + d)
        q = torch.zeros(n, h, d, dtype=torch.float64)
        k = torch.randint(-3, 4, (l, h, d), generator=gen).double()
        t = torch.randint(0, 2, (l, hv, d), generator=gen).double()
        v = torch.where(torch.arange(l) % 2 == 0, 1.0, -1.0).double()[:, None, None] + t * 2.0 ** -10
        g = torch.randint(-2, 3, (n, h, d), generator=gen).double()
        out = (2.0 ** -10 * t.mean(0, keepdim=True)).expand(n, h, d).contiguous()
        dv = (g.sum(0, keepdim=True) / l).expand(l, h, d)
        dv = dv.sum(1, keepdim=True) if hv == 1 else dv
        _cases[key] = (q, k, v, g, torch.full((n, h), float(l), dtype=torch.float64), out, dv.contiguous())
    return _cases[key]


RANDOM_SCALES = (1.0, 0.125)
# (1, 1) is replaced by (1, 2) in the random cases: with one key out = v, the true dq and dk are 0 and what is left of them is
# the rounding of g . v - delta against a bar of 2e-6 gmax; the emulation sits at 0.74 of the bar there (sigmoid, D = 32),
# above the half it must keep to.  The exact-mask and cross-term cases keep (1, 1).
RANDOM_SHAPES = [(1, 2)] + SHAPES[1:]
V_LO_SHAPES = [(70, 256), (257, 512)]


def random_params():
    return [(arm, d, h, hv, s) for arm in ARMS for d in WIDTHS for h, hv in HEADS for s in RANDOM_SCALES]


# ---- the emulation ----------------------------------------------------------------------------------------------------------------
def split(a):
    """hi, lo of fp32 values held in an fp64 tensor: hi = bf16(a), lo = bf16(a - hi), lo = 0 where hi is not finite"""
    a32 = a.float()
    hi = a32.bfloat16().float()
    lo = torch.where(torch.isfinite(hi), (a32 - hi).bfloat16().float(), torch.zeros_like(hi))
    return hi.double(), lo.double()


class Emu:
    """The arm's arithmetic: every product is hi.hi + hi.lo + lo.hi in fp64 of operands rounded to fp32 and split; `drop` names
    an operand whose lo term is left out of every product it enters ('q', 'k', 'v': the three cross-term cases)."""

    def __init__(self, drop=None):
        self.drop = drop

    def prod(self, eq, a, b, na="", nb=""):
        ah, al = split(a)
        bh, bl = split(b)
        r = torch.einsum(eq, ah, bh)
        if nb != self.drop:
            r = r + torch.einsum(eq, ah, bl)
        if na != self.drop:
            r = r + torch.einsum(eq, al, bh)
        return r

    def run(self, arm, q, k, v, g, scale=1.0):
        h = q.shape[1]
        ve = v.expand(-1, h, -1)
        z = scale * self.prod("nhd,lhd->nlh", q, k, "q", "k")
        if arm == "softmax":
            m = z.max(1, keepdim=True).values
            p = torch.exp(z - m)
            r = p.sum(1)
            saved = m[:, 0] + torch.log(r)
        else:
            p = torch.sigmoid(z)
            r = saved = p.sum(1)
        out = (self.prod("nlh,lhd->nhd", p, ve, "p", "v") / r[:, :, None]).float().double()
        delta = (g * out).sum(2)
        gv = self.prod("nhd,lhd->nlh", g, ve, "g", "v")
        if arm == "softmax":
            w = torch.exp(z - saved[:, None, :])
            dz = scale * w * (gv - delta[:, None, :])
        else:
            w = p / r[:, None, :]
            dz = p * (1.0 - p) * ((gv - delta[:, None, :]) / r[:, None, :])
        dq = self.prod("nlh,lhd->nhd", dz, k, "dz", "k")
        dk = self.prod("nlh,nhd->lhd", dz, q, "dz", "q")
        dv = self.prod("nlh,nhd->lhd", w, g, "w", "g")
        if v.shape[1] == 1:
            dv = dv.sum(1, keepdim=True)
        return out, saved, dq, dk, dv


def worst_ratios(got, ref, bar, grad_tol):
    """(forward: the worst error / bar over out and the saved row value, backward: over the three gradients)"""
    fwd = max(float(((got[0] - ref[0]).abs() / bar[0]).max()), float(((got[1] - ref[1]).abs() / bar[1]).max()))
    gmax = max(float(t.norm()) for t in ref[2:5])
    bwd = max(float((a - b).norm()) / (grad_tol * (float(b.norm()) + 1e-2 * gmax)) for a, b in zip(got[2:5], ref[2:5]))
    return fwd, bwd


@pytest.mark.parametrize("arm,d,h,hv,scale", random_params())
def test_emulation_meets_half_the_bars_on_the_random_cases(arm, d, h, hv, scale):
    for n, l in RANDOM_SHAPES:
        arm_, q, k, v, g, sc, ref, bar = random_case(arm, n, l, h, hv, d, scale)
        fwd, bwd = worst_ratios(Emu().run(arm, q, k, v, g, sc), ref, bar, GRAD_TOL_X3)
        print(f"X3_EMU random[{arm},{n}x{l},H{h},Hv{hv},D{d},s{scale}] fwd {fwd:.4f} bwd {bwd:.4f}")
        assert fwd <= 0.5, (n, l, fwd)
        assert scale != 0.125 or bwd <= 0.5, (n, l, bwd)


@pytest.mark.parametrize("arm", ARMS)
def test_emulation_meets_half_the_forward_bar_on_the_large_scores(arm):
    cases = [moving_case(arm, 64), moving_case(arm, 32)]
    if arm == "softmax":
        cases.append(random_case(arm, 257, 255, 2, 2, 64, 1.0, zmax=3000.0))
    else:
        cases.append(random_case(arm, 257, 255, 2, 2, 64, 1.0, zmax=30.0))
    for arm_, q, k, v, g, sc, ref, bar in cases:
        got = Emu().run(arm, q, k, v, g, sc)
        fwd, bwd = worst_ratios(got, ref, bar, GRAD_TOL_X3)
        print(f"X3_EMU large[{arm},{q.shape[0]}x{k.shape[0]}] fwd {fwd:.4f} bwd (not asserted) {bwd:.4f}")
        assert fwd <= 0.5
        assert all(bool(torch.isfinite(t).all()) for t in got)


def _cross_errors(arm, case, drop):
    """(max |out - masked mean| in ulps of fp32, whether the saved row value is exact) of the emulation on a cross-term case"""
    q, k, v, g, count, out_ref, dv_ref = case
    out, saved = Emu(drop).run(arm, q, k, v, g)[:2]
    ulp = 2.0 ** -23 * torch.exp2(torch.floor(torch.log2(out_ref.abs().clamp_min(1e-30))))
    return float(((out - out_ref).abs() / ulp).max())


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("d", WIDTHS)
def test_cross_term_cases_discriminate(arm, d):
    """with all three terms the emulation returns the masked mean; with the case's own term dropped it does not (it returns the
    uniform average, or 0), and a case does not notice a term it was not built for going missing in the forward"""
    for kind, drop in (("q_lo", "q"), ("k_lo", "k")):
        for n, l in [(33, 31), (70, 193)]:
            case = cross_case(kind, n, l, 3, 1, d)
            assert _cross_errors(arm, case, None) <= 1.0, (kind, n, l)
            assert _cross_errors(arm, case, drop) > 1e3, (kind, n, l)
    case = v_lo_case(70, 256, 3, 3, d)
    assert _cross_errors(arm, case, None) <= 1.0
    out = Emu("v").run(arm, *case[:4])[0]
    assert float(out.abs().max()) == 0.0 and float(case[5].abs().min()) > 0.0
