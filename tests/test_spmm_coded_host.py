"""The 12-bit coded operand rows of sgf_spmm_coded, on the CPU: the numpy codec the GPU tests judge the kernels with
(tests/coded_rows.py) round-trips every kind of row bit for bit and escapes exactly the rows the format cannot hold; the scaled
product the gather forms is the dense product as an exact rational; the tag rule of the scaled values; the new entries are
declared, bound, exported and on the kernel table, and reject what they cannot take before any HIP call."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import coded_rows as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["sgf_spmm_coded_bytes", "sgf_spmm_coded_supported", "sgf_spmm_code_rows", "sgf_spmm_code_values", "sgf_spmm_coded"]
A = 0x10000              # a 64 KiB-aligned dummy address, never dereferenced
BF16, F32 = 1, 0


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _bf16_as_f32(rows):
    return (rows.astype(np.uint32) << 16).view(np.float32)


@pytest.mark.parametrize("make", [C.gaussian, C.gaussian_scaled, C.relu_relu])
def test_round_trip_random_rows(make):
    rows = make(2000, seed=3)
    slots, scale, escaped = C.encode(rows)
    assert slots.shape == (2000, C.SLOT) and escaped == int((scale == C.ESCAPED).sum())
    assert escaped <= 0.05 * 2000                       # (2.5 % / 2.6 % / 1.8 % on 200 000 rows)
    keep = scale != C.ESCAPED
    assert np.array_equal(C.decode(slots, scale)[keep], rows[keep])
    assert not slots[~keep].any()
    dec = C.decode_floats(slots)[keep]
    e = (dec >> 23) & 0xFF
    assert ((e <= 15) & ((dec & 0xFFFF) == 0)).all()    # ±0 or a normal float of [2^-126, 2^-111)
    assert (((dec & 0x7FFFFFFF) == 0) == ((rows[keep] & 0x7FFF) == 0)).all()


def test_zero_rows_and_negative_zero():
    rows = np.zeros((3, C.D), dtype=np.uint16)
    rows[1] = 0x8000
    rows[2, ::3] = 0x8000
    slots, scale, escaped = C.encode(rows)
    assert escaped == 0 and (scale == 15).all()
    assert np.array_equal(C.decode(slots, scale), rows)
    assert np.array_equal(C.decode_floats(slots), rows.astype(np.uint32) << 16)      # ±0 decodes to ±0, no select


def test_window_of_14_binades():
    base = np.full(C.D, 0x4000, dtype=np.uint16)                 # 2.0: Ek = 128
    fits, out = base.copy(), base.copy()
    fits[17] = 0x4000 - (14 << 7) | 0x8055                       # 14 binades under, negative, a mantissa
    out[17] = 0x4000 - (15 << 7)
    slots, scale, escaped = C.encode(np.stack([fits, out]))
    assert scale.tolist() == [128, C.ESCAPED] and escaped == 1
    assert np.array_equal(C.decode(slots, scale)[0], fits)
    assert (C.decode_floats(slots)[0, 17] >> 23) & 0xFF == 1     # e = 1, the bottom of the window


@pytest.mark.parametrize("bits", [0x0001, 0x807F, 0x7F80, 0xFF80, 0x7FC0, 0xFFFF])
def test_subnormal_inf_nan_escape(bits):
    rows = C.gaussian(4, seed=1)
    rows[2, 200] = bits
    scale = C.encode(rows)[1]
    assert scale[2] == C.ESCAPED and C.row_scale(rows[2:3])[0] == C.ESCAPED


def test_scale_at_both_ends():
    lo = np.full(C.D, 0x0080, dtype=np.uint16)                   # Ek = 1, the smallest normals
    lo[5] = 0x80FF
    hi = np.full(C.D, 0x7F7F, dtype=np.uint16)                   # Ek = 254, the largest finite
    hi[9] = (240 << 7) | 0x8001                                  # 14 binades under
    rows = np.stack([lo, hi])
    slots, scale, escaped = C.encode(rows)
    assert scale.tolist() == [1, 254] and escaped == 0
    assert np.array_equal(C.decode(slots, scale), rows)
    e = (C.decode_floats(slots) >> 23) & 0xFF
    assert e[0].max() == 15 and e[1].max() == 15 and e[1, 9] == 1


def test_scaled_product_is_the_dense_product_exactly():
    """float32(v * 2^s) * decode(code) == float32(v) * float32(x) as rationals, so an FMA of either rounds to the same bits."""
    rng = np.random.default_rng(7)
    rows = np.concatenate([C.gaussian(40, 1), C.gaussian_scaled(40, 2), C.relu_relu(40, 3)])
    slots, scale, _ = C.encode(rows)
    keep = np.flatnonzero(scale != C.ESCAPED)
    colind = rng.choice(keep, size=600).astype(np.int32)
    val = rng.uniform(0.01, 1.0, size=600).astype(np.float32)
    vc, neg = C.code_values(colind, val, scale)
    # (rows scaled up by 2^16 or more push v * 2^(E - 15) past the largest float: those entries are tagged and stay dense)
    tagged = vc.view(np.uint32) >> 31 != 0
    assert neg == 0 and tagged.sum() < 150 and np.array_equal(np.abs(vc[tagged]), val[tagged])
    assert (scale[colind[tagged]].astype(int) - 15 + ((val[tagged].view(np.uint32) >> 23) & 0xFF) > 254).all()
    dec = _f32(C.decode_floats(slots))
    dense = _bf16_as_f32(rows)
    checked = 0
    for k in np.flatnonzero(~tagged):
        col = int(rng.integers(0, C.D))
        a = Fraction(float(vc[k])) * Fraction(float(dec[colind[k], col]))
        b = Fraction(float(val[k])) * Fraction(float(dense[colind[k], col]))
        assert a == b, (k, col)
        checked += b != 0
    assert checked > 300
    # the factor is the power of two the scale byte names
    k = int(np.flatnonzero(~tagged)[0])
    assert Fraction(float(vc[k])) == Fraction(float(val[k])) * Fraction(2) ** (int(scale[colind[k]]) - 15)


def test_value_tag_rule():
    scale = np.array([15, 254, 1, C.ESCAPED, 127], dtype=np.uint8)
    tiny, huge = np.float32(2.0 ** -120), np.float32(2.0 ** 100)
    colind = np.array([0, 0, 1, 2, 3, 4, 4, 4, 0, 4, 3], dtype=np.int32)
    val = np.array([0.5, 0.0, huge, tiny, 0.25, 0.75, np.float32(1e-45), np.inf, -0.5, np.nan, -0.0], dtype=np.float32)
    vc, neg = C.code_values(colind, val, scale)
    u, uv = vc.view(np.uint32), val.view(np.uint32)
    assert neg == 2                                              # -0.5 and -0.0: the sign bit is taken, the tag cannot mark them
    assert C.code_values(colind[:8], val[:8], scale)[1] == 0
    assert vc[0] == 0.5                                          # scale 2^0
    assert u[1] == 0x80000000                                    # a stored zero: -0.0, the tag
    assert u[2] == uv[2] ^ 0x80000000                            # 2^100 * 2^239 overflows: tagged
    assert u[3] == uv[3] ^ 0x80000000                            # 2^-120 * 2^-14 underflows: tagged
    assert u[4] == uv[4] ^ 0x80000000                            # the source row escaped
    assert vc[5] == np.float32(0.75 * 2.0 ** 112)                # 2^(127 - 15)
    assert u[6] == uv[6] ^ 0x80000000 and u[7] == uv[7] ^ 0x80000000     # a subnormal and an Inf value
    assert u[9] == uv[9] ^ 0x80000000                            # NaN keeps its payload under the tag
    assert (u[[1, 2, 3, 4, 6, 7, 9]] >> 31).all() and not (u[[0, 5]] >> 31).any()
    assert np.array_equal(np.abs(vc[[1, 2, 3, 4, 6, 7]]), val[[1, 2, 3, 4, 6, 7]])   # |val'| is the original value


def test_entries_are_declared_bound_and_on_the_table():
    from sgformer_amd import _lib, graph, kernels
    header = open(os.path.join(ROOT, "include", "sgf.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m is not None, f"{name} not declared in include/sgf.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
    assert int(re.search(r"#define\s+SGF_VERSION\s+(\d+)", header).group(1)) >= 671
    for method in ("spmm_coded", "spmm_code_rows", "spmm_code_values", "spmm_coded_supported"):
        assert callable(getattr(graph.K, method)), method
    assert "spmm_coded" in kernels.counters
    assert isinstance(graph.CODED_CLASSES, frozenset) and graph.CODED_CLASSES <= {"fwd2", "fwd3", "bwd3", "bwd2", "bwd1"}
    assert graph.CODED_MIN_NODES == 65536
    if not _lib.available():
        pytest.skip("libsgf.so not built (run `make`)")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), f"{name} not exported"


@pytest.fixture(scope="module")
def lib():
    from sgformer_amd import _lib
    if not _lib.available():
        pytest.skip("libsgf.so not built (run `make`)")
    return _lib.load()


def test_coded_bytes(lib):
    assert lib.sgf_spmm_coded_bytes(0) == 0 and lib.sgf_spmm_coded_bytes(-1) == 0
    assert lib.sgf_spmm_coded_bytes(2449029) == 2449029 * 384


def test_supported_follows_the_launch_rule(lib, monkeypatch):
    n = 2449029
    ok = lambda **kw: lib.sgf_spmm_coded_supported(*[{**dict(d=256, dtype=BF16, ldx=256, ldy=256, n_cols=n, aligned16=1), **kw}[k]
                                                     for k in ("d", "dtype", "ldx", "ldy", "n_cols", "aligned16")])
    assert lib.sgf_spmm_arm(256, BF16, 256, 256, n, 1, 0) == 2          # the wave-per-row kernel
    assert ok() == 1
    assert ok(dtype=F32) == 0 and ok(d=128) == 0 and ok(d=512) == 0 and ok(dtype=7) == 0
    assert ok(n_cols=12000000) == 0                                     # beyond 32-bit offsets
    monkeypatch.setenv("SGF_SPMM_CODED", "0")
    lib.sgf_reload_env()
    try:
        assert ok() == 0
    finally:
        monkeypatch.delenv("SGF_SPMM_CODED")
        lib.sgf_reload_env()
    assert ok() == 1
    monkeypatch.setenv("SGF_SPMM_KERNEL", "wave")
    lib.sgf_reload_env()
    try:
        assert ok() == 0
    finally:
        monkeypatch.delenv("SGF_SPMM_KERNEL")
        lib.sgf_reload_env()


def test_rejections_before_any_launch(lib):
    def rows(**kw):
        a = {**dict(x=A, ldx=256, n=10, coded=A, scale=A, esc=A), **kw}
        return lib.sgf_spmm_code_rows(a["x"], a["ldx"], a["n"], a["coded"], a["scale"], a["esc"], None)
    for kw in (dict(x=None), dict(coded=None), dict(scale=None), dict(esc=None), dict(ldx=128), dict(ldx=258), dict(x=A + 4),
               dict(coded=A + 64), dict(scale=A + 8), dict(n=-1)):
        assert rows(**kw) < 0, kw
        assert lib.sgf_last_error().startswith(b"sgf_spmm_code_rows:"), lib.sgf_last_error()

    def values(**kw):
        a = {**dict(ci=A, val=A, nnz=10, scale=A, vc=A, uns=A), **kw}
        return lib.sgf_spmm_code_values(a["ci"], a["val"], a["nnz"], a["scale"], a["vc"], a["uns"], None)
    for kw in (dict(uns=None), dict(nnz=-1), dict(ci=None), dict(val=None), dict(scale=None), dict(vc=None), dict(ci=A + 4),
               dict(val=A + 8), dict(vc=A + 4)):
        assert values(**kw) < 0, kw
        assert lib.sgf_last_error().startswith(b"sgf_spmm_code_values:"), lib.sgf_last_error()

    def mm(**kw):
        a = {**dict(vc=A, coded=A, uns=A, d=256, long_len=1024, segs=0), **kw}
        return lib.sgf_spmm_coded(A, A, A, a["vc"], A, 256, 10, a["coded"], a["uns"], A, 256, 10, a["d"], BF16, a["long_len"],
                                  a["segs"], None, 0, None)
    for kw in (dict(vc=None), dict(coded=None), dict(uns=None), dict(coded=A + 16), dict(d=6), dict(long_len=0), dict(segs=3)):
        assert mm(**kw) < 0, kw
        assert lib.sgf_last_error().startswith(b"sgf_spmm_coded:"), lib.sgf_last_error()
