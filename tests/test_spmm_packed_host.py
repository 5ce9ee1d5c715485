"""The packed operand rows of the forward GCN SpMM, on the CPU: the numpy encoder / decoder the GPU tests judge the kernels
with (tests/packed_rows.py) round-trips every crafted row, and the new entries are declared, bound and exported alike and
reject what they cannot take before any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import packed_rows as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["sgf_bn_apply_packed", "sgf_spmm_packed", "sgf_spmm_packed_supported", "sgf_spmm_packed_bytes"]
A = 0x10000              # a 64 KiB-aligned dummy address, never dereferenced
BF16, F32 = 1, 0


@pytest.mark.parametrize("slot_bytes", [384, 448])
def test_round_trip(slot_bytes):
    cap = P.capacity(slot_bytes)
    assert cap == {384: 176, 448: 208}[slot_bytes]
    rows = P.crafted_rows(slot_bytes, 64, seed=1)
    slots, over = P.encode(rows, slot_bytes)
    assert over == 0 and slots.shape == (64, slot_bytes)
    assert np.array_equal(P.decode(slots), rows)
    nz = (rows != 0).sum(1)
    assert np.array_equal(P.counts(slots), nz)
    assert nz[0] == 0 and nz[1] == 1 and nz[2] == cap and nz[4] == cap and nz[5] == cap - 1
    assert slots[1, 31] == 0x80 and slots[1, :31].sum() == 0 and slots[1, 32:34].view(np.uint16)[0] == 0x4000
    assert (rows[3, ::7] == 0x8000).all() and (P.decode(slots)[3, ::7] == 0x8000).all()      # -0.0 survives
    for i in range(64):                                                                       # zero behind the last value
        assert not slots[i, 32 + 2 * nz[i]:].any()


@pytest.mark.parametrize("slot_bytes", [384, 448])
def test_overflow_rows_are_counted_and_truncated(slot_bytes):
    cap = P.capacity(slot_bytes)
    rows = P.crafted_rows(slot_bytes, 16, seed=2, overflow_row=True)
    slots, over = P.encode(rows, slot_bytes)
    assert over == 1 and P.counts(slots)[5] == 256
    assert np.array_equal(slots[5, 32:].view(np.uint16), rows[5, :cap])
    dec = P.decode(slots)
    assert (dec[5] == 0xFFFF).all()
    keep = np.arange(16) != 5
    assert np.array_equal(dec[keep], rows[keep])


def test_entries_are_declared_bound_and_exported():
    from sgformer_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgf.h")).read(), flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m is not None, f"{name} not declared in include/sgf.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
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


def test_packed_bytes(lib):
    assert lib.sgf_spmm_packed_bytes(0, 384) == 128
    assert lib.sgf_spmm_packed_bytes(1000, 384) == 1000 * 384 + 128
    assert lib.sgf_spmm_packed_bytes(2449029, 448) == 2449029 * 448 + 128


def test_supported_follows_the_launch_rule(lib, monkeypatch):
    n = 2449029
    ok = lambda **kw: lib.sgf_spmm_packed_supported(*[{**dict(d=256, dtype=BF16, ldx=256, ldy=256, n_cols=n, aligned16=1,
                                                             slot_bytes=384), **kw}[k]
                                                      for k in ("d", "dtype", "ldx", "ldy", "n_cols", "aligned16", "slot_bytes")])
    assert lib.sgf_spmm_arm(256, BF16, 256, 256, n, 1, 0) == 2          # the wave-per-row kernel
    assert ok() == 1 and ok(slot_bytes=448) == 1
    assert ok(slot_bytes=512) == 0 and ok(slot_bytes=320) == 0
    assert ok(dtype=F32) == 0 and ok(d=128) == 0 and ok(d=512) == 0
    assert ok(n_cols=12000000) == 0                                     # slots beyond 32-bit offsets (and x beyond them too)
    monkeypatch.setenv("SGF_SPMM_PACKED", "0")
    lib.sgf_reload_env()
    try:
        assert ok() == 0
    finally:
        monkeypatch.delenv("SGF_SPMM_PACKED")
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
    def bn(**kw):
        a = {**dict(x=A, ldx=256, res=None, ldr=0, n=10, d=256, dtype=BF16, y=A, ldy=256, packed=A, slot=384, over=A), **kw}
        return lib.sgf_bn_apply_packed(a["x"], a["ldx"], A, A, None, None, a["res"], a["ldr"], 1, a["n"], a["d"], a["dtype"],
                                       a["y"], a["ldy"], a["packed"], a["slot"], a["over"], None)
    for kw in (dict(packed=None), dict(over=None), dict(d=128), dict(dtype=F32), dict(slot=512), dict(packed=A + 64),
               dict(x=A + 8), dict(ldx=260)):
        assert bn(**kw) < 0, kw
        assert lib.sgf_last_error().startswith(b"sgf_bn_apply_packed:"), lib.sgf_last_error()

    def mm(**kw):
        a = {**dict(packed=A, slot=384, over=A, d=256, long_len=1024, segs=0), **kw}
        return lib.sgf_spmm_packed(A, A, A, A, 256, 10, a["packed"], a["slot"], a["over"], A, 256, 10, a["d"], BF16,
                                   a["long_len"], a["segs"], None, 0, None)
    for kw in (dict(packed=None), dict(over=None), dict(slot=400), dict(packed=A + 16), dict(d=6), dict(long_len=0),
               dict(segs=3)):
        assert mm(**kw) < 0, kw
        assert lib.sgf_last_error().startswith(b"sgf_spmm_packed:"), lib.sgf_last_error()
