"""sgf_sampled_csr_* (csrc/sampled_csr.hip) on the host: the C ABI, the argument checks that run before any HIP call, and the
CONTRACT restated without a global sort.

A neighbour-sampled batch (sgf_neighbor_sample_batch, oracle/graph_oracle.py::neighbor_sample) emits its edges hop after hop,
in frontier order inside a hop, and every node is a frontier node exactly once.  Hence the two preconditions of
sgf_sampled_csr_build — targets non-decreasing, no row longer than max(fanouts) — and the three sort-free pieces the kernels
are made of, restated here in numpy and checked bit for bit against the oracle's csr_build / csr_transpose (which argsort
the whole edge list, like 100M/ours.py:72-79):
  * rowptr = lower bound into the target array,
  * a sort of at most max(fanouts) sources inside each row,
  * the transpose as a STABLE counting sort of the forward entries by source.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import graph_oracle as G
from oracle import sgformer_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"sgf_sampled_csr_supported": 1, "sgf_sampled_csr_build_workspace_bytes": 2, "sgf_sampled_csr_build": 13,
         "sgf_sampled_csr_transpose_workspace_bytes": 2, "sgf_sampled_csr_transpose": 11}
FANOUTS = [[15, 10, 5], [3, 2], [32], [40, 3], [0, 5], [5, 0, 3]]


# ------------------------------------------------------------------------------------------------
# C ABI
# ------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "sgf.h")).read()


def test_abi_header_binding_and_library_agree():
    from sgformer_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, nargs in NAMES.items():
        m = re.search(r"\b(?:int|int32_t|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m is not None, f"{name} not declared in include/sgf.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs, name
        assert name in _lib.SIGNATURES, f"{name} not bound in _lib.SIGNATURES"
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert int(re.search(r"#define\s+SGF_VERSION\s+(\d+)", _header()).group(1)) >= 650
    # the header names the reference lines each entry replaces
    block = _header().split("sgf_sampled_csr_build (", 1)[1]
    assert "100M/ours.py:72-79" in block and "large/ours.py:26-33" in block and "large/ours.py:34" in block
    assert _lib.available(), "libsgf.so not built (run `make`)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} not exported by libsgf.so"
    lib.sgf_version.restype = ctypes.c_int
    assert lib.sgf_version() >= 650


def test_arguments_are_checked_before_any_hip_call():
    from sgformer_amd import _lib
    lib = _lib.load()
    for k in range(0, 65):
        assert lib.sgf_sampled_csr_supported(k) == 1, k
    for k in (-1, -7, -2 ** 31):
        assert lib.sgf_sampled_csr_supported(k) == 0, k
    one = ctypes.c_void_p(256)          # a non-null address: never dereferenced, every call below fails its checks first
    E_INVALID = -1
    build = lib.sgf_sampled_csr_build
    bad_build = [
        (one, one, one, -1, 8, 4, one, one, one, one, None, 0, None),        # negative node capacity
        (one, one, one, 8, -1, 4, one, one, one, one, None, 0, None),        # negative edge capacity
        (one, one, one, 8, 8, -3, one, one, one, one, None, 0, None),        # negative fan-out
        (one, one, one, 8, 8, 4, None, one, one, one, None, 0, None),        # null rowptr_b
        (one, one, one, 8, 8, 4, one, None, one, one, None, 0, None),        # null colind_b
        (one, one, one, 8, 8, 4, one, one, None, one, None, 0, None),        # null val_b
        (one, one, one, 8, 8, 4, one, one, one, None, None, 0, None),        # null deg_b
        (one, one, None, 8, 8, 4, one, one, one, one, None, 0, None),        # null counts
        (None, one, one, 8, 8, 4, one, one, one, one, None, 0, None),        # null edge list
    ]
    for args in bad_build:
        assert build(*args) == E_INVALID, args
        assert b"sgf_sampled_csr_build" in lib.sgf_last_error()
    # a fan-out the kernels do not take is UNSUPPORTED (the caller keeps sgf_csr_build), not a launch
    big = 1 << 20
    assert lib.sgf_sampled_csr_supported(big) == 0
    assert build(one, one, one, 8, 8, big, one, one, one, one, None, 0, None) == -4
    assert b"sgf_sampled_csr_build" in lib.sgf_last_error()
    tr = lib.sgf_sampled_csr_transpose
    bad_tr = [
        (one, one, one, -1, 8, one, one, one, one, 1 << 20, None),           # negative n
        (one, one, one, 8, -1, one, one, one, one, 1 << 20, None),           # negative nnz
        (None, one, one, 8, 8, one, one, one, one, 1 << 20, None),           # null rowptr
        (one, one, one, 8, 8, None, one, one, one, 1 << 20, None),           # null t_rowptr
        (one, one, one, 8, 8, one, None, one, one, 1 << 20, None),           # null t_colind
        (one, one, one, 8, 8, one, one, None, one, 1 << 20, None),           # null t_val
        (one, None, one, 8, 8, one, one, one, one, 1 << 20, None),           # null colind
    ]
    for args in bad_tr:
        assert tr(*args) == E_INVALID, args
        assert b"sgf_sampled_csr_transpose" in lib.sgf_last_error()
    # a workspace that cannot hold the entry arrays: SGF_E_WORKSPACE, also decided on the host
    for ws, nbytes in ((None, 1 << 20), (one, 0), (one, 63)):
        assert tr(one, one, one, 8, 8, one, one, one, ws, nbytes, None) == -2, (ws, nbytes)
        assert b"sgf_sampled_csr_transpose" in lib.sgf_last_error()
    assert lib.sgf_sampled_csr_transpose_workspace_bytes(-1, 8) == 0 and lib.sgf_sampled_csr_transpose_workspace_bytes(8, -1) == 0


# ------------------------------------------------------------------------------------------------
# the contract, restated without a sort of the edge list
# ------------------------------------------------------------------------------------------------
def ref_build(src, dst, nn, max_fanout):
    """(rowptr, colind, val, deg) of a sampled batch's edge list: lower-bound rowptr, per-row source sort, fp32 values."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    assert np.all(np.diff(dst) >= 0), "precondition: targets non-decreasing"
    rowptr = np.searchsorted(dst, np.arange(nn + 1), side="left").astype(np.int64)       # lower bound; rowptr[nn] = ne
    deg = np.diff(rowptr)
    assert deg.size == 0 or int(deg.max()) <= max_fanout, "precondition: no row longer than max(fanouts)"
    colind = np.empty_like(src)
    for j in np.nonzero(deg)[0]:
        b, e = rowptr[j], rowptr[j + 1]
        colind[b:e] = np.sort(src[b:e], kind="stable")          # at most max_fanout sources
    d32 = deg.astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.sqrt(np.float32(1.0) / d32[np.repeat(np.arange(nn), deg)])
        b = np.sqrt(np.float32(1.0) / d32[colind])
        val = (a * b).astype(np.float32)
    val[~np.isfinite(val)] = np.float32(0.0)
    return rowptr, colind, val, deg.astype(np.int64)


def ref_transpose(rowptr, colind, val):
    """(t_rowptr, t_colind, t_val): a stable counting sort of the forward entries by source."""
    n, nnz = rowptr.size - 1, colind.size
    t_rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(colind, minlength=n), out=t_rowptr[1:])
    nxt = t_rowptr[:-1].copy()
    t_colind, t_val = np.empty(nnz, dtype=np.int64), np.empty(nnz, dtype=np.float32)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    for i in range(nnz):                                        # forward order = target order: placement is stable
        q = nxt[colind[i]]
        nxt[colind[i]] += 1
        t_colind[q], t_val[q] = row[i], val[i]
    return t_rowptr, t_colind, t_val


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def parent():
    from sgformer_amd import synth
    n = 4000
    ei = synth.synthetic_graph_skewed(n, 14.0, gamma=2.5).numpy()
    rowptr, colind, _, _ = O.csr_build(ei, n)
    return n, rowptr, colind


@pytest.mark.parametrize("fanouts", FANOUTS)
def test_sort_free_restatement_equals_the_oracle_on_sampled_batches(parent, fanouts):
    """Three batches per fan-out list.  At least one of them must hold an entry with val == 0 AND one with val != 0, so that
    the zero rule is exercised and is not the only thing exercised.  A list that begins with fan-out 0 ([0, 5]) cannot: hop 0
    samples nothing, the frontier ends there and the batch has NO entry at all (oracle/graph_oracle.py::neighbor_sample,
    csrc/sampler.hip) — for such a list the test asserts exactly that (every batch edgeless, CSR of nn empty rows) instead."""
    n, rowptr, colind = parent
    g = torch.Generator().manual_seed(5)
    zero_and_nonzero, entries = False, 0
    for b in range(3):
        seeds = torch.randperm(n, generator=g)[:200].numpy()
        n_id, src, dst = G.neighbor_sample(rowptr, colind, seeds, fanouts, 1234, b)
        nn = len(n_id)
        src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
        # the two preconditions, from the sampler's own output
        assert np.all(np.diff(dst) >= 0)
        assert (np.bincount(dst, minlength=nn).max() if dst.size else 0) <= max(fanouts)
        ei = np.stack([src, dst])
        rp, ci, va, dg = ref_build(src, dst, nn, max(fanouts))
        o_rp, o_ci, o_va, o_dg = O.csr_build(ei, nn)
        assert np.array_equal(rp, o_rp) and np.array_equal(ci, o_ci) and np.array_equal(dg, o_dg)
        assert np.array_equal(_bits(va), _bits(o_va))
        t_rp, t_ci, t_va = ref_transpose(rp, ci, va)
        ot_rp, ot_ci, ot_va, _ = O.csr_transpose(ei, nn)
        assert np.array_equal(t_rp, ot_rp) and np.array_equal(t_ci, ot_ci) and np.array_equal(_bits(t_va), _bits(ot_va))
        # sources that entered in the last hop have in-degree 0: 1 / 0 -> inf -> 0 (nan_to_num, 100M/ours.py:78)
        if va.size:
            assert np.array_equal(va == 0, dg[ci] == 0)
            zero_and_nonzero |= bool((va == 0).any() and (va != 0).any())
        entries += int(va.size)
        if fanouts[0] == 0:
            assert va.size == 0 and nn == 200 and not rp.any() and not t_rp.any()
    if fanouts[0] == 0:
        assert entries == 0
    else:
        assert zero_and_nonzero, "no batch exercised both the zero-value rule and an ordinary value"


def test_restatement_keeps_duplicates_and_long_transposed_rows():
    """Duplicate stored edges stay (large/ours.py:33 does not coalesce), and a transposed row is as long as it comes."""
    src = np.array([3, 3, 1, 2, 2, 2, 0], dtype=np.int64)
    dst = np.array([0, 0, 0, 1, 1, 1, 2], dtype=np.int64)
    rp, ci, va, dg = ref_build(src, dst, 4, 3)
    o = O.csr_build(np.stack([src, dst]), 4)
    assert np.array_equal(rp, o[0]) and np.array_equal(ci, o[1]) and np.array_equal(_bits(va), _bits(o[2]))
    t = ref_transpose(rp, ci, va)
    ot = O.csr_transpose(np.stack([src, dst]), 4)
    assert all(np.array_equal(a, b) for a, b in zip(t[:2], ot[:2])) and np.array_equal(_bits(t[2]), _bits(ot[2]))
    # a star: 5000 targets with the one source 5000
    m = 5000
    src, dst = np.full(m, m, dtype=np.int64), np.arange(m, dtype=np.int64)
    rp, ci, va, dg = ref_build(src, dst, m + 1, 1)
    t_rp, t_ci, t_va = ref_transpose(rp, ci, va)
    ot = O.csr_transpose(np.stack([src, dst]), m + 1)
    assert t_rp[m + 1] - t_rp[m] == m and np.array_equal(t_rp, ot[0]) and np.array_equal(t_ci, ot[1])
    assert np.array_equal(_bits(t_va), _bits(ot[2])) and not t_va.any()      # the hub has no in-edge: every value is 0
