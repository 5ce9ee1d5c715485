"""SGF_F32_BF16X3 on the attention from the un-projected input (sgf_attn_h_fwd / _bwd_reduce / _bwd_apply, csrc/attn_f32x.hip):
the host query in the header, the binding and the library, kernels.py's choice of code for these entries, and a numpy
restatement of the three passes on the split / x3_matmul model of tests/test_f32_precision.py, held against fp64 to the
bounds tests/test_gpu_attn_f32x.py puts on the kernels.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

from tests.test_f32_precision import BOUND, x3_matmul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACC = 5e-6


def test_header_binding_and_library_export_the_query():
    from sgformer_amd import _lib
    header = open(os.path.join(ROOT, "include", "sgf.h")).read()
    assert re.search(r"int32_t\s+sgf_attn_h_supported\(int32_t d, int32_t dtype\);", header)
    assert "sgf_attn_h_supported" in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.sgf_attn_h_supported(64, _lib.SGF_F32) == 1


@pytest.mark.parametrize("d", [64, 128, 256])
def test_host_queries(d):
    from sgformer_amd import _lib
    lib = _lib.load()
    x3 = _lib.SGF_F32_BF16X3
    assert lib.sgf_attn_h_supported(d, x3) == 1
    assert lib.sgf_attn_h_supported(d, _lib.SGF_F32) == 1 and lib.sgf_attn_h_supported(d, _lib.SGF_BF16) == 1
    # the three-call bf16 backward keeps refusing the code
    assert lib.sgf_attn_h_bwd_split_supported(d, x3) == 0
    # fp32 storage needs no scratch for the apply under either code
    assert lib.sgf_attn_h_bwd_apply_workspace_bytes(1000, d, x3) == 0


def test_host_query_follows_the_exact_entries_shapes():
    from sgformer_amd import _lib
    lib = _lib.load()
    for code in (_lib.SGF_F32, _lib.SGF_F32_BF16X3):
        assert [lib.sgf_attn_h_supported(d, code) for d in (4, 48, 60, 100)] == [1, 1, 1, 1]
        assert [lib.sgf_attn_h_supported(d, code) for d in (0, 62, 258, 260)] == [0, 0, 0, 0]
    assert lib.sgf_attn_h_supported(64, 7) == 0


@pytest.fixture
def restore_precision():
    yield
    torch.set_float32_matmul_precision("highest")


def test_kernels_chooses_the_code_for_the_attention(restore_precision):
    from sgformer_amd import _lib, kernels
    a32 = torch.zeros(4, 256)
    a16 = torch.zeros(4, 256, dtype=torch.bfloat16)
    for prec, want in (("highest", _lib.SGF_F32), ("high", _lib.SGF_F32_BF16X3), ("medium", _lib.SGF_F32_BF16X3)):
        torch.set_float32_matmul_precision(prec)
        assert kernels._mm_code(a32, "sgf_attn_h_supported", 256) == want
        assert kernels._mm_code(a16, "sgf_attn_h_supported", 256) == _lib.SGF_BF16
    torch.set_float32_matmul_precision("high")
    # a width the entries do not take keeps SGF_F32 (and is then refused exactly as under 'highest')
    assert kernels._mm_code(a32, "sgf_attn_h_supported", 258) == _lib.SGF_F32


def test_kernels_hands_the_entries_the_chosen_code():
    import inspect
    from sgformer_amd import kernels
    for fn in (kernels.HipKernels.attn_h_fwd, kernels.HipKernels.attn_h_bwd_reduce, kernels.HipKernels.attn_h_bwd_apply):
        assert '_mm_code(h, "sgf_attn_h_supported", d)' in inspect.getsource(fn), fn.__name__


# ---- the three passes on the split model: only the matrix products are split, everything else is fp64 here ----------------
def _inputs(n, d, seed, kind):
    rng = np.random.default_rng(seed)
    if kind == "random":
        h = rng.standard_normal((n, d))
        g = rng.standard_normal((n, d))
        M = rng.standard_normal((d, d)) / d ** 0.5
        D = rng.standard_normal((d, d)) / d ** 0.5
    else:   # 1 + 2^-9 + 2^-17 with random signs: hi drops 2^-9 at the tie, lo holds only part of the rest
        v = 1 + 2.0 ** -9 + 2.0 ** -17
        h = v * rng.choice([-1.0, 1.0], (n, d))
        g = v * rng.choice([-1.0, 1.0], (n, d))
        M = v * rng.choice([-1.0, 1.0], (d, d)) / d
        D = (1 - 2.0 ** -9 - 2.0 ** -18) * rng.choice([-1.0, 1.0], (d, d)) / d
    f32 = lambda a: a.astype(np.float32)
    w = f32(0.5 * rng.uniform(0, 1, d) / d)
    return f32(h), f32(g), f32(M), f32(D), f32(rng.standard_normal(d)), w, f32(rng.standard_normal(d))


@pytest.mark.parametrize("kind", ["random", "adversarial"])
@pytest.mark.parametrize("n,d", [(300, 64), (131, 256), (64, 48)])
def test_three_passes_on_the_split_model_stay_inside_the_bounds(n, d, kind):
    h, g, M, D, m, w, ds = _inputs(n, d, n + d, kind)
    f64 = lambda a: a.astype(np.float64)
    h64, g64, M64, D64 = f64(h), f64(g), f64(M), f64(D)
    den = (h64 @ f64(w) + 3.0).reshape(-1, 1)
    assert np.all(np.abs(den - 3.0) < 1.0)

    def inside(got, ref, p):
        return np.all(np.abs(got - ref) <= BOUND * p + ACC * np.abs(ref).max())

    # forward: out = (h M + m) / den
    out64 = (h64 @ M64 + f64(m)) / den
    out = (x3_matmul(h, M) + f64(m)) / den
    assert inside(out, out64, (np.abs(h64) @ np.abs(M64)) / np.abs(den))
    # backward from (g, out, den): dnum is formed in fp32 and THEN split, as the kernels do
    o32 = out64.astype(np.float32)
    den32 = den.astype(np.float32)
    dnum32 = (g / den32).astype(np.float32)
    dnum64 = g64 / f64(den32)
    dden64 = -(g64 * f64(o32)).sum(1, keepdims=True) / f64(den32)
    dh64 = dnum64 @ M64.T + dden64 * f64(w) + h64 @ D64 + f64(ds)
    dh = x3_matmul(dnum32, np.ascontiguousarray(M.T)) + dden64 * f64(w) + x3_matmul(h, D) + f64(ds)
    assert inside(dh, dh64, np.abs(dnum64) @ np.abs(M64).T + np.abs(h64) @ np.abs(D64))
    # reduce: the d x d block of hstats
    dM = x3_matmul(np.ascontiguousarray(h.T), dnum32)
    assert inside(dM, h64.T @ dnum64, np.abs(h64).T @ np.abs(dnum64))
