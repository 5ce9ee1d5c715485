"""torch.set_float32_matmul_precision('high' / 'medium') on the fp32 path: the split-bf16 error model (numpy restatement),
the SGF_F32_BF16X3 code in the header, the binding and the library's host queries, kernels.py's choice of code and the
launcher's --sgf-f32-matmul option.  No GPU needed (tests/test_gpu_f32_precision.py runs the kernels)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Error model: |a - hi| <= 2^-8 |a|, |a - hi - lo| <= 2^-16 |a|; the three dropped terms bound each product's
# error by 3 * 2^-16 |a b|.  Test bound per element: 2^-14 (|A|^T |B|)_ij plus an fp32 accumulation allowance.
BOUND = 2.0 ** -14


def bf16_rne(a):
    """fp32 -> bf16 (as fp32 values) by bit arithmetic: round to nearest even, NaN kept (a quiet NaN)."""
    a = np.asarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    nan = np.isnan(a)
    r = np.where(nan, (u | 0x400000) & 0xFFFF0000, r)
    return r.astype(np.uint32).view(np.float32)


def split(a):
    a = np.asarray(a, dtype=np.float32)
    hi = bf16_rne(a)
    with np.errstate(invalid="ignore"):
        rest = np.where(np.isfinite(hi), a - hi, np.float32(0.0)).astype(np.float32)
    return hi, bf16_rne(rest)


def x3_matmul(a, b):
    """C = A B as three bf16 products, summed in fp64 (the model of the kernels without their fp32 accumulation)."""
    ah, al = (v.astype(np.float64) for v in split(a))
    bh, bl = (v.astype(np.float64) for v in split(b))
    return ah @ bh + ah @ bl + al @ bh


def test_split_is_exact_where_it_claims():
    rng = np.random.default_rng(0)
    a = (rng.standard_normal(100000) * np.exp(rng.uniform(-30, 30, 100000))).astype(np.float32)
    hi, lo = split(a)
    assert np.all((hi.view(np.uint32) & 0xFFFF) == 0) and np.all((lo.view(np.uint32) & 0xFFFF) == 0)
    a64 = a.astype(np.float64)
    assert np.all(np.abs(a64 - hi) <= 2.0 ** -8 * np.abs(a64))
    assert np.all(np.abs(a64 - hi - lo) <= 2.0 ** -16 * np.abs(a64))


@pytest.mark.parametrize("kind", ["random", "adversarial", "mixed"])
def test_three_product_bound_against_fp64(kind):
    rng = np.random.default_rng({"random": 1, "adversarial": 2, "mixed": 3}[kind])
    n, k, m = 64, 300, 48
    if kind == "random":
        a = rng.standard_normal((n, k)).astype(np.float32)
        b = rng.standard_normal((k, m)).astype(np.float32)
    elif kind == "adversarial":
        # 1 + 2^-9 + 2^-17: hi drops 2^-9 exactly at the tie, lo can hold only part of the rest
        v = np.float32(1 + 2.0 ** -9 + 2.0 ** -17)
        a = np.full((n, k), v, dtype=np.float32) * rng.choice([-1, 1], (n, k)).astype(np.float32)
        b = np.full((k, m), v, dtype=np.float32)
        b[::3] = np.float32(1 - 2.0 ** -9 - 2.0 ** -18)
    else:
        a = (rng.standard_normal((n, k)) * np.exp(rng.uniform(-20, 20, (n, k)))).astype(np.float32)
        b = (rng.standard_normal((k, m)) * np.exp(rng.uniform(-20, 20, (k, m)))).astype(np.float32)
    ref = a.astype(np.float64) @ b.astype(np.float64)
    p = np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64))
    err = np.abs(x3_matmul(a, b) - ref)
    assert np.all(err <= BOUND * p)


def test_non_finite_inputs_stay_non_finite():
    a = np.array([[np.inf, 1.0], [-np.inf, 2.0], [np.nan, 3.0], [1.5, 2.5]], dtype=np.float32)
    b = np.array([[1.25, -3.0], [0.5, 2.0]], dtype=np.float32)
    hi, lo = split(a)
    assert np.isposinf(hi[0, 0]) and lo[0, 0] == 0 and np.isneginf(hi[1, 0]) and lo[1, 0] == 0
    assert np.isnan(hi[2, 0]) and lo[2, 0] == 0
    with np.errstate(invalid="ignore"):
        ref = a.astype(np.float64) @ b.astype(np.float64)
        got = x3_matmul(a, b)
    assert np.array_equal(np.isfinite(got), np.isfinite(ref))
    assert np.all(np.isnan(got[2]))


def test_header_and_binding_define_the_code():
    from sgformer_amd import _lib
    header = open(os.path.join(ROOT, "include", "sgf.h")).read()
    assert int(re.search(r"#define\s+SGF_F32_BF16X3\s+(\d+)", header).group(1)) == 2
    assert _lib.SGF_F32_BF16X3 == 2 and len({_lib.SGF_F32, _lib.SGF_BF16, _lib.SGF_F32_BF16X3}) == 3


@pytest.mark.parametrize("d", [64, 128, 256])
def test_host_queries_accept_the_code(d):
    from sgformer_amd import _lib
    lib = _lib.load()
    x3 = _lib.SGF_F32_BF16X3
    assert lib.sgf_combine_fc_supported(d, 48, x3) == 1 and lib.sgf_combine_fc_supported(d, d, x3) == 1
    assert lib.sgf_gcn_epilogue_supported(d, d, x3) == 1 and lib.sgf_gcn_epilogue_supported(d, 60, x3) == 1
    # the entries that run no fp32 Linear keep refusing the code
    assert lib.sgf_gcn_epilogue_cat_supported(d, x3) == 0 and lib.sgf_gcn_epilogue_dx2_acc_supported(d, x3) == 0
    assert lib.sgf_gram_bn_bwd_supported(d, d, x3) == 0
    # outside the fp32 shapes, refused as SGF_F32 is
    assert lib.sgf_gcn_epilogue_supported(d, 258, x3) == lib.sgf_gcn_epilogue_supported(d, 258, _lib.SGF_F32) == 0


@pytest.fixture
def restore_precision():
    yield
    torch.set_float32_matmul_precision("highest")


def test_kernels_maps_the_torch_setting(restore_precision):
    from sgformer_amd import _lib, kernels
    a32 = torch.zeros(4, 4)
    a16 = torch.zeros(4, 4, dtype=torch.bfloat16)
    for prec, want in (("highest", _lib.SGF_F32), ("high", _lib.SGF_F32_BF16X3), ("medium", _lib.SGF_F32_BF16X3)):
        torch.set_float32_matmul_precision(prec)
        assert kernels.f32_matmul_code() == want
        assert kernels._mm_code(a32) == want
        assert kernels._mm_code(a32, "sgf_gcn_epilogue_supported", 64, 64) == want
        assert kernels._mm_code(a16) == _lib.SGF_BF16               # bf16 storage is not affected
    torch.set_float32_matmul_precision("high")
    # a shape the entry does not take keeps SGF_F32 (the entry then refuses it as before)
    assert kernels._mm_code(a32, "sgf_gcn_epilogue_supported", 64, 1000) == _lib.SGF_F32


def test_tf32_switches_select_high(restore_precision):
    from sgformer_amd import _lib, kernels
    torch.backends.cuda.matmul.allow_tf32 = True
    try:
        assert torch.get_float32_matmul_precision() == "high" and kernels.f32_matmul_code() == _lib.SGF_F32_BF16X3
    finally:
        torch.backends.cuda.matmul.allow_tf32 = False
    assert kernels.f32_matmul_code() == _lib.SGF_F32


def test_launcher_option(restore_precision):
    from sgformer_amd import launch
    argv = ["trainer.py", "--sgf-f32-matmul", "high", "--lr", "0.01"]
    assert launch.apply_f32_matmul(argv) == "high"
    assert argv == ["trainer.py", "--lr", "0.01"] and torch.get_float32_matmul_precision() == "high"
    argv = ["trainer.py", "--sgf-f32-matmul=medium"]
    assert launch.apply_f32_matmul(argv) == "medium" and argv == ["trainer.py"]
    assert torch.get_float32_matmul_precision() == "medium"
    argv = ["trainer.py", "--epochs", "3"]
    torch.set_float32_matmul_precision("highest")
    assert launch.apply_f32_matmul(argv) is None and torch.get_float32_matmul_precision() == "highest"
    with pytest.raises(SystemExit, match="sgf-f32-matmul"):
        launch.apply_f32_matmul(["trainer.py", "--sgf-f32-matmul", "tf32"])
    # main() applies it before anything else (here: before it finds no trainer)
    with pytest.raises(SystemExit):
        launch.main(["--sgf-f32-matmul", "high"])
    assert torch.get_float32_matmul_precision() == "high"
