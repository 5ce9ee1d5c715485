"""sgf_dropout_dev (include/sgf.h): sgf_dropout with its 64-bit Philox seed read from device memory when the kernel runs —
bit-identical to the immediate-seed kernel for the same seed value, through autograd inside a seed scope, and as ONE
captured launch that draws a new mask whenever its slot has been rewritten."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SEEDS = (5, 2 ** 32 + 5, 2 ** 62 - 1)          # the last two differ from the first only above bit 31: a 32-bit read shows
PS = (0.0, 0.2, 0.5, 1.0)


def _operands(cuda, shape, dtype, with_res):
    """x (and res) of `shape`; (130, 172) as column slices of wider tensors, so that ld > d (and ldx != ldr)."""
    n, d = shape
    g = torch.Generator().manual_seed(n * 1000 + d)
    if shape == (130, 172):
        x = (torch.rand(n, 180, generator=g) + 0.5).to(dtype).to(cuda)[:, 4:176]
        res = (torch.rand(n, 176, generator=g) * 2 - 1).to(dtype).to(cuda)[:, :172]
        assert x.stride(0) == 180 and res.stride(0) == 176
    else:
        x = (torch.rand(n, d, generator=g) + 0.5).to(dtype).to(cuda)
        res = (torch.rand(n, d, generator=g) * 2 - 1).to(dtype).to(cuda)
    return x, (res if with_res else None)


@pytest.mark.parametrize("shape", [(1, 4), (3, 8), (257, 64), (130, 172)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_equals_the_immediate_seed_kernel(cuda, dtype, with_res, shape):
    """Every p, seed and slot of a bank of 4: torch.equal with K.dropout under the same seed value.  (257, 64): n d / 4 is no
    multiple of the block; seeds beyond 2^32 catch a 32-bit read of the slot, slot 3 a wrong pointer offset (the other
    slots hold other seeds)."""
    from sgformer_amd import ops
    K = ops.K
    x, res = _operands(cuda, shape, dtype, with_res)
    for seed in SEEDS:
        for slot in (0, 3):
            host = [seed ^ 0x5A5A5A5A5A5A5A + j for j in range(4)]
            host[slot] = seed
            seeds = torch.tensor(host, dtype=torch.int64, device=cuda)
            assert int(seeds[slot]) == seed
            for p in PS:
                got = K.dropout_dev(x, res, p, seeds, slot)
                want = K.dropout(x, res, p, int(seeds[slot]))
                assert torch.equal(got, want), (seed, slot, p)
    if shape[0] * shape[1] >= 64:                # the seed matters at all, also above bit 31 (enough elements to tell)
        a = K.dropout_dev(x, None, 0.5, torch.tensor([SEEDS[0]], dtype=torch.int64, device=cuda), 0)
        b = K.dropout_dev(x, None, 0.5, torch.tensor([SEEDS[1]], dtype=torch.int64, device=cuda), 0)
        assert not torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_through_autograd_inside_a_seed_scope(cuda, dtype):
    """ops.dropout_res inside an active seed scope: no generator draw, the backward's non-zero pattern is the forward's keep
    pattern element for element (as tests/test_gpu_kernels.py::test_fused_dropout checks for the eager kernel), the
    residual's gradient is the incoming one, and the result is K.dropout's under the slot's seed."""
    from sgformer_amd import kernels, ops
    n, d, p = 257, 64, 0.5
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(n, d, generator=g) + 0.5).to(dtype)
    res = (torch.rand(n, d, generator=g) * 2 - 1).to(dtype)
    w = (torch.rand(n, d, generator=g) + 0.5).to(dtype).to(cuda)
    xg, rg = x.to(cuda).requires_grad_(True), res.to(cuda).requires_grad_(True)
    bank = kernels.SeedBank(cuda, 4)
    bank.seeds.copy_(torch.tensor([11, 2 ** 40 + 3, 13, 14]))
    torch.manual_seed(7)
    state = torch.random.get_rng_state()
    kernels.begin_seed_scope(bank)
    try:
        y0 = ops.dropout_res(xg.detach(), None, p)               # slot 0
        y = ops.dropout_res(xg, rg, p)                           # slot 1
    finally:
        kernels.end_seed_scope()
    assert bank.used == 2 and torch.equal(torch.random.get_rng_state(), state)
    assert torch.equal(y0, ops.K.dropout(xg.detach(), None, p, 11))
    assert torch.equal(y.detach(), ops.K.dropout(xg.detach(), rg.detach(), p, 2 ** 40 + 3))
    y.backward(w)
    keep = y.detach() != rg.detach()
    assert 0.4 < float(keep.float().mean()) < 0.6
    assert torch.equal(xg.grad != 0, keep)                       # same pattern, element for element
    assert torch.equal(xg.grad, ops.K.dropout(w, None, p, 2 ** 40 + 3))
    assert torch.equal(rg.grad, w)


def test_one_captured_launch_follows_its_slot(cuda):
    """A single launch captured with torch.cuda.graph: after each rewrite of the slot the replay equals K.dropout with that
    seed and differs from the previous replay; rewriting the same seed gives the same output again."""
    from sgformer_amd import ops
    K = ops.K
    x, res = _operands(cuda, (257, 64), torch.bfloat16, True)
    seeds = torch.tensor([1, 2, 3, 4], dtype=torch.int64, device=cuda)
    K.dropout_dev(x, res, 0.5, seeds, 2)                         # (the code object is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = K.dropout_dev(x, res, 0.5, seeds, 2)
    prev = None
    for seed in (7, 2 ** 32 + 7, 2 ** 62 - 1, 2 ** 62 - 1):
        seeds[2] = seed
        graph.replay()
        out = y.clone()
        assert torch.equal(out, K.dropout(x, res, 0.5, seed)), seed
        if prev is not None:
            assert torch.equal(out, prev[1]) == (seed == prev[0])
        prev = (seed, out)
    torch.cuda.synchronize()
    del graph


def test_bad_seed_slots_are_rejected_on_the_host(cuda):
    """A null or misaligned seed_slot with n > 0 is SGF_E_INVALID (-1) before any launch; n == 0 returns SGF_OK without
    reading the slot (a null one is accepted)."""
    from sgformer_amd import _lib
    lib = _lib.load()
    x = torch.ones(8, 8, device=cuda)
    y = torch.full((8, 8), -1.0, device=cuda)
    seeds = torch.tensor([5, 6], dtype=torch.int64, device=cuda)
    P = ctypes.c_void_p

    def call(slot, n):
        return lib.sgf_dropout_dev(P(x.data_ptr()), 8, None, 0, 0.5, slot, n, 8, _lib.SGF_F32, P(y.data_ptr()), 8, None)

    assert call(None, 8) == -1 and b"sgf_dropout_dev" in lib.sgf_last_error()
    assert call(P(seeds.data_ptr() + 4), 8) == -1 and b"sgf_dropout_dev" in lib.sgf_last_error()
    assert call(None, 0) == 0
    torch.cuda.synchronize()
    assert bool((y == -1.0).all())                               # nothing was launched by any of the three
    assert call(P(seeds.data_ptr() + 8), 8) == 0
    torch.cuda.synchronize()
    assert torch.equal(y, __import__("sgformer_amd").ops.K.dropout(x, None, 0.5, 6))
