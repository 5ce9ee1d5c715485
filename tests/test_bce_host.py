"""The multi-label loss (BCEWithLogitsLoss on the training rows; include/sgf.h block N4b) above the C ABI, on the CPU:
ops.bce_loss_rows / loss.bce_with_logits_rows, dist.sharded_bce_loss under gloo, and launch.patch_bce_loss driven by callers
that are not the reference's trainers.  The CPU kernel table of tests/cpu_kernels_bce.py stands in for libsgf; the reference
is torch.nn.functional.binary_cross_entropy_with_logits in float64 on the same stored logits.  Bounds: those of the GPU
kernel test (tests/test_gpu_bce.py), taken from the project's NLL tests."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _no_leftover_patch():
    """Other test files run sgformer_amd.launch.main in `all` mode and restore only the patches they know about: start (and
    leave) every test here with the original F.binary_cross_entropy_with_logits, whatever ran before."""
    from sgformer_amd import launch
    launch.unpatch_bce_loss()
    yield
    launch.unpatch_bce_loss()


@pytest.fixture
def cpu_table():
    from sgformer_amd import ops
    from tests.cpu_kernels_bce import CpuKernelsBce
    prev = ops.set_kernels(CpuKernelsBce())
    yield
    ops.set_kernels(prev)


def _dense_target(target, n, c):
    """float64 [n, c] view of any of the three target kinds (class index outside [0, c): an all-zero row)."""
    if target.shape == (n, c):
        return target.double()
    return (target.reshape(-1)[:, None] == torch.arange(c)[None, :]).double()


def _reference(logits, target, rows, denom=None):
    """fp64 torch on the stored logits: loss and the [n, c] gradient."""
    n, c = logits.shape
    x = logits.detach().double().requires_grad_(True)
    t = _dense_target(target, n, c)
    if rows.numel() == 0:
        return torch.zeros((), dtype=torch.float64), torch.zeros(n, c, dtype=torch.float64)
    if denom is None:
        loss = F.binary_cross_entropy_with_logits(x[rows], t[rows])
    else:
        loss = F.binary_cross_entropy_with_logits(x[rows], t[rows], reduction="sum") / (denom * c)
    loss.backward()
    return loss.detach(), x.grad


def _check(loss, grad, lref, gref, bf16=False):
    loss = loss.detach()
    assert abs(float(loss) - float(lref)) <= 2e-6 * abs(float(lref)) + 1e-6, (float(loss), float(lref))
    gmax = float(gref.abs().max())
    bound = ((2.0 ** -8 + 1e-6) if bf16 else 1e-6) * gmax
    assert float((grad.double() - gref).abs().max()) <= bound, (float((grad.double() - gref).abs().max()), bound)


def _logits(n, c, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, generator=g) * 3
    x.view(-1)[::17] = 60.0
    x.view(-1)[5::23] = -60.0
    x.view(-1)[7::29] = 0.0
    return x.to(dtype)


def _targets(kind, n, c, seed):
    g = torch.Generator().manual_seed(seed + 100)
    if kind == "f32":
        return torch.rand(n, c, generator=g)                       # soft targets
    if kind == "i64":
        return torch.randint(0, 2, (n, c), generator=g)
    if kind == "bool":
        return torch.randint(0, 2, (n, c), generator=g).bool()
    if kind == "class":
        return torch.randint(0, c, (n,), generator=g)
    if kind == "class_n1":
        return torch.randint(0, c, (n, 1), generator=g)
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", ["f32", "i64", "bool", "class", "class_n1"])
@pytest.mark.parametrize("rows", ["int64", "mask", "none"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bce_loss_rows_matches_fp64_torch(cpu_table, kind, rows, dtype):
    from sgformer_amd import ops
    n, c = 61, 7
    logits = _logits(n, c, 1, dtype).requires_grad_(True)
    target = _targets(kind, n, c, 1)
    sel = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:23]
    if rows == "int64":
        idx = sel
    elif rows == "mask":
        idx = torch.zeros(n, dtype=torch.bool)
        idx[sel] = True
        sel = idx.nonzero().view(-1)
    else:
        idx, sel = None, torch.arange(n)
    loss = ops.bce_loss_rows(logits, target, idx)
    loss.backward()
    lref, gref = _reference(logits, target, sel)
    assert logits.grad.dtype == dtype and loss.dtype == torch.float32
    _check(loss, logits.grad, lref, gref, bf16=dtype == torch.bfloat16)
    off = torch.ones(n, dtype=torch.bool)
    off[sel] = False
    assert int(torch.count_nonzero(logits.grad[off])) == 0


def test_public_entry_and_denominator_override(cpu_table):
    from sgformer_amd import loss as L
    n, c = 50, 5
    logits = _logits(n, c, 2).requires_grad_(True)
    target = _targets("i64", n, c, 2)
    idx = torch.arange(0, n, 3)
    out = L.bce_with_logits_rows(logits, target, idx, denom=40)
    out.backward()
    lref, gref = _reference(logits, target, idx, denom=40)
    _check(out, logits.grad, lref, gref)
    assert "large/main.py:130-137" in L.bce_with_logits_rows.__doc__


def test_no_training_rows_gives_zero_loss_and_zero_gradient(cpu_table):
    from sgformer_amd import ops
    logits = _logits(20, 4, 3).requires_grad_(True)
    for idx in (torch.zeros(0, dtype=torch.int64), torch.zeros(20, dtype=torch.bool)):
        logits.grad = None
        loss = ops.bce_loss_rows(logits, _targets("f32", 20, 4, 3), idx)
        loss.backward()
        assert float(loss) == 0.0 and int(torch.count_nonzero(logits.grad)) == 0


def test_class_index_out_of_range_is_an_all_zero_target_row(cpu_table):
    from sgformer_amd import ops
    n, c = 30, 6
    logits = _logits(n, c, 4).requires_grad_(True)
    target = _targets("class", n, c, 4)
    target[3], target[10], target[11] = -1, c, 10 ** 12
    idx = torch.arange(n)
    loss = ops.bce_loss_rows(logits, target, idx)
    loss.backward()
    assert torch.isfinite(loss) and bool(torch.isfinite(logits.grad).all())
    dense = _dense_target(target, n, c)
    assert float(dense[3].sum()) == 0 and float(dense[10].sum()) == 0 and float(dense[11].sum()) == 0
    lref, gref = _reference(logits, dense, idx)
    _check(loss, logits.grad, lref, gref)


@pytest.mark.parametrize("case", ["float_class_indices", "wrong_rows", "indices_for_one_column", "wrong_columns", "1d_logits"])
def test_unreadable_targets_raise_a_clear_error(cpu_table, case):
    from sgformer_amd import ops
    n, c = 12, 3
    logits = torch.randn(n, c)
    if case == "float_class_indices":
        target = torch.zeros(n)
    elif case == "wrong_rows":
        target = torch.zeros(n - 1, dtype=torch.int64)
    elif case == "indices_for_one_column":
        logits, target = torch.randn(n, 1), torch.zeros(n, dtype=torch.int64)
    elif case == "wrong_columns":
        target = torch.zeros(n, c + 1)
    else:
        logits, target = torch.randn(n), torch.zeros(n)
    with pytest.raises(ValueError, match="bce_loss_rows"):
        ops.bce_loss_rows(logits, target, torch.arange(n))


def test_rows_that_overlap_in_memory_are_copied_first(cpu_table):
    """ops.bce_loss_rows on an expanded [1, C] row (stride 0) and on a [1, C] view with strides (1, 1): a real copy is made,
    the result is the reference's."""
    from sgformer_amd import ops
    n, c = 9, 5
    base = _logits(1, c, 5)
    target = _targets("f32", n, c, 5)
    for view, tgt in ((lambda leaf: leaf.expand(n, c), target), (lambda leaf: leaf.reshape(c, 1).t(), target[:1])):
        leaf = base.clone().requires_grad_(True)
        logits = view(leaf)
        assert logits.stride(0) < c
        loss = ops.bce_loss_rows(logits, tgt, None)
        loss.backward()
        ref_leaf = base.double().requires_grad_(True)
        lref = F.binary_cross_entropy_with_logits(view(ref_leaf), tgt.double())
        lref.backward()
        _check(loss, leaf.grad, lref.detach(), ref_leaf.grad)


def test_second_derivative_raises_instead_of_returning_a_constant(cpu_table):
    """The backward is one kernel without a graph: differentiating it again (create_graph=True) is an error autograd
    reports, not a silently wrong zero."""
    from sgformer_amd import ops
    x = _logits(8, 3, 6).requires_grad_(True)
    loss = ops.bce_loss_rows(x, _targets("f32", 8, 3, 6), None)
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(loss, x, create_graph=True)
    g, = torch.autograd.grad(loss, x)                    # the ordinary backward is unaffected
    assert g.shape == x.shape and not g.requires_grad


def test_hip_table_rejects_cpu_tensors():
    """No CPU path in the product: the real kernel table raises on a CPU tensor, as for every other operator."""
    from sgformer_amd import ops
    assert ops.K.name == "hip"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bce_loss_rows(torch.zeros(4, 3), torch.zeros(4, 3), torch.arange(4))


# ------------------------------------------------------------------------------------------------
# node-sharded: the sum over ranks is the full-graph mean
# ------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _problem(kind):
    n, c = 203, 5                         # 203 is not divisible by 2: uneven shards
    logits = _logits(n, c, 7)
    target = _targets(kind, n, c, 7)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(8))[: n // 2]
    return n, c, logits, target, idx


def _worker(rank, world, port, kind, ret):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        from sgformer_amd import ops
        from sgformer_amd.dist import ShardContext, sharded_bce_loss
        from tests.cpu_kernels_bce import CpuKernelsBce
        ops.set_kernels(CpuKernelsBce())
        n, c, logits, target, idx = _problem(kind)
        ctx = ShardContext(n)
        local = ctx.shard_rows(logits).clone().requires_grad_(True)
        loss = sharded_bce_loss(local, ctx.shard_rows(target), ctx.local_index(idx), idx.numel())
        loss.backward()
        total = loss.detach().clone()
        dist.all_reduce(total)
        ret[rank] = (float(total), ctx.r0, ctx.r1, local.grad.clone())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("kind", ["i64", "class"])
def test_sharded_bce_loss_sums_to_the_full_graph_mean(kind):
    from sgformer_amd import ops
    from tests.cpu_kernels_bce import CpuKernelsBce
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), kind, ret), nprocs=world, join=True)
    assert len(ret) == world
    n, c, logits, target, idx = _problem(kind)
    prev = ops.set_kernels(CpuKernelsBce())
    try:
        single = logits.clone().requires_grad_(True)
        lsingle = ops.bce_loss_rows(single, target, idx)
        lsingle.backward()
    finally:
        ops.set_kernels(prev)
    grad = torch.zeros(n, c)
    for rank in range(world):
        total, r0, r1, g = ret[rank]
        assert abs(total - float(lsingle)) <= 2e-6 * abs(float(lsingle)) + 1e-6
        grad[r0:r1] = g[: r1 - r0]
    assert float((grad - single.grad).abs().max()) <= 1e-6 * float(single.grad.abs().max())
    lref, gref = _reference(logits, target, idx)
    _check(lsingle, grad, lref, gref)


# ------------------------------------------------------------------------------------------------
# the launcher patch behind torch.nn.functional.binary_cross_entropy_with_logits
# ------------------------------------------------------------------------------------------------
class _Spy:
    def __init__(self):
        self.calls = 0


@pytest.fixture
def patched_bce(monkeypatch):
    from sgformer_amd import launch, ops
    from tests.cpu_kernels_bce import CpuKernelsBce
    table = CpuKernelsBce()
    spy = _Spy()
    inner = table.bce_fwd

    def bce_fwd(*a, **k):
        spy.calls += 1
        return inner(*a, **k)

    table.bce_fwd = bce_fwd
    prev = ops.set_kernels(table)
    bce0 = F.binary_cross_entropy_with_logits
    launch.patch_bce_loss(min_elements=0)        # every size: these tests drive the one-pass form with small inputs
    try:
        yield bce0, spy
    finally:
        launch.unpatch_bce_loss()
        ops.set_kernels(prev)
    assert F.binary_cross_entropy_with_logits is bce0


def _value_and_grad(fn, x, *args, **kw):
    x = x.detach().clone().requires_grad_(True)
    out = fn(x, *args, **kw)
    w = torch.arange(1, out.numel() + 1, dtype=out.dtype).reshape(out.shape) / out.numel()
    g, = torch.autograd.grad((out * w).sum(), x)
    return out.detach(), g


def test_patch_takes_the_trainers_case_in_one_pass(patched_bce):
    """`criterion(out[train_idx], true_label.squeeze(1)[train_idx].to(torch.float))` with criterion = nn.BCEWithLogitsLoss()."""
    bce0, spy = patched_bce
    n, c = 90, 112
    out = _logits(n, c, 11).requires_grad_(True)
    true_label = _targets("i64", n, c, 11).unsqueeze(1)
    train_idx = torch.arange(0, n, 2)
    criterion = nn.BCEWithLogitsLoss()
    loss = criterion(out[train_idx], true_label.squeeze(1)[train_idx].to(torch.float))
    assert spy.calls == 1 and loss.dtype == torch.float32 and loss.shape == ()
    loss.backward()
    lref, gref = _reference(out, true_label.squeeze(1), train_idx)
    _check(loss, out.grad, lref, gref)
    # bf16 logits and targets: torch's own result dtype, the same arithmetic on the stored values
    out16 = _logits(n, c, 12, torch.bfloat16).requires_grad_(True)
    t16 = _targets("i64", n, c, 12).to(torch.bfloat16)
    loss16 = F.binary_cross_entropy_with_logits(out16, t16)
    assert spy.calls == 2 and loss16.dtype == bce0(out16.detach(), t16).dtype == torch.bfloat16
    loss16.backward()
    lref, gref = _reference(out16, t16, torch.arange(n))
    assert abs(float(loss16) - float(lref)) <= 2.0 ** -8 * abs(float(lref)) + 1e-6     # (the loss itself is stored in bf16)
    assert float((out16.grad.double() - gref).abs().max()) <= (2.0 ** -8 + 1e-6) * float(gref.abs().max())


@pytest.mark.parametrize("case", ["pos_weight", "weight", "sum", "none", "1d", "int_target", "non_contiguous", "f64_target",
                                  "f64_input", "target_needs_grad", "empty", "module", "module_pos_weight",
                                  "size_average", "3d", "expanded_rows", "one_row_view"])
def test_patch_third_party_calls_reach_the_original(patched_bce, case):
    """Every call outside the trainers' exact case gives the un-patched function's value and gradient, through the original
    (the kernel table is not entered)."""
    bce0, spy = patched_bce
    g = torch.Generator().manual_seed(21)
    n, c = 14, 6
    x = torch.randn(n, c, generator=g)
    t = torch.randint(0, 2, (n, c), generator=g).float()
    kw = {}
    fn_new, fn_old = F.binary_cross_entropy_with_logits, bce0
    if case == "pos_weight":
        kw = dict(pos_weight=torch.rand(c, generator=g) + 0.5)
    elif case == "weight":
        kw = dict(weight=torch.rand(n, c, generator=g))
    elif case in ("sum", "none"):
        kw = dict(reduction=case)
    elif case == "1d":
        x, t = x.reshape(-1), t.reshape(-1)
    elif case == "int_target":
        t = t.long()
    elif case == "non_contiguous":
        x, t = torch.randn(c, n, generator=g).t(), t
    elif case == "f64_target":
        t = t.double()
    elif case == "f64_input":
        x, t = x.double(), t.double()
    elif case == "target_needs_grad":
        t = torch.rand(n, c, generator=g).requires_grad_(True)
    elif case == "empty":
        x, t = torch.zeros(0, c), torch.zeros(0, c)
    elif case == "module":
        crit = nn.BCEWithLogitsLoss(reduction="sum")
        fn_new = lambda a, b: crit(a, b)                                                  # noqa: E731
        fn_old = lambda a, b: bce0(a, b, reduction="sum")                                 # noqa: E731
    elif case == "module_pos_weight":
        pw = torch.rand(c, generator=g) + 0.5
        crit = nn.BCEWithLogitsLoss(pos_weight=pw)
        fn_new = lambda a, b: crit(a, b)                                                  # noqa: E731
        fn_old = lambda a, b: bce0(a, b, pos_weight=pw)                                   # noqa: E731
    elif case == "size_average":
        kw = dict(size_average=False)
    elif case == "3d":
        x, t = torch.randn(3, 4, 5, generator=g), torch.rand(3, 4, 5, generator=g)
    elif case == "expanded_rows":               # row stride 0 < c: legal for ATen, not a matrix the kernels can address
        x = torch.randn(1, c, generator=g)
        fn_new = lambda a, b: F.binary_cross_entropy_with_logits(a.expand(n, c), b)      # noqa: E731
        fn_old = lambda a, b: bce0(a.expand(n, c), b)                                     # noqa: E731
    elif case == "one_row_view":                # [1, c] view with strides (1, 1)
        x, t = torch.randn(c, 1, generator=g).t(), t[:1]
    if case == "int_target":            # torch's own behaviour, whatever it is, must surface unchanged
        try:
            ref = _value_and_grad(fn_old, x, t, **kw)
        except Exception as e:          # noqa: BLE001
            with pytest.raises(type(e)):
                fn_new(x, t, **kw)
            assert spy.calls == 0
            return
    else:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = _value_and_grad(fn_old, x, t, **kw)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = _value_and_grad(fn_new, x, t, **kw)
    assert spy.calls == 0
    assert got[0].dtype == ref[0].dtype and got[0].shape == ref[0].shape
    assert torch.equal(got[0], ref[0]) or (case == "empty" and bool(torch.isnan(got[0]).all()) and bool(torch.isnan(ref[0]).all()))
    assert torch.equal(got[1], ref[1]) or (case == "empty" and got[1].shape == ref[1].shape)
    if case == "target_needs_grad":
        tg, = torch.autograd.grad(F.binary_cross_entropy_with_logits(x, t), t)
        assert torch.equal(tg, torch.autograd.grad(bce0(x, t), t)[0])


def test_default_patch_keeps_small_inputs_on_the_original(patched_bce):
    """patch_bce_loss() without arguments takes inputs of at least launch.BCE_PATCH_MIN_ELEMENTS elements (the measured size
    from which the one-pass form is not the slower one); a smaller input gives the original's very result."""
    from sgformer_amd import launch
    bce0, spy = patched_bce
    launch.patch_bce_loss()
    assert F.binary_cross_entropy_with_logits._sgf_orig is bce0
    c = 112
    n_big = -(-launch.BCE_PATCH_MIN_ELEMENTS // c)
    g = torch.Generator().manual_seed(5)
    for n, taken in ((n_big - 1, False), (n_big, True)):
        x = torch.randn(n, c, generator=g)
        t = torch.randint(0, 2, (n, c), generator=g).float()
        assert (x.numel() >= launch.BCE_PATCH_MIN_ELEMENTS) == taken
        before = spy.calls
        got = F.binary_cross_entropy_with_logits(x, t)
        assert spy.calls == before + int(taken)
        ref = bce0(x, t)
        assert torch.equal(got, ref) if not taken else abs(float(got) - float(ref)) <= 2e-6 * abs(float(ref)) + 1e-6


def test_patch_surfaces_torchs_error_for_a_target_of_another_shape(patched_bce):
    bce0, spy = patched_bce
    x, t = torch.randn(6, 4), torch.rand(6, 3)
    with pytest.raises(ValueError) as want:
        bce0(x, t)
    with pytest.raises(ValueError) as got:
        F.binary_cross_entropy_with_logits(x, t)
    assert str(got.value) == str(want.value) and spy.calls == 0
    with pytest.raises(ValueError):
        nn.BCEWithLogitsLoss()(x, t)


def test_modules_look_the_patch_up_at_call_time(patched_bce):
    bce0, spy = patched_bce
    x, t = _logits(10, 4, 31), _targets("f32", 10, 4, 31)
    crit = nn.BCEWithLogitsLoss()
    got = _value_and_grad(lambda a, b: crit(a, b), x, t)
    ref = _value_and_grad(bce0, x.double(), t.double())
    assert spy.calls == 1
    _check(got[0], got[1], ref[0], ref[1])


def test_patch_leaves_cpu_tensors_alone_under_the_hip_table():
    """With the product's kernel table a CPU input is not the patch's business: ATen's result, no 'no CPU fallback' error."""
    from sgformer_amd import launch, ops
    assert ops.K.name == "hip"
    bce0 = F.binary_cross_entropy_with_logits
    launch.patch_bce_loss()
    try:
        x, t = _logits(9, 5, 41), _targets("f32", 9, 5, 41)
        got = _value_and_grad(F.binary_cross_entropy_with_logits, x, t)
        crit = _value_and_grad(lambda a, b: nn.BCEWithLogitsLoss()(a, b), x, t)
        ref = _value_and_grad(bce0, x, t)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
        assert torch.equal(crit[0], ref[0]) and torch.equal(crit[1], ref[1])
    finally:
        launch.unpatch_bce_loss()
    assert F.binary_cross_entropy_with_logits is bce0


def test_patch_is_idempotent_and_unpatch_restores_the_original():
    from sgformer_amd import launch
    bce0 = F.binary_cross_entropy_with_logits
    assert not hasattr(bce0, "_sgf_orig")
    launch.patch_bce_loss()
    first = F.binary_cross_entropy_with_logits
    launch.patch_bce_loss()
    try:
        assert first is not bce0 and F.binary_cross_entropy_with_logits._sgf_orig is bce0 and first._sgf_orig is bce0
    finally:
        launch.unpatch_bce_loss()
    assert F.binary_cross_entropy_with_logits is bce0
    launch.unpatch_bce_loss()                      # nothing installed: a no-op
    assert F.binary_cross_entropy_with_logits is bce0


@pytest.mark.parametrize("mode", ["all", "minimal", "aten_loss"])
def test_launcher_modes(tmp_path, monkeypatch, mode):
    """`--sgf-patches all` installs the patch; `minimal` and `--sgf-aten-loss 1` leave F.binary_cross_entropy_with_logits the
    very object it was."""
    import builtins
    import types
    from sgformer_amd import launch
    tdir = tmp_path / "large"
    tdir.mkdir()
    trainer = tdir / "main.py"
    trainer.write_text("import builtins, torch.nn.functional as F\nbuiltins._sgf_seen_bce = F.binary_cross_entropy_with_logits\n")
    tg = types.ModuleType("torch_geometric")
    tgu = types.ModuleType("torch_geometric.utils")
    tgu.subgraph, tgu.to_undirected, tgu.remove_self_loops, tgu.add_self_loops = "pyg-subgraph", "pyg-und", "pyg-rsl", "pyg-asl"
    tg.utils = tgu
    monkeypatch.setitem(sys.modules, "torch_geometric", tg)
    monkeypatch.setitem(sys.modules, "torch_geometric.utils", tgu)
    monkeypatch.setitem(sys.modules, "ours", None)
    monkeypatch.setattr(sys, "argv", list(sys.argv))
    monkeypatch.setattr(sys, "path", list(sys.path))
    adam0, adam_flag = torch.optim.Adam.__init__, getattr(torch.optim.Adam, "_sgf_patched", False)
    bce0 = F.binary_cross_entropy_with_logits
    extra = {"all": [], "minimal": ["--sgf-patches", "minimal"], "aten_loss": ["--sgf-aten-loss", "1"]}[mode]
    try:
        launch.main(extra + [str(trainer)])
        seen = builtins._sgf_seen_bce
        if mode == "all":
            assert seen is not bce0 and seen._sgf_orig is bce0 and F.binary_cross_entropy_with_logits is seen
        else:
            assert seen is bce0 and F.binary_cross_entropy_with_logits is bce0
    finally:
        if hasattr(builtins, "_sgf_seen_bce"):
            del builtins._sgf_seen_bce
        launch.unpatch_bce_loss()
        launch.unpatch_nll_loss()
        torch.optim.Adam.__init__ = adam0
        torch.optim.Adam._sgf_patched = adam_flag
    assert F.binary_cross_entropy_with_logits is bce0


def test_abi_lists_the_new_entry_points():
    """header, binding table and kernel table name the same three symbols (tests/test_host.py checks the library)."""
    from sgformer_amd import _lib
    from sgformer_amd.kernels import HipKernels
    header = open(os.path.join(ROOT, "include", "sgf.h")).read()
    for name in ("sgf_bce_workspace_bytes", "sgf_bce_fwd", "sgf_bce_bwd"):
        assert name in _lib.SIGNATURES and name + "(" in header
    assert callable(HipKernels.bce_fwd) and callable(HipKernels.bce_bwd)
    assert "SGF_BCE_TARGET_CLASS 2" in header and _lib.SGF_BCE_TARGET_CLASS == 2
