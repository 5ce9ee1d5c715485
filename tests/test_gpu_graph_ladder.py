"""The graph-construction kernels at their lap boundaries, bit for bit against the numpy restatements of oracle/:
sgf_subgraph_csr_* (csrc/subgraph_csr.hip), sgf_subgraph_* (csrc/subgraph.hip), sgf_csr_build / sgf_csr_transpose
(csrc/csr.hip), sgf_graph_prologue_* (csrc/prologue.hip) and sgf_sampled_csr_* (csrc/sampled_csr.hip).  The inputs and
references come from tests/graph_ladder.py; tests/test_graph_ladder_host.py proves on the CPU that every case below holds
the boundary its id names.  Every comparison is array_equal on integers and on uint32 views of fp32 values."""
import functools

import numpy as np
import pytest
import torch

from oracle import sgformer_oracle as O
from tests import graph_ladder as L

pytestmark = pytest.mark.gpu

# ---- 1 + 2: subgraph_csr ----
LADDER_M, LADDER_N, LADDER_SEED = 3000, 20000, 11
LADDER_POSITIONS = tuple([0] + list(range(7, 7 + 22 * 134, 22)) + [LADDER_M - 1])     # 136 probe rows: 17 lengths x 8 patterns
MILLION = L.ROW_THREAD_LAP + 257
BATCH_SIZES = (1, 2, 3, 4, 5, 64, 65, 128, 129, L.WALK_LAP, L.WALK_LAP + 1, 2 * L.WALK_LAP + 3, MILLION)
HYGIENE_M = 2500


@functools.lru_cache(maxsize=None)
def batch_inputs(key):
    """(edge_index, n, subset, probe positions, probe rows) of case `key`: "rows" (the row ladder) or a batch size."""
    if key == "rows":
        pos, rows = LADDER_POSITIONS, L.ALL_ROWS
        return L.parent_ladder(LADDER_M, pos, rows, LADDER_N, LADDER_SEED) + (pos, rows)
    m = int(key)
    pos = tuple(L.lap_positions(m))
    rows = L.batch_rows(m, len(pos))
    return L.parent_ladder(m, pos, rows, 1100000 if m > L.ROW_THREAD_LAP else 0, 100 + m % 97) + (pos, rows)


@functools.lru_cache(maxsize=None)
def batch_reference(key):
    ei, n, subset = batch_inputs(key)[:3]
    return L.ref_batch(ei, n, subset)


@functools.lru_cache(maxsize=None)
def hygiene_subset():
    """A second valid batch of the row ladder's parent: other nodes, probe rows among them."""
    n = batch_inputs("rows")[1]
    return torch.from_numpy(np.random.RandomState(5).permutation(n)[:HYGIENE_M].astype(np.int64))


@functools.lru_cache(maxsize=None)
def hygiene_reference():
    ei, n = batch_inputs("rows")[:2]
    return L.ref_batch(ei, n, hygiene_subset())


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_batch(eid, n, subd, ref, fresh_parent=True):
    """batching.subgraph(relabel_nodes=True) on the parent-CSR path against the reference of the batch."""
    from sgformer_amd import batching, ops
    _, rowptr, colind, val, deg = ref
    m = int(subd.numel())
    if fresh_parent:
        batching._parents.clear()
    out, none = batching.subgraph(subd, eid, num_nodes=n, relabel_nodes=True)
    hints = ops.hints_of(out)
    assert none is None and hints.csr is not None and hints.trusted
    rb, cb, vb, db = (t.cpu().numpy() for t in hints.csr)
    assert np.array_equal(rb, rowptr)
    assert np.array_equal(db, deg)
    assert np.array_equal(cb, colind)
    assert np.array_equal(_u32(vb), _u32(val))
    got = out.cpu().numpy()
    assert got.shape == (2, colind.size)
    assert np.array_equal(got[0], colind) and np.array_equal(got[1], np.repeat(np.arange(m), np.diff(rowptr)))
    assert hints.max_in_degree == int(np.diff(rowptr).max())
    parent = next(reversed(batching._parents.values()))[1]
    assert int((parent.local_of != -1).sum()) == 0
    return parent


def test_subgraph_csr_row_ladder(cuda):
    """Parent rows of 0 .. 4097 entries x eight keep patterns: the chunk-to-chunk carry of k_walk's write slot."""
    ei, n, subset = batch_inputs("rows")[:3]
    _check_batch(ei.to(cuda), n, subset.to(cuda), batch_reference("rows"))


@pytest.mark.parametrize("m", BATCH_SIZES, ids=[f"m{m}" for m in BATCH_SIZES])
def test_subgraph_csr_batch_size_ladder(cuda, m):
    """Batch sizes on both sides of a power of two (the sort width), of k_walk's row lap and of the thread lap of k_mark /
    k_unmark / k_off32 / k_values, probe rows on both sides of every lap."""
    ei, n, subset = batch_inputs(m)[:3]
    _check_batch(ei.to(cuda), n, subset.to(cuda), batch_reference(m))


def test_subgraph_csr_table_hygiene(cuda):
    """One parent, one local_of table: a valid batch, a subset with a repeated node, subsets that leave the graph, then
    another valid batch - the rejected calls carry no CSR and leave no mark, the last batch is bit-exact."""
    from sgformer_amd import batching, ops
    ei, n, subset = batch_inputs("rows")[:3]
    eid, subd = ei.to(cuda), subset.to(cuda)
    parent = _check_batch(eid, n, subd, batch_reference("rows"))
    bad = [torch.cat([subd[:50], subd[3:8]]), torch.cat([subd[:40], subd.new_tensor([-1])]),
           torch.cat([subd.new_tensor([n]), subd[:40]])]
    for sub in bad:
        out, _ = batching.subgraph(sub, eid, num_nodes=n, relabel_nodes=True)
        assert ops.hints_of(out).csr is None
        assert next(reversed(batching._parents.values()))[1] is parent
        assert int((parent.local_of != -1).sum()) == 0
    again = _check_batch(eid, n, hygiene_subset().to(cuda), hygiene_reference(), fresh_parent=False)
    assert again is parent


# ---- 4: the edge pass ----
EDGE_NNZ = (1, 255, 256, 257, L.EDGE_LAP, L.EDGE_LAP + 1, L.SG_BLOCKS * 512 + 1)


@functools.lru_cache(maxsize=None)
def edge_inputs(nnz, pattern):
    return L.edge_pass_case(nnz, pattern, seed=nnz % 1000 + len(pattern))


@pytest.mark.parametrize("pattern", L.EDGE_PATTERNS)
@pytest.mark.parametrize("nnz", EDGE_NNZ, ids=[f"nnz{k}" for k in EDGE_NNZ])
def test_subgraph_edge_pass(cuda, monkeypatch, nnz, pattern):
    """sgf_subgraph_plan / _emit with the kept edges at prescribed places of the blocks' chunks: the mask reference exactly,
    original order kept, with and without relabelling, with the kept positions (the edge_attr path)."""
    from sgformer_amd import batching, ops
    ei, n, subset, keep = edge_inputs(nnz, pattern)
    plain = L.ref_subgraph(subset, ei, n, False)[0].numpy()
    relabelled = L.ref_subgraph(subset, ei, n, True)[0].numpy()
    eid, subd = ei.to(cuda), subset.to(cuda)
    out, none = batching.subgraph(subd, eid, relabel_nodes=False, num_nodes=n)
    assert none is None and np.array_equal(out.cpu().numpy(), plain)
    attr = torch.arange(nnz, dtype=torch.int64, device=cuda)             # the attribute of an edge: its position
    out, kept = batching.subgraph(subd, eid, edge_attr=attr, relabel_nodes=True, num_nodes=n)
    assert ops.hints_of(out).csr is None
    assert np.array_equal(out.cpu().numpy(), relabelled) and np.array_equal(kept.cpu().numpy(), np.flatnonzero(keep))
    out, kept = batching.subgraph(subd, eid, edge_attr=attr, relabel_nodes=False, num_nodes=n)
    assert np.array_equal(out.cpu().numpy(), plain) and np.array_equal(kept.cpu().numpy(), np.flatnonzero(keep))
    monkeypatch.setenv("SGF_SUBGRAPH_CSR", "0")
    out, none = batching.subgraph(subd, eid, relabel_nodes=True, num_nodes=n)
    assert none is None and ops.hints_of(out).csr is None and np.array_equal(out.cpu().numpy(), relabelled)


# ---- 5: csr_build / csr_transpose ----
CSR_SMALL_N = (1, 2, 3, 256, 257, 65536, 65537)
CSR_LARGE_NNZ = (L.EDGE_LAP, L.EDGE_LAP + 1, 2 * L.EDGE_LAP + 5)
CSR_HUB = 100000


@functools.lru_cache(maxsize=None)
def csr_inputs(kind, size):
    return L.csr_small(size, seed=size % 1000) if kind == "n" else L.csr_large(size, seed=size % 1000, hub=CSR_HUB)


@functools.lru_cache(maxsize=None)
def symmetric_inputs():
    return L.symmetric_trio(seed=3)


def _check_csr(cuda, ei, n):
    from sgformer_amd import ops
    e = ei.to(cuda).contiguous()
    rowptr, colind, val, deg = O.csr_build(ei.numpy(), n)
    rp, ci, va, dg = ops.K.csr_build(e, n)
    assert np.array_equal(rp.cpu().numpy(), rowptr) and np.array_equal(ci.cpu().numpy(), colind)
    assert np.array_equal(dg.cpu().numpy(), deg) and np.array_equal(_u32(va.cpu().numpy()), _u32(val))
    t_rowptr, t_colind, t_val, sym = O.csr_transpose(ei.numpy(), n)
    trp, tci, tva, flag = ops.K.csr_transpose(e, n, dg, rp, ci)
    assert np.array_equal(trp.cpu().numpy(), t_rowptr) and np.array_equal(tci.cpu().numpy(), t_colind)
    assert np.array_equal(_u32(tva.cpu().numpy()), _u32(t_val))
    assert flag is sym
    return sym


@pytest.mark.parametrize("n", CSR_SMALL_N, ids=[f"n{n}" for n in CSR_SMALL_N])
def test_csr_key_width(cuda, n):
    """n at 2^k and 2^k + 1 with edges out of and into node n - 1: the radix sort's 32 + ceil(log2 n) bits."""
    _check_csr(cuda, *csr_inputs("n", n))


@pytest.mark.parametrize("nnz", CSR_LARGE_NNZ, ids=[f"nnz{k}" for k in CSR_LARGE_NNZ])
def test_csr_past_the_edge_lap(cuda, nnz):
    """The grid-stride loops of the histogram, the key packing, finalize and k_compare on their second and third lap, one
    hub row of 10^5 entries with stored duplicates."""
    assert _check_csr(cuda, *csr_inputs("nnz", nnz)) is False


@pytest.mark.parametrize("which", ["symmetric", "twin_late", "twin_last"])
def test_symmetry_flag_past_the_edge_lap(cuda, which):
    """k_compare decides whether the backward reuses the forward CSR: True on a symmetric graph of > EDGE_LAP entries, False
    when A and A^T differ only behind position EDGE_LAP, False when only the last stored entry was changed."""
    trio = symmetric_inputs()
    ei = trio[("symmetric", "twin_late", "twin_last").index(which)]
    assert _check_csr(cuda, ei, trio[3]) is (which == "symmetric")


# ---- 6: prologue ----
@functools.lru_cache(maxsize=None)
def prologue_inputs(name):
    return L.prologue_case(name, seed=len(name))


@pytest.mark.parametrize("name", L.PROLOGUE_CASES)
def test_prologue_ladder(cuda, name):
    from sgformer_amd import batching
    ei, n, undirected = prologue_inputs(name)
    out = batching.graph_prologue(ei.to(cuda), n, undirected=undirected)
    assert out.dtype == torch.int64 and np.array_equal(out.cpu().numpy(), L.ref_prologue(ei, n, undirected))


# ---- 7: sampled_csr, direct calls ----
SENTINEL = 0x5A5A5A5A
# (id, rows, one repeated source per row, node slack, edge slack, max_fanout)
SAMPLED_BUILD = (("ladder", "ladder", False, 37, 91, 256), ("over_the_bound", "over", False, 5, 3, 256),
                 ("repeated_source", "ladder", True, 1, 1, 256), ("over_repeated", "over", True, 9, 700, 256),
                 ("no_edges", "empty", False, 11, 64, 5), ("full_capacity", "ladder", False, 0, 0, 256),
                 ("edge_lap", "lap", False, 3, 5, 4))


@functools.lru_cache(maxsize=None)
def sampled_inputs(rows, one_source):
    if rows == "empty":
        return L.sampled_case([], 50, seed=1)
    lens, nn = L.sampled_rows(rows)
    return L.sampled_case(lens, nn, seed=len(rows), one_source=one_source)


@pytest.mark.parametrize("case", SAMPLED_BUILD, ids=[c[0] for c in SAMPLED_BUILD])
def test_sampled_csr_build_prefixes_and_tails(cuda, case):
    """sgf_sampled_csr_build on sampler-shaped inputs with capacities above the counts: the prefixes equal csr_build bit for
    bit and nothing is written behind them (include/sgf.h) - rows of 0 .. 256 entries, rows above the advisory bound, rows
    of one repeated source, no edge at all, counts equal to the capacities, the second lap of the one-thread-per-edge grid."""
    from sgformer_amd import kernels
    _, rows, one_source, node_slack, edge_slack, fanout = case
    src, dst, nn, ne = sampled_inputs(rows, one_source)
    node_cap, edge_cap = nn + node_slack, ne + edge_slack
    i32 = dict(dtype=torch.int32, device=cuda)
    e_src, e_dst = torch.full((max(edge_cap, 1),), -7, **i32), torch.full((max(edge_cap, 1),), -7, **i32)
    e_src[:ne], e_dst[:ne] = torch.from_numpy(src).to(cuda), torch.from_numpy(dst).to(cuda)
    counts = torch.tensor([nn, ne], dtype=torch.int64, device=cuda)
    rowptr_b = torch.full((node_cap + 1,), SENTINEL, dtype=torch.int64, device=cuda)
    deg_b = torch.full((node_cap + 1,), SENTINEL, **i32)
    colind_b = torch.full((max(edge_cap, 1),), SENTINEL, **i32)
    val_b = torch.full((max(edge_cap, 1),), SENTINEL, **i32)             # fp32 storage, looked at as bits only
    kernels._launch(cuda, "sgf_sampled_csr_build", e_src, e_dst, counts, node_cap, edge_cap, fanout, rowptr_b, colind_b,
                    val_b, deg_b, None, 0)
    rowptr, colind, val, deg = L.ref_sampled(src, dst, nn, ne)
    rb, cb, vb, db = (t.cpu().numpy() for t in (rowptr_b, colind_b, val_b, deg_b))
    assert np.array_equal(rb[:nn + 1], rowptr) and np.array_equal(db[:nn], deg)
    assert np.array_equal(cb[:ne], colind) and np.array_equal(_u32(vb[:ne]), _u32(val))
    assert np.array_equal(rb[nn + 1:], np.full(node_cap - nn, SENTINEL)) and np.array_equal(db[nn:], np.full(node_cap + 1 - nn, SENTINEL))
    assert np.array_equal(cb[ne:], np.full(cb.size - ne, SENTINEL)) and np.array_equal(vb[ne:], np.full(vb.size - ne, SENTINEL))


def test_sampled_csr_build_through_the_kernel_table(cuda):
    """The same ladder through ops.K.sampled_csr_build, as the sampler calls it."""
    from sgformer_amd import ops
    src, dst, nn, ne = sampled_inputs("ladder", False)
    counts = torch.tensor([nn, ne], dtype=torch.int64, device=cuda)
    assert ops.K.sampled_csr_supported(L.MAX_FANOUT) and not ops.K.sampled_csr_supported(L.MAX_FANOUT + 1)
    got = ops.K.sampled_csr_build(torch.from_numpy(src).to(cuda), torch.from_numpy(dst).to(cuda), counts, nn, ne, L.MAX_FANOUT)
    rowptr, colind, val, deg = L.ref_sampled(src, dst, nn, ne)
    rb, cb, vb, db = (t.cpu().numpy() for t in got)
    assert np.array_equal(rb[:nn + 1], rowptr) and np.array_equal(db[:nn], deg)
    assert np.array_equal(cb[:ne], colind) and np.array_equal(_u32(vb[:ne]), _u32(val))


SAMPLED_TRANSPOSE = ("n1", "n256", "n257", "lap")


@functools.lru_cache(maxsize=None)
def transpose_inputs(name):
    return L.transpose_case(name, seed=len(name))


@pytest.mark.parametrize("name", SAMPLED_TRANSPOSE)
def test_sampled_csr_transpose(cuda, name):
    """sgf_sampled_csr_transpose of a forward CSR in ascending source order == csr_transpose's arrays: n at a power of two
    (the sorted source bits), source n - 1 present, empty rows first and last, nnz past the thread lap."""
    from sgformer_amd import ops
    ei, n = transpose_inputs(name)
    rowptr, colind, val, _ = O.csr_build(ei.numpy(), n)
    t_rowptr, t_colind, t_val, _ = O.csr_transpose(ei.numpy(), n)
    trp, tci, tva = ops.K.sampled_csr_transpose(torch.from_numpy(rowptr).to(cuda), torch.from_numpy(colind.astype(np.int32)).to(cuda),
                                                torch.from_numpy(val).to(cuda), n)
    assert np.array_equal(trp.cpu().numpy(), t_rowptr) and np.array_equal(tci.cpu().numpy(), t_colind)
    assert np.array_equal(_u32(tva.cpu().numpy()), _u32(t_val))
