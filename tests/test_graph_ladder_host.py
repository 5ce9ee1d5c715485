"""GPU-free guards of tests/test_gpu_graph_ladder.py: the geometry restated in tests/graph_ladder.py is what the kernel
sources define, every GPU case holds the boundary its id names (row length, lap index, chunk edge, key width, position of the
first difference - all read off the REFERENCE output, never the library's), the vectorised references agree with naive
per-edge loops and with the CPU kernel table, and the CPU side of every case stays within its time budget."""
import os
import re
import time

import numpy as np
import pytest
import torch

from oracle import sgformer_oracle as O
from tests import graph_ladder as L
from tests import test_gpu_graph_ladder as T

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sgformer_amd", "csrc")
BUDGET_SECONDS = 10.0


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _int(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return int(found[0])


# ------------------------------------------------------------------------------------------------
# the restated geometry is the sources'
# ------------------------------------------------------------------------------------------------
def test_geometry_follows_the_sources():
    common = _text("common.h")
    num_cu = _int(r"constexpr int kNumCU = (\d+);", common)
    wave = _int(r"constexpr int kWave = (\d+);", common)
    files = {f: _text(f) for f in ("csr.hip", "subgraph.hip", "subgraph_csr.hip", "prologue.hip", "sampled_csr.hip")}
    threads = {f: _int(r"constexpr int kThreads = (\d+);", t) for f, t in files.items()}
    assert (num_cu, wave) == (L.NUM_CU, L.WAVE) and set(threads.values()) == {L.THREADS}
    cap = {f: _int(r"const int64_t cap = static_cast<int64_t>\(kNumCU\) \* (\d+);", files[f])
           for f in ("csr.hip", "subgraph_csr.hip", "prologue.hip", "sampled_csr.hip")}
    assert cap == {"csr.hip": 8, "prologue.hip": 8, "subgraph_csr.hip": 16, "sampled_csr.hip": 16}
    # subgraph_csr.hip: k_walk gets one wave per row, the other row kernels one thread per row
    sc = files["subgraph_csr.hip"]
    assert "constexpr int kWavesPerBlock = kThreads / kWave;" in sc
    assert sc.count("(k_walk<false>), dim3(grid_rows(m, kWavesPerBlock))") == 1
    assert sc.count("(k_walk<true>), dim3(grid_rows(m, kWavesPerBlock))") == 1
    for kernel, rows in (("k_mark", "m"), ("k_unmark", "m"), ("k_values", "m"), ("k_off32", "m + 1")):
        assert f"hipLaunchKernelGGL({kernel}, dim3(grid_rows({rows}, kThreads))" in sc, kernel
    assert "for (int64_t i = b; i < e; i += kWave)" in sc
    assert L.WALK_LAP == num_cu * cap["subgraph_csr.hip"] * (threads["subgraph_csr.hip"] // wave)
    assert L.ROW_THREAD_LAP == num_cu * cap["subgraph_csr.hip"] * threads["subgraph_csr.hip"]
    assert L.ROW_THREAD_LAP == num_cu * cap["sampled_csr.hip"] * threads["sampled_csr.hip"]
    assert L.EDGE_LAP == num_cu * cap["csr.hip"] * threads["csr.hip"] == num_cu * cap["prologue.hip"] * threads["prologue.hip"]
    # subgraph.hip: the fixed grid and chunk_of
    sg = files["subgraph.hip"]
    assert L.SG_BLOCKS == _int(r"constexpr int kBlocks = (\d+);", sg)
    assert "int64_t c = (nnz + kBlocks - 1) / kBlocks;" in sg and "return (c + kThreads - 1) / kThreads * kThreads;" in sg
    assert sg.count("dim3(kBlocks), dim3(kThreads)") == 2                 # k_count and k_emit
    assert L.MAX_FANOUT == _int(r"constexpr int kMaxFanout = (\d+);", files["sampled_csr.hip"])
    # the three width loops
    loop = "while ((static_cast<int64_t>(1) << b) < n && b < 31) ++b;"
    assert loop in files["csr.hip"] and "return 32u + b;" in files["csr.hip"]
    assert loop in files["prologue.hip"] and "0u, 32u + bits_for(n), st)" in files["prologue.hip"]
    assert loop in files["sampled_csr.hip"]
    assert "while ((int64_t{1} << bits) < m) ++bits;" in sc and "off32, off32 + 1, 0, bits, st)" in sc


def test_restated_functions():
    assert [L.sg_chunk(k) for k in T.EDGE_NNZ] == [256, 256, 256, 256, 256, 512, 768]
    assert [L.key_bits(n) for n in T.CSR_SMALL_N] == [33, 33, 34, 40, 41, 48, 49]
    assert [L.sort_bits(m) for m in T.BATCH_SIZES] == [1, 1, 2, 2, 3, 6, 7, 7, 8, 14, 15, 16, 21]
    assert L.sort_bits(T.LADDER_M) == 12
    from sgformer_amd import _lib
    if _lib.available():
        lib = _lib.load()
        assert lib.sgf_sampled_csr_supported(L.MAX_FANOUT) == 1 and lib.sgf_sampled_csr_supported(L.MAX_FANOUT + 1) == 0


# ------------------------------------------------------------------------------------------------
# subgraph_csr: what the batches hold, from the reference alone
# ------------------------------------------------------------------------------------------------
def _probe_rows(key):
    """Per probe of case `key`: (wanted (length, pattern), parent row's membership in stored order, induced row) - from
    O.csr_build of the parent and of the reference batch."""
    ei, n, subset, positions, rows = T.batch_inputs(key)
    _, rowptr_b, colind_b, _, _ = T.batch_reference(key)
    rowptr, colind, _, _ = O.csr_build(ei.numpy(), n)
    member = np.zeros(n, dtype=bool)
    member[subset.numpy()] = True
    out = []
    for pos, want in zip(positions, rows):
        v = int(subset[pos])
        stored = colind[rowptr[v]:rowptr[v + 1]]
        assert np.all(np.diff(stored) >= 0)
        out.append((want, member[stored], colind_b[rowptr_b[pos]:rowptr_b[pos + 1]], pos))
    return out


def _check_probes(key, every_self_loop=False):
    m = int(T.batch_inputs(key)[2].numel())
    seen, loops = set(), 0
    for (length, pattern), kept, induced, pos in _probe_rows(key):
        mask = L.keep_mask(length, pattern)
        assert kept.size == length and np.array_equal(kept, mask), (key, length, pattern)
        assert induced.size == int(mask.sum())
        chunks = [int(kept[i:i + L.WAVE].sum()) for i in range(0, length, L.WAVE)]
        want = [int(mask[i:i + L.WAVE].sum()) for i in range(0, length, L.WAVE)]
        assert chunks == want
        if induced.size:                                     # the probe's own self-loop is among the kept entries
            loops += pos in induced.tolist()
            assert pos in induced.tolist() or not every_self_loop, (key, length, pattern)
        assert induced.size == 0 or (0 <= induced.min() and induced.max() < m)
        seen.add((length, pattern))
    assert loops >= 1
    return seen


def _corner_row_present(key):
    m = int(T.batch_inputs(key)[2].numel())
    _, rowptr_b, colind_b, _, _ = T.batch_reference(key)
    want = {0, min(1, m - 1), m - 1} | ({1 << (L.sort_bits(m) - 1)} if m > 1 else set())
    rows = np.repeat(np.arange(m), np.diff(rowptr_b))
    hit = np.isin(colind_b, sorted(want))
    cand = np.unique(rows[hit])
    return any(want <= set(colind_b[rowptr_b[r]:rowptr_b[r + 1]].tolist()) for r in cand.tolist())


def test_the_row_ladder_holds_every_length_and_pattern():
    seen = _check_probes("rows", every_self_loop=True)
    assert seen == set(L.ALL_ROWS) and len(seen) == 17 * 8
    ei, n, subset, positions, _ = T.batch_inputs("rows")
    m = int(subset.numel())
    assert (m, n) == (T.LADDER_M, T.LADDER_N) and len(positions) == 136 and {0, m - 1} <= set(positions)
    assert m < L.WALK_LAP                                     # one lap: this case is about the rows
    # the carried total: rows whose first kept entry comes after chunks that kept nothing (a zero carried over), and rows
    # that write from a second or later chunk with a non-zero total carried into the slot
    probes = _probe_rows("rows")
    zero = {(len_, p) for (len_, p), kept, _, _ in probes if len_ > L.WAVE and kept[:L.WAVE].sum() == 0 and kept.sum() > 0}
    assert {(4097, "last"), (1025, "last"), (65, "last")} <= zero
    carried = {(len_, p) for (len_, p), kept, _, _ in probes if kept[:L.WAVE].sum() > 0 and kept[L.WAVE:].sum() > 0}
    assert carried >= {(len_, p) for len_ in L.ROW_LENGTHS if len_ >= 128 for p in ("all", "lane0", "lane63", "alt", "half")}
    assert {(65, "all"), (65, "lane0"), (65, "alt")} <= carried
    # stored duplicates with both copies kept; the subset is no ascending list; one row holds local ids 0, 1, 2^k and m - 1
    assert any(np.any(np.diff(ind) == 0) for _, _, ind, _ in _probe_rows("rows"))
    assert np.any(np.diff(subset.numpy()) < 0)
    assert _corner_row_present("rows")
    # the fillers: one or two parent in-edges each, some kept and some not
    _, rowptr_b, _, _, deg_b = T.batch_reference("rows")
    parent_deg = np.bincount(ei[1].numpy(), minlength=n)[subset.numpy()]
    filler = np.ones(m, dtype=bool)
    filler[list(positions)] = False
    assert set(parent_deg[filler].tolist()) <= {1, 2, 3, 4, 5, 6} and {1, 2} <= set(parent_deg[filler].tolist())
    assert np.any(deg_b[filler] < parent_deg[filler]) and np.any(deg_b[filler] > 0) and np.any(deg_b[filler] == 0)


@pytest.mark.parametrize("m", T.BATCH_SIZES, ids=[f"m{m}" for m in T.BATCH_SIZES])
def test_the_batch_size_ladder_sits_on_its_laps(m):
    ei, n, subset, positions, rows = T.batch_inputs(m)
    assert int(subset.numel()) == m and np.unique(subset.numpy()).size == m and 0 <= int(subset.min()) and int(subset.max()) < n
    assert list(positions) == L.lap_positions(m) and {0, m - 1} <= set(positions)
    seen = _check_probes(m)
    assert len(seen) >= min(len(positions), 2) and any(length > L.WAVE for length, _ in seen)
    assert _corner_row_present(m)
    lap_of = {p: p // L.WALK_LAP for p in positions}
    if m > L.WALK_LAP:
        assert {L.WALK_LAP - 1, L.WALK_LAP} <= set(positions) and {0, 1} <= set(lap_of.values())
    if m > 2 * L.WALK_LAP:
        assert {L.WALK_LAP + 1, 2 * L.WALK_LAP - 1, 2 * L.WALK_LAP} <= set(positions) and 2 in lap_of.values()
    if m > L.ROW_THREAD_LAP:
        assert {L.ROW_THREAD_LAP - 1, L.ROW_THREAD_LAP, L.ROW_THREAD_LAP + 1} <= set(positions) and n >= 1100000
    if m > 2:
        assert np.any(np.diff(subset.numpy()) < 0)


def _walk_fill(local, carry):
    """k_walk<true> on one parent row, restated: `local` = local_of of its stored sources; chunk by chunk, a kept entry goes to
    slot total + (kept entries below its lane).  carry=False is the defect the ladder is there for: a total that is not
    carried from chunk to chunk."""
    out = np.full(int((local >= 0).sum()), -9, dtype=np.int64)
    total = 0
    for c in range(0, local.size, L.WAVE):
        loc = local[c:c + L.WAVE]
        keep = loc >= 0
        rank = np.cumsum(keep) - keep
        out[(total if carry else 0) + rank[keep]] = loc[keep]
        total += int(keep.sum())
    return out


def _sort_on(ids, bits):
    return ids[np.argsort(ids & ((1 << bits) - 1), kind="stable")]


def test_the_ladder_tells_a_dropped_carry_and_a_short_sort_apart():
    """The restated walk + sort gives the reference rows; the same walk without the carried total, or a sort one bit short,
    does not - on the rows / batch sizes that are in the ladder for that reason."""
    ei, n, subset, positions, rows = T.batch_inputs("rows")
    _, rowptr_b, colind_b, _, _ = T.batch_reference("rows")
    rowptr, colind, _, _ = O.csr_build(ei.numpy(), n)
    m = int(subset.numel())
    local_of = np.full(n, -1, dtype=np.int64)
    local_of[subset.numpy()] = np.arange(m)
    caught = set()
    for pos, (length, pattern) in zip(positions, rows):
        v = int(subset[pos])
        local = local_of[colind[rowptr[v]:rowptr[v + 1]]]
        want = colind_b[rowptr_b[pos]:rowptr_b[pos + 1]]
        assert np.array_equal(_sort_on(_walk_fill(local, True), L.sort_bits(m)), want)
        if not np.array_equal(_sort_on(_walk_fill(local, False), L.sort_bits(m)), want):
            caught.add((length, pattern))
    kept_chunks = {r: sum(1 for i in range(0, r[0], L.WAVE) if L.keep_mask(*r)[i:i + L.WAVE].any()) for r in rows}
    assert caught == {r for r in rows if kept_chunks[r] >= 2} >= {(65, "all"), (129, "lane63"), (4097, "half"), (1025, "lane0")}
    for k in (6, 7, 14):                                     # m = 2^k + 1: local id 2^k needs the (k + 1)-th bit
        m = (1 << k) + 1
        _, rowptr_b, colind_b, _, _ = T.batch_reference(m)
        short = [r for r in range(m) if not np.array_equal(_sort_on(colind_b[rowptr_b[r]:rowptr_b[r + 1]], L.sort_bits(m) - 1),
                                                           colind_b[rowptr_b[r]:rowptr_b[r + 1]])]
        assert short, m
        _, rowptr_b, colind_b, _, _ = T.batch_reference(m - 1)               # ... and m = 2^k does not
        assert all(np.array_equal(_sort_on(colind_b[rowptr_b[r]:rowptr_b[r + 1]], L.sort_bits(m - 1)),
                                  colind_b[rowptr_b[r]:rowptr_b[r + 1]]) for r in range(m - 1))


def test_the_batch_sizes_straddle_the_widths_and_laps():
    sizes = set(T.BATCH_SIZES)
    for k in (6, 7, 14):
        assert {1 << k, (1 << k) + 1} <= sizes and L.sort_bits((1 << k) + 1) == L.sort_bits(1 << k) + 1
    assert {1, 2, 3, 4, 5} <= sizes and {L.WALK_LAP, L.WALK_LAP + 1, 2 * L.WALK_LAP + 3, L.ROW_THREAD_LAP + 257} <= sizes
    # the second valid batch of the hygiene test: another subset of the same parent
    a, b = T.batch_inputs("rows")[2], T.hygiene_subset()
    assert b.numel() == T.HYGIENE_M and np.unique(b.numpy()).size == T.HYGIENE_M
    assert 0 < np.intersect1d(a.numpy(), b.numpy()).size < T.HYGIENE_M
    assert int(T.hygiene_reference()[1][-1]) > 0


# ------------------------------------------------------------------------------------------------
# subgraph.hip: the edge pass
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nnz", T.EDGE_NNZ, ids=[f"nnz{k}" for k in T.EDGE_NNZ])
def test_the_edge_pass_cases_keep_what_they_say(nnz):
    chunk = L.sg_chunk(nnz)
    owners = -(-nnz // chunk)                                # blocks that own an edge; the others lie wholly behind nnz
    assert owners <= L.SG_BLOCKS and (owners == L.SG_BLOCKS) == (nnz == L.EDGE_LAP)
    if nnz == T.EDGE_NNZ[-1]:
        assert (chunk, owners) == (768, 1366)
    for pattern in L.EDGE_PATTERNS:
        ei, n, subset, _ = T.edge_inputs(nnz, pattern)
        out, keep = L.ref_subgraph(subset, ei, n, False)
        keep = keep.numpy()
        assert np.array_equal(keep, L.edge_keep(nnz, pattern)) and out.shape[1] == int(keep.sum())
        per_block = np.bincount(np.flatnonzero(keep) // chunk, minlength=L.SG_BLOCKS)
        assert per_block.size == L.SG_BLOCKS and not per_block[owners:].any()
        e = np.flatnonzero(keep)
        if pattern == "all":
            assert e.size == nnz
        elif pattern == "none":
            assert e.size == 0
        elif pattern == "chunk_ends":
            assert set((e % chunk).tolist()) <= {0, chunk - 1} and per_block[:owners - 1].tolist() == [2] * (owners - 1)
            assert keep[0] and (owners == 1 or (keep[chunk - 1] and keep[chunk]))
        elif pattern == "lane0":
            assert set((e % L.WAVE).tolist()) == {0}
        elif pattern == "lane63":
            assert set((e % L.WAVE).tolist()) <= {L.WAVE - 1} and e.size == nnz // L.WAVE
        else:
            assert not per_block[:owners - 1].any() and per_block[owners - 1] == nnz - (owners - 1) * chunk
        member = np.zeros(n, dtype=bool)
        member[subset.numpy()] = True
        s_in, t_in = member[ei[0].numpy()], member[ei[1].numpy()]
        kinds = {(bool(a), bool(b)) for a, b in zip(s_in[~keep][:64].tolist(), t_in[~keep][:64].tolist())}
        if (~keep).sum() >= 5:
            assert kinds == {(False, True), (True, False), (False, False)}
        assert np.any(np.diff(subset.numpy()) < 0)            # relabelling is no identity in disguise


# ------------------------------------------------------------------------------------------------
# csr.hip
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", T.CSR_SMALL_N, ids=[f"n{n}" for n in T.CSR_SMALL_N])
def test_the_small_csr_cases_touch_the_last_node(n):
    ei, n_ = T.csr_inputs("n", n)
    assert n_ == n
    rowptr, colind, _, deg = O.csr_build(ei.numpy(), n)
    out_deg = np.bincount(colind, minlength=n)
    assert deg[n - 1] > 0 and out_deg[n - 1] > 0 and int(colind.max()) == n - 1 and rowptr[n] - rowptr[n - 1] == deg[n - 1]
    for v in {0, n - 2} - {n - 1, -1}:
        assert deg[v] == 0 and out_deg[v] == 0
    assert (1 << (L.key_bits(n) - 32)) >= n and (n <= 2 or (1 << (L.key_bits(n) - 33)) < n)


@pytest.mark.parametrize("nnz", T.CSR_LARGE_NNZ, ids=[f"nnz{k}" for k in T.CSR_LARGE_NNZ])
def test_the_large_csr_cases_pass_the_edge_lap(nnz):
    ei, n = T.csr_inputs("nnz", nnz)
    rowptr, colind, _, deg = O.csr_build(ei.numpy(), n)
    assert colind.size == nnz and -(-nnz // L.EDGE_LAP) == {L.EDGE_LAP: 1, L.EDGE_LAP + 1: 2, 2 * L.EDGE_LAP + 5: 3}[nnz]
    hub = int(np.argmax(deg))
    row = colind[rowptr[hub]:rowptr[hub + 1]]
    assert row.size >= T.CSR_HUB and np.count_nonzero(np.diff(row) == 0) > 1000        # stored duplicates
    assert deg[n - 1] > 0 and int(colind.max()) == n - 1


def test_the_symmetry_cases_differ_where_they_say():
    sym, late, last, n = T.symmetric_inputs()
    rp, ci, _, _ = O.csr_build(sym.numpy(), n)
    t_rp, t_ci, _, flag = O.csr_transpose(sym.numpy(), n)
    assert flag is True and ci.size > L.EDGE_LAP and n + 1 < L.EDGE_LAP
    # twin_late: against the symmetric graph and against its own transpose, nothing differs before position EDGE_LAP, and
    # rowptr (all of it on the first lap) does not differ at all: only second-lap threads of k_compare can see it
    rp2, ci2, _, _ = O.csr_build(late.numpy(), n)
    t_rp2, t_ci2, _, flag2 = O.csr_transpose(late.numpy(), n)
    assert flag2 is False and np.array_equal(rp2, t_rp2)
    assert L.first_difference(ci2, ci) >= L.EDGE_LAP and L.first_difference(ci2, t_ci2) >= L.EDGE_LAP
    assert ci2.size == ci.size + 3
    # twin_last: the same arrays as the symmetric graph but for the very last stored entry
    rp3, ci3, _, _ = O.csr_build(last.numpy(), n)
    assert O.csr_transpose(last.numpy(), n)[3] is False
    assert np.array_equal(rp3, rp) and ci3.size == ci.size and L.first_difference(ci3, ci) == ci.size - 1


# ------------------------------------------------------------------------------------------------
# prologue.hip
# ------------------------------------------------------------------------------------------------
def _longest_run(keys):
    starts = np.concatenate([[0], np.flatnonzero(keys[1:] != keys[:-1]) + 1, [keys.size]])
    i = int(np.argmax(np.diff(starts)))
    return int(starts[i]), int(starts[i + 1])


def test_the_prologue_cases_hold_their_runs():
    assert set(L.PROLOGUE_CASES) == {"one_edge", "straddle", "all_loops", "single", "n256", "n257", "n65536", "n65537", "directed_loops"}
    for name in L.PROLOGUE_CASES:
        ei, n, undirected = T.prologue_inputs(name)
        ref = L.ref_prologue(ei, n, undirected)
        loops = np.stack([np.arange(n), np.arange(n)])
        assert np.array_equal(ref[:, ref.shape[1] - n:], loops) and undirected == (name != "directed_loops")
        body = ref[:, :ref.shape[1] - n]
        if name == "one_edge":
            assert ei.shape[1] > L.EDGE_LAP and np.array_equal(body, [[2, 5], [5, 2]])
            assert _longest_run(L.sorted_keys(ei))[1] > L.EDGE_LAP
        elif name == "straddle":
            b, e = _longest_run(L.sorted_keys(ei))
            assert e - b == 1001 and b < L.EDGE_LAP - 256 and e > L.EDGE_LAP + 256       # whole blocks on either side
            assert body.shape[1] == 2 * (ei.shape[1] - 1000)
        elif name == "all_loops":
            assert bool((ei[0] == ei[1]).all()) and body.shape[1] == 0
        elif name == "single":
            assert ei.shape[1] == 1 and np.array_equal(body, [[1, 3], [3, 1]])
        elif name == "directed_loops":
            m = ei.shape[1]
            assert m > L.EDGE_LAP and int(ei[0, 0]) == int(ei[1, 0]) and int(ei[0, m - 1]) == int(ei[1, m - 1])
            assert int(ei[0, L.EDGE_LAP]) == int(ei[1, L.EDGE_LAP])
            keep = (ei[0] != ei[1]).numpy()
            assert np.array_equal(body, ei.numpy()[:, keep]) and not keep[0] and not keep[m - 1]
        else:
            assert n == int(name[1:]) and body[0, -1] == n - 1
            assert np.any((body[0] == n - 1) & (body[1] == 0)) and np.any((body[0] == 0) & (body[1] == n - 1))


# ------------------------------------------------------------------------------------------------
# sampled_csr.hip
# ------------------------------------------------------------------------------------------------
def test_the_sampled_cases_are_sampler_shaped():
    for name, rows, one_source, node_slack, edge_slack, fanout in T.SAMPLED_BUILD:
        src, dst, nn, ne = T.sampled_inputs(rows, one_source)
        assert src.dtype == dst.dtype == np.int32 and src.size == dst.size == ne
        assert np.all(np.diff(dst) >= 0) and (ne == 0 or (0 <= src.min() and src.max() < nn and dst.max() < nn))
        rowptr, colind, _, deg = L.ref_sampled(src, dst, nn, ne)
        lens = set(np.diff(rowptr).tolist())
        assert fanout <= L.MAX_FANOUT
        if rows == "ladder":
            assert lens == {0, 1, 2, 255, 256} and deg[0] == 0 and deg[nn - 1] == 0 and max(lens) == fanout
        elif rows == "over":
            assert {257, 300} <= lens and max(lens) > fanout
        elif rows == "lap":
            assert ne == L.ROW_THREAD_LAP + 300 and max(lens) == fanout == 4 and {0, 1, 2, 3, 4} == lens
        else:
            assert ne == 0 and nn > 0
        if one_source:
            assert all(np.unique(colind[rowptr[j]:rowptr[j + 1]]).size == 1 for j in np.flatnonzero(np.diff(rowptr) > 0))
        elif ne:
            assert colind.max() == nn - 1
            if rows != "lap":                                # equal sources inside the longest rows
                assert all(np.any(np.diff(colind[rowptr[j]:rowptr[j + 1]]) == 0) for j in np.flatnonzero(np.diff(rowptr) >= 255))
        if name == "full_capacity":
            assert node_slack == 0 and edge_slack == 0
        elif name != "edge_lap":
            assert node_slack > 0 and edge_slack > 0
    for name in T.SAMPLED_TRANSPOSE:
        ei, n = T.transpose_inputs(name)
        rowptr, colind, _, _ = O.csr_build(ei.numpy(), n)
        assert int(colind.max()) == n - 1
        if name == "lap":
            assert colind.size > L.ROW_THREAD_LAP
        elif name != "n1":
            assert n == int(name[1:]) and rowptr[3] == 0 and rowptr[n - 3] == rowptr[n] and L.sort_bits(256) + 1 == L.sort_bits(257)
    assert {"n1", "n256", "n257", "lap"} == set(T.SAMPLED_TRANSPOSE)


# ------------------------------------------------------------------------------------------------
# the references themselves
# ------------------------------------------------------------------------------------------------
def test_references_agree_with_naive_loops():
    # subgraph + csr_build of a small parent ladder
    ei, n, subset = L.parent_ladder(40, (0, 5, 17, 39), ((65, "all"), (3, "alt"), (64, "lane0"), (130, "last")), 150, seed=2)
    ref_ei, rowptr, colind, val, deg = L.ref_batch(ei, n, subset)
    naive_ei, _ = L.naive_subgraph(subset, ei, n, True)
    assert np.array_equal(ref_ei.numpy(), naive_ei)
    rp, ci, bits = L.naive_csr(naive_ei, 40)
    assert np.array_equal(rp, rowptr) and np.array_equal(ci, colind) and np.array_equal(bits, val.view(np.uint32))
    # the edge pass, both ways
    for pattern in L.EDGE_PATTERNS:
        ei, n, subset, keep = L.edge_pass_case(777, pattern, seed=4, n=60)
        for relabel in (False, True):
            out, kept = L.ref_subgraph(subset, ei, n, relabel)
            naive_out, naive_keep = L.naive_subgraph(subset, ei, n, relabel)
            assert np.array_equal(out.numpy(), naive_out) and np.array_equal(kept.numpy(), naive_keep)
    # csr_build / csr_transpose
    for ei, n in (L.csr_small(257, seed=1), L.csr_small(3, seed=1), L.csr_large(3000, seed=2, n=50, hub=500)):
        rowptr, colind, val, _ = O.csr_build(ei.numpy(), n)
        rp, ci, bits = L.naive_csr(ei.numpy(), n)
        assert np.array_equal(rp, rowptr) and np.array_equal(ci, colind) and np.array_equal(bits, val.view(np.uint32))
        t_rowptr, t_colind, t_val, _ = O.csr_transpose(ei.numpy(), n)
        rp, ci, bits = L.naive_csr(ei.numpy(), n, transposed=True)
        assert np.array_equal(rp, t_rowptr) and np.array_equal(ci, t_colind) and np.array_equal(bits, t_val.view(np.uint32))
    # prologue
    for name in ("all_loops", "single", "n256", "n257"):
        ei, n, undirected = L.prologue_case(name, seed=1)
        assert np.array_equal(L.ref_prologue(ei, n, undirected), L.naive_prologue(ei.numpy(), n, undirected))
    ei = torch.tensor([[4, 1, 1, 3, 3, 0], [4, 2, 2, 3, 1, 0]])
    assert np.array_equal(L.ref_prologue(ei, 5, False), L.naive_prologue(ei.numpy(), 5, False))
    # sampled batches
    src, dst, nn, ne = L.sampled_case([0, 3, 0, 7, 1], 9, seed=3)
    rowptr, colind, val, _ = L.ref_sampled(src, dst, nn, ne)
    rp, ci, bits = L.naive_csr(np.stack([src, dst]).astype(np.int64), nn)
    assert np.array_equal(rp, rowptr) and np.array_equal(ci, colind) and np.array_equal(bits, val.view(np.uint32))


def test_the_cpu_kernel_table_gives_the_same_arrays():
    """The ladder cases tests/cpu_kernels.py implements, through that table, against the references used on the GPU."""
    from tests.cpu_kernels import CpuKernels as C
    cases = [T.csr_inputs("n", n) for n in T.CSR_SMALL_N] + [T.csr_inputs("nnz", k) for k in T.CSR_LARGE_NNZ] + \
        [(e, T.symmetric_inputs()[3]) for e in T.symmetric_inputs()[:3]]
    for ei, n in cases:
        rowptr, colind, val, deg = O.csr_build(ei.numpy(), n)
        rp, ci, va, dg = C.csr_build(ei, n)
        assert np.array_equal(rp.numpy(), rowptr) and np.array_equal(ci.numpy(), colind) and np.array_equal(dg.numpy(), deg)
        assert ci.dtype == torch.int32 and np.array_equal(va.numpy().view(np.uint32), val.view(np.uint32))
        t_rowptr, t_colind, t_val, sym = O.csr_transpose(ei.numpy(), n)
        trp, tci, tva, flag = C.csr_transpose(ei, n, dg, rp, ci)
        assert np.array_equal(trp.numpy(), t_rowptr) and np.array_equal(tci.numpy(), t_colind) and flag is sym
        assert np.array_equal(tva.numpy().view(np.uint32), t_val.view(np.uint32))
    for nnz in T.EDGE_NNZ:
        for pattern in L.EDGE_PATTERNS:
            ei, n, subset, keep = T.edge_inputs(nnz, pattern)
            for relabel in (False, True):
                out, eid = C.subgraph(ei, n, subset, relabel, True)
                assert np.array_equal(out.numpy(), L.ref_subgraph(subset, ei, n, relabel)[0].numpy())
                assert np.array_equal(eid.numpy(), np.flatnonzero(keep))
    for key in ("rows",) + T.BATCH_SIZES:
        ei, n, subset = T.batch_inputs(key)[:3]
        out, _ = C.subgraph(ei, n, subset, True, False)
        got = C.csr_build(out, int(subset.numel()))
        for a, b in zip(got, T.batch_reference(key)[1:]):
            a = a.numpy()
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) if b.dtype == np.float32 else np.array_equal(a, b)
    for name in L.PROLOGUE_CASES:
        ei, n, undirected = T.prologue_inputs(name)
        assert np.array_equal(C.graph_prologue(ei, n, undirected, True, True).numpy(), L.ref_prologue(ei, n, undirected))


# ------------------------------------------------------------------------------------------------
# the CPU side of every GPU case
# ------------------------------------------------------------------------------------------------
def _timed(fn, *args):
    t0 = time.process_time()
    out = fn(*args)
    return out, time.process_time() - t0


def test_the_cpu_side_of_every_case_stays_within_budget():
    """Inputs + reference of every GPU case, built afresh (the undecorated builders): an accidentally quadratic reference or
    builder shows here, against the 0.1 - 0.2 s of the oracle alone on a million edges."""
    spent = {}
    for key in ("rows",) + T.BATCH_SIZES:
        (ei, n, subset, _, _), a = _timed(T.batch_inputs.__wrapped__, key)
        _, b = _timed(L.ref_batch, ei, n, subset)
        spent[f"batch-{key}"] = a + b
    for nnz in T.EDGE_NNZ:
        for pattern in L.EDGE_PATTERNS:
            (ei, n, subset, _), a = _timed(T.edge_inputs.__wrapped__, nnz, pattern)
            _, b = _timed(lambda: (L.ref_subgraph(subset, ei, n, False), L.ref_subgraph(subset, ei, n, True)))
            spent[f"edge-{nnz}-{pattern}"] = a + b
    for kind, sizes in (("n", T.CSR_SMALL_N), ("nnz", T.CSR_LARGE_NNZ)):
        for size in sizes:
            (ei, n), a = _timed(T.csr_inputs.__wrapped__, kind, size)
            _, b = _timed(lambda: (O.csr_build(ei.numpy(), n), O.csr_transpose(ei.numpy(), n)))
            spent[f"csr-{kind}{size}"] = a + b
    trio, a = _timed(T.symmetric_inputs.__wrapped__)
    for i, which in enumerate(("symmetric", "twin_late", "twin_last")):
        _, b = _timed(lambda: (O.csr_build(trio[i].numpy(), trio[3]), O.csr_transpose(trio[i].numpy(), trio[3])))
        spent[f"symmetry-{which}"] = a + b
    for name in L.PROLOGUE_CASES:
        (ei, n, undirected), a = _timed(T.prologue_inputs.__wrapped__, name)
        _, b = _timed(L.ref_prologue, ei, n, undirected)
        spent[f"prologue-{name}"] = a + b
    for case in T.SAMPLED_BUILD:
        (src, dst, nn, ne), a = _timed(T.sampled_inputs.__wrapped__, case[1], case[2])
        _, b = _timed(L.ref_sampled, src, dst, nn, ne)
        spent[f"sampled-{case[0]}"] = a + b
    for name in T.SAMPLED_TRANSPOSE:
        (ei, n), a = _timed(T.transpose_inputs.__wrapped__, name)
        _, b = _timed(lambda: (O.csr_build(ei.numpy(), n), O.csr_transpose(ei.numpy(), n)))
        spent[f"transpose-{name}"] = a + b
    worst = max(spent, key=spent.get)
    print("slowest CPU sides:", sorted(((round(v, 3), k) for k, v in spent.items()), reverse=True)[:6])
    assert spent[worst] <= BUDGET_SECONDS, (worst, spent[worst])
