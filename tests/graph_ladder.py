"""Inputs and references of the graph-construction ladder tests (tests/test_gpu_graph_ladder.py,
tests/test_graph_ladder_host.py): the integer kernels of csrc/csr.hip, csrc/subgraph.hip, csrc/subgraph_csr.hip,
csrc/prologue.hip and csrc/sampled_csr.hip at the places where their launch geometry turns over - the second grid lap,
the second 64-entry chunk of a row, a block's chunk edge, a key width at a power of two.  CPU only, plain numpy / torch.

Every comparison built on this module is array_equal on integers (and on the uint32 view of fp32 values); the references
are the numpy restatements of oracle/ (csr_build, csr_transpose, graph_prologue) and the mask-and-relabel restatement of
torch_geometric.utils.subgraph below.
"""
import numpy as np
import torch

from oracle import graph_oracle as G
from oracle import sgformer_oracle as O

# ------------------------------------------------------------------------------------------------
# launch geometry, restated (tests/test_graph_ladder_host.py parses the sources and asserts each of these)
# ------------------------------------------------------------------------------------------------
WAVE = 64                # csrc/common.h: constexpr int kWave = 64
NUM_CU = 256             # csrc/common.h: constexpr int kNumCU = 256
THREADS = 256            # constexpr int kThreads = 256 in each of the five files
# csrc/subgraph_csr.hip grid_rows: cap = kNumCU * 16 blocks; k_walk: one wave per row, kWavesPerBlock = kThreads / kWave
WALK_LAP = NUM_CU * 16 * (THREADS // WAVE)
# the same cap with one thread per row (k_mark, k_unmark, k_off32, k_values); csrc/sampled_csr.hip grid_for: kNumCU * 16
ROW_THREAD_LAP = NUM_CU * 16 * THREADS
# csrc/csr.hip and csrc/prologue.hip grid_for: cap = kNumCU * 8 blocks of kThreads
EDGE_LAP = NUM_CU * 8 * THREADS
SG_BLOCKS = 2048         # csrc/subgraph.hip: constexpr int kBlocks = 2048
MAX_FANOUT = 256         # csrc/sampled_csr.hip: constexpr int kMaxFanout = 256

assert (WALK_LAP, ROW_THREAD_LAP, EDGE_LAP) == (16384, 1048576, 524288)


def sg_chunk(nnz):
    """chunk_of (csrc/subgraph.hip): the edges one block owns - ceil(nnz / kBlocks) rounded up to kThreads."""
    c = (nnz + SG_BLOCKS - 1) // SG_BLOCKS
    return (c + THREADS - 1) // THREADS * THREADS


def key_bits(n):
    """key_bits (csrc/csr.hip): the sorted bits of a (target << 32 | source) key; 32 + bits_for(n) in csrc/prologue.hip."""
    b = 1
    while (1 << b) < n and b < 31:
        b += 1
    return 32 + b


def sort_bits(m):
    """The `bits` loop of sgf_subgraph_csr_emit: the sorted bits of a local id; source_bits in csrc/sampled_csr.hip."""
    b = 1
    while (1 << b) < m:
        b += 1
    return b


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------
def ref_subgraph(subset, ei, n, relabel):
    """torch_geometric.utils.subgraph (PyG 1.7.2): node mask, edge mask, optional relabel; the original edge order."""
    mask_n = torch.zeros(n, dtype=torch.bool)
    mask_n[subset] = True
    keep = mask_n[ei[0]] & mask_n[ei[1]]
    out = ei[:, keep]
    if relabel:
        idx = torch.zeros(n, dtype=torch.int64)
        idx[subset] = torch.arange(subset.numel())
        out = idx[out]
    return out, keep


def ref_batch(ei, n, subset):
    """What sgf_subgraph_csr_* must return for a batch: (induced edge list, relabelled; its rowptr, colind, val, deg)."""
    ref_ei, _ = ref_subgraph(subset, ei, n, True)
    return (ref_ei,) + tuple(O.csr_build(ref_ei.numpy(), int(subset.numel())))


def ref_sampled(e_src, e_dst, nn, ne):
    """sgf_sampled_csr_build's contract (include/sgf.h): csr_build of the first ne edges on nn nodes."""
    return O.csr_build(np.stack([np.asarray(e_src[:ne], dtype=np.int64), np.asarray(e_dst[:ne], dtype=np.int64)]), nn)


def naive_subgraph(subset, ei, n, relabel):
    """ref_subgraph edge by edge."""
    local = {int(v): j for j, v in enumerate(subset.tolist())}
    out, keep = [], []
    for s, t in zip(ei[0].tolist(), ei[1].tolist()):
        k = s in local and t in local
        keep.append(k)
        if k:
            out.append((local[s], local[t]) if relabel else (s, t))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2).T, np.asarray(keep, dtype=bool)


def naive_csr(ei, n, transposed=False):
    """O.csr_build / O.csr_transpose edge by edge: (rowptr, colind, val bits) with Python's sort and one fp32 op at a time."""
    pairs = list(zip(ei[0].tolist(), ei[1].tolist()))
    deg = [0] * n
    for _, t in pairs:
        deg[t] += 1
    order = sorted(pairs, key=(lambda p: (p[0], p[1])) if transposed else (lambda p: (p[1], p[0])))
    rows = [0] * n
    for s, t in pairs:
        rows[s if transposed else t] += 1
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(rows)
    one = np.float32(1.0)
    with np.errstate(divide="ignore"):
        val = [np.sqrt(one / np.float32(deg[t])) * np.sqrt(one / np.float32(deg[s])) for s, t in order]
    val = np.asarray([v if np.isfinite(v) else np.float32(0.0) for v in val], dtype=np.float32)
    colind = np.asarray([(t if transposed else s) for s, t in order], dtype=np.int64)
    return rowptr, colind, val.view(np.uint32)


def naive_prologue(ei, n, undirected):
    """G.graph_prologue edge by edge."""
    pairs = list(zip(ei[0].tolist(), ei[1].tolist()))
    if undirected:
        pairs = sorted(set(pairs) | {(c, r) for r, c in pairs})
    pairs = [p for p in pairs if p[0] != p[1]] + [(i, i) for i in range(n)]
    return np.asarray(pairs, dtype=np.int64).reshape(-1, 2).T


# ------------------------------------------------------------------------------------------------
# subgraph_csr: the parent ladder
# ------------------------------------------------------------------------------------------------
ROW_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 1023, 1024, 1025, 4097)
PATTERNS = ("all", "none", "lane0", "lane63", "alt", "last", "first", "half")
ALL_ROWS = tuple((L, p) for L in ROW_LENGTHS for p in PATTERNS)
ZONE = 2100              # members in the alternating id zone [0, 2 ZONE): enough for a 4097-entry row kept every other entry


def keep_mask(L, pattern):
    """Which stored entries of a parent row of length L (ascending source order, as k_walk reads it) are in the batch."""
    i = np.arange(L)
    if pattern == "all":
        return np.ones(L, dtype=bool)
    if pattern == "none":
        return np.zeros(L, dtype=bool)
    if pattern == "lane0":
        return i % WAVE == 0
    if pattern == "lane63":
        return i % WAVE == WAVE - 1
    if pattern == "alt":
        return i % 2 == 0
    if pattern == "last":                                    # every earlier chunk contributes zero to the carried total
        return i >= (max(L - 1, 0) // WAVE) * WAVE
    if pattern == "first":
        return i < WAVE
    if pattern == "half":
        return np.random.RandomState(7919 * L + 13).rand(L) < 0.5
    raise ValueError(pattern)


def runs_of(mask):
    return 0 if mask.size == 0 else 1 + int(np.count_nonzero(mask[1:] != mask[:-1]))


def row_fits(L, pattern, m):
    """Whether the id zone of a batch of m nodes can hold this row (each run of equal membership needs an id of its own)."""
    mask = keep_mask(L, pattern)
    zk = min(m, ZONE)
    return runs_of(mask) + (0 if mask.size == 0 or mask[0] else 1) <= 2 * zk


def _row_sources(mask, zk, rng):
    """L source ids whose ASCENDING order has the membership `mask`: run r of equal membership draws (with repeats: stored
    duplicates, both copies kept or both dropped) from its own window of the zone, where even ids are members."""
    L = mask.size
    if L == 0:
        return np.zeros(0, dtype=np.int64)
    starts = np.concatenate([[0], np.flatnonzero(mask[1:] != mask[:-1]) + 1])
    lens = np.diff(np.concatenate([starts, [L]]))
    R = starts.size
    run = np.repeat(np.arange(R), lens)
    w = (2 * zk) // R
    if w >= 2:
        w -= w % 2
        ids = run * w + 2 * rng.randint(0, w // 2, size=L) + (~mask)
    else:
        off = 0 if mask[0] else 1                            # ids r + off: their parity alternates with the runs
        if R + off > 2 * zk:
            raise ValueError(f"a row of {R} runs does not fit a zone of {2 * zk} ids")
        ids = run + off
    return ids.astype(np.int64)


def parent_ladder(m, positions, rows=ALL_ROWS, n_min=0, seed=0):
    """(edge_index int64 [2, E], n, subset int64 [m]) of a parent graph and a batch of it.

    subset[positions[i]] is a PROBE node: its parent in-neighbour list (the row k_walk reads, ascending source ids) has
    rows[i] = (length, keep pattern) - exactly keep_mask(length, pattern) of its stored sources are in the batch.  Rows hold
    stored duplicates (both copies kept, or both dropped) and, where the pattern keeps anything, the probe's own self-loop.
    Node ids: [0, 2 zk) alternate member / non-member (zk = min(m, ZONE)), the other members follow three to every
    non-member, the rest up to n is outside the batch.  The subset is a seeded permutation of the members, so local-id
    order is not global-id order.  One more row (a filler's) holds the nodes of local ids 0, 1, 2^k and m - 1 together,
    2^k the largest power of two below m.  Every other node sits on a sparse ring: one in-edge from its id successor, a
    second from a random node for four in ten - kept or not as membership falls.  The edge list is shuffled."""
    assert m >= 1 and len(rows) == len(positions) == len(set(positions)) and all(0 <= p < m for p in positions)
    rng = np.random.RandomState(seed)
    zk = min(m, ZONE)
    rest = m - zk
    tail = (rest // 3) * 4 + rest % 3
    n = max(int(n_min), 2 * zk + tail + 2)
    member = np.zeros(n, dtype=bool)
    member[0:2 * zk:2] = True
    member[2 * zk:2 * zk + tail] = np.arange(tail) % 4 != 3
    assert int(member.sum()) == m
    is_probe = np.zeros(n, dtype=bool)
    src, dst, probes = [], [], []
    for L, pattern in rows:
        mask = keep_mask(L, pattern)
        ids = _row_sources(mask, zk, rng)
        probe = -1
        for at in rng.permutation(np.flatnonzero(mask))[:64]:   # the target is one of its own kept sources: a self-loop
            if not is_probe[ids[at]]:
                probe = int(ids[at])
                break
        if probe < 0:                                        # nothing kept (or every candidate taken): any free member
            free = np.flatnonzero(member & ~is_probe)
            probe = int(free[rng.randint(free.size)])
        is_probe[probe] = True
        probes.append(probe)
        src.append(ids)
        dst.append(np.full(L, probe, dtype=np.int64))
    others = rng.permutation(np.flatnonzero(member & ~is_probe))
    subset = np.full(m, -1, dtype=np.int64)
    subset[np.asarray(positions, dtype=np.int64)] = probes
    subset[subset < 0] = others
    if others.size:                                          # local ids 0, 1, 2^k and m - 1 in one row
        corner = sorted({0, min(1, m - 1), 1 << (sort_bits(m) - 1) if m > 1 else 0, m - 1})
        corner = [c for c in corner if c < m]
        src.append(subset[corner])
        dst.append(np.full(len(corner), others[0], dtype=np.int64))
    v = np.flatnonzero(~is_probe)
    src.append((v + 1) % n)
    dst.append(v)
    second = v[rng.rand(v.size) < 0.4]
    src.append(rng.randint(0, n, size=second.size).astype(np.int64))
    dst.append(second)
    ei = np.stack([np.concatenate(src), np.concatenate(dst)])
    ei = ei[:, rng.permutation(ei.shape[1])]
    return torch.from_numpy(ei), n, torch.from_numpy(subset)


def lap_positions(m):
    """The local positions at which the batch-size ladder puts its probes: both sides of every lap a batch of m rows reaches."""
    want = [0, WALK_LAP - 1, WALK_LAP, WALK_LAP + 1, 2 * WALK_LAP - 1, 2 * WALK_LAP, ROW_THREAD_LAP - 1, ROW_THREAD_LAP,
            ROW_THREAD_LAP + 1, m - 1]
    return sorted({p for p in want if 0 <= p < m})


# rows of the batch-size ladder, by priority: those a batch of m nodes can hold are dealt to its probe positions in turn
LADDER_ROWS = ((65, "all"), (129, "lane63"), (193, "last"), (1025, "half"), (64, "lane0"), (128, "alt"), (4097, "first"),
               (2, "all"), (256, "none"), (1024, "all"))


def batch_rows(m, count):
    fit = [r for r in LADDER_ROWS if row_fits(r[0], r[1], m)]
    return tuple(fit[i % len(fit)] for i in range(count))


# ------------------------------------------------------------------------------------------------
# subgraph.hip: the edge pass
# ------------------------------------------------------------------------------------------------
EDGE_PATTERNS = ("all", "none", "chunk_ends", "lane0", "lane63", "final_block")


def edge_keep(nnz, pattern):
    e, c = np.arange(nnz), sg_chunk(nnz)
    if pattern == "all":
        return np.ones(nnz, dtype=bool)
    if pattern == "none":
        return np.zeros(nnz, dtype=bool)
    if pattern == "chunk_ends":                              # the last edge of each block's chunk and the first of the next
        return (e % c == c - 1) | (e % c == 0)
    if pattern == "lane0":
        return e % WAVE == 0
    if pattern == "lane63":
        return e % WAVE == WAVE - 1
    if pattern == "final_block":                             # only the last block that owns any edge, its partial chunk
        return e >= (nnz - 1) // c * c
    raise ValueError(pattern)


def edge_pass_case(nnz, pattern, seed=0, n=1000):
    """(edge_index [2, nnz], n, subset, keep [nnz]): edge e survives the subset iff keep[e] = edge_keep(nnz, pattern)[e];
    dropped edges turn through the three kinds (source outside, target outside, both outside) by position."""
    rng = np.random.RandomState(seed)
    perm = rng.permutation(n)
    ins, outs = perm[:n // 2], perm[n // 2:]
    keep = edge_keep(nnz, pattern)
    kind = np.arange(nnz) % 3
    a, b = ins[rng.randint(0, ins.size, nnz)], ins[rng.randint(0, ins.size, nnz)]
    x, y = outs[rng.randint(0, outs.size, nnz)], outs[rng.randint(0, outs.size, nnz)]
    src = np.where(keep | (kind == 1), a, x)
    dst = np.where(keep | (kind == 0), b, y)
    return torch.from_numpy(np.stack([src, dst]).astype(np.int64)), n, torch.from_numpy(ins.astype(np.int64)), keep


# ------------------------------------------------------------------------------------------------
# csr.hip
# ------------------------------------------------------------------------------------------------
def csr_small(n, seed=0):
    """A graph on n nodes with edges out of and into node n - 1 (the top of the key range) and, where they are other nodes,
    0 and n - 2 isolated."""
    rng = np.random.RandomState(seed)
    allowed = np.union1d(np.setdiff1d(np.arange(n, dtype=np.int64), [0, n - 2]), [n - 1])
    k = min(4 * n, 6000)
    src, dst = allowed[rng.randint(0, allowed.size, k)], allowed[rng.randint(0, allowed.size, k)]
    top = np.full(3, n - 1, dtype=np.int64)
    other = allowed[rng.randint(0, allowed.size, 3)]
    src = np.concatenate([src, top, other, [n - 1]])
    dst = np.concatenate([dst, other, top, [n - 1]])
    p = rng.permutation(src.size)
    return torch.from_numpy(np.stack([src[p], dst[p]])), n


def csr_large(nnz, seed=0, n=65537, hub=100000):
    """nnz edges on n nodes, `hub` of them into one node (a row with stored duplicates: hub > n), shuffled."""
    rng = np.random.RandomState(seed)
    src = rng.randint(0, n, nnz).astype(np.int64)
    dst = rng.randint(0, n, nnz).astype(np.int64)
    dst[:hub] = n // 2
    src[hub - 1], dst[nnz - 1] = n - 1, n - 1
    p = rng.permutation(nnz)
    return torch.from_numpy(np.stack([src[p], dst[p]])), n


def symmetric_trio(seed=0, n=50000, pairs=300000):
    """(symmetric graph, twin_late, twin_last, n).  The symmetric graph stores both directions of `pairs` random pairs
    (> EDGE_LAP entries).  twin_late adds a directed 3-cycle among three of the last nodes: in- and out-degrees stay
    equal, so rowptr and its transpose agree and A differs from A^T in stored columns behind position EDGE_LAP only.
    twin_last replaces the source of the very last stored entry."""
    rng = np.random.RandomState(seed)
    a, b = rng.randint(0, n, pairs).astype(np.int64), rng.randint(0, n, pairs).astype(np.int64)
    x, y, z = n - 30, n - 20, n - 10
    tri = np.isin(a, (x, y, z)) & np.isin(b, (x, y, z))
    a, b = a[~tri], b[~tri]
    a, b = np.concatenate([a, [n - 1]]), np.concatenate([b, [n - 2]])     # the last row is not empty
    sym = np.stack([np.concatenate([a, b]), np.concatenate([b, a])])
    late = np.concatenate([sym, np.asarray([[x, y, z], [y, z, x]], dtype=np.int64)], axis=1)
    last = sym.copy()
    in_last = np.flatnonzero(sym[1] == n - 1)
    at = in_last[np.argmax(sym[0][in_last])]                 # the largest source of the last row: the last stored entry
    last[0, at] = n - 1                                      # ... becomes a self-loop (n - 1 > n - 2, the old largest)
    return tuple(torch.from_numpy(e) for e in (sym, late, last)) + (n,)


def first_difference(u, v):
    """First position at which two arrays differ (their common length when one is a prefix of the other; -1 when equal)."""
    k = min(u.size, v.size)
    d = np.flatnonzero(u[:k] != v[:k])
    return int(d[0]) if d.size else (-1 if u.size == v.size else k)


# ------------------------------------------------------------------------------------------------
# prologue.hip
# ------------------------------------------------------------------------------------------------
PROLOGUE_CASES = ("one_edge", "straddle", "all_loops", "single", "n256", "n257", "n65536", "n65537", "directed_loops")


def prologue_case(name, seed=0):
    """(edge_index, n, undirected) of the named case."""
    rng = np.random.RandomState(seed)
    if name == "one_edge":                                   # m copies of one edge: collapses to it and its reverse
        m = EDGE_LAP + 3
        return torch.tensor([[5], [2]]).expand(2, m).contiguous(), 9, True
    if name == "straddle":
        # distinct (low, high) edges: the sorted symmetrised keys start with all of them in (row, col) order; the edge of rank
        # EDGE_LAP - 500 is stored 1000 more times, so its run of equal keys lies across sorted position EDGE_LAP
        lo, hi, m0 = 40000, 40000, EDGE_LAP + 5000
        key = np.unique(rng.randint(0, lo * hi, size=m0 + 4000).astype(np.int64))
        key = key[rng.permutation(key.size)[:m0]]
        r, c = key // hi, lo + key % hi
        at = np.argsort(key)[EDGE_LAP - 500]
        r, c = np.concatenate([r, np.full(1000, r[at])]), np.concatenate([c, np.full(1000, c[at])])
        p = rng.permutation(r.size)
        return torch.from_numpy(np.stack([r[p], c[p]])), lo + hi, True
    if name == "all_loops":
        v = rng.randint(0, 300, 5000).astype(np.int64)
        return torch.from_numpy(np.stack([v, v])), 300, True
    if name == "single":
        return torch.tensor([[3], [1]]), 4, True
    if name.startswith("n"):
        n = int(name[1:])
        src, dst = rng.randint(0, n, 4000).astype(np.int64), rng.randint(0, n, 4000).astype(np.int64)
        src[0], dst[0] = n - 1, 0
        src[1], dst[1] = n - 1, n - 2
        return torch.from_numpy(np.stack([src, dst])), n, True
    if name == "directed_loops":                             # self-loops at the first and the last input position
        m = EDGE_LAP + 7
        src, dst = rng.randint(0, 5000, m).astype(np.int64), rng.randint(0, 5000, m).astype(np.int64)
        dst[0], dst[m - 1], dst[EDGE_LAP] = src[0], src[m - 1], src[EDGE_LAP]
        return torch.from_numpy(np.stack([src, dst])), 5000, False
    raise ValueError(name)


def ref_prologue(ei, n, undirected):
    return G.graph_prologue(ei.numpy(), n, undirected=undirected)


def sorted_keys(ei):
    """The sorted (row << 32 | col) keys of the symmetrised input: what k_pro_flags walks."""
    r, c = ei[0].numpy(), ei[1].numpy()
    return np.sort(np.concatenate([(r << 32) | c, (c << 32) | r]))


# ------------------------------------------------------------------------------------------------
# sampled_csr.hip
# ------------------------------------------------------------------------------------------------
def sampled_case(lens, nn, seed=0, one_source=False):
    """(edge_src_local int32 [ne], edge_dst_local int32 [ne], nn, ne) shaped like a sampler's batch: node j < len(lens) is
    the target of lens[j] consecutive edges (targets non-decreasing), nodes behind have no in-edge; sources are random
    nodes of the batch, or - one_source - one node per row, repeated."""
    lens = np.asarray(lens, dtype=np.int64)
    assert lens.size <= nn
    rng = np.random.RandomState(seed)
    dst = np.repeat(np.arange(lens.size), lens)
    if one_source:
        src = np.repeat(rng.randint(0, nn, lens.size), lens)
    else:
        src = rng.randint(0, nn, dst.size)
        if src.size:
            src[rng.randint(0, src.size, 3)] = nn - 1
    return src.astype(np.int32), dst.astype(np.int32), int(nn), int(dst.size)


def sampled_rows(name):
    """Row lengths and node count of the named build case."""
    if name == "ladder":                                     # 0, 1, 2, 255 and 256 entries, empty rows first and last
        lens = [0, 0, 1, 2, 255, 0, 256, 1, 256, 255, 2, 0, 256, 0]
        return lens, len(lens) + 40
    if name == "over":                                       # rows past the 256-entry bound: advisory inside the kernels
        return [3, 257, 0, 300, 256, 1, 257], 60
    if name == "lap":                                        # past the 1 048 576-thread lap, rows of at most 4 entries
        ne = ROW_THREAD_LAP + 300
        lens = np.tile(np.asarray([4, 0, 3, 1, 2, 4, 4, 2], dtype=np.int64), ne // 20 + 1)
        cut = int(np.searchsorted(np.cumsum(lens), ne))
        lens = lens[:cut + 1].copy()
        lens[cut] -= int(lens.sum()) - ne
        return lens, lens.size + 1000
    raise ValueError(name)


def transpose_case(name, seed=0):
    """(edge_index, n) of a graph whose forward CSR sgf_sampled_csr_transpose takes."""
    rng = np.random.RandomState(seed)
    if name == "n1":
        return torch.zeros((2, 5), dtype=torch.int64), 1
    if name in ("n256", "n257"):                             # source n - 1 present; rows 0-2 and n-3.. empty in both orientations
        n = int(name[1:])
        k = 3000
        src, dst = rng.randint(3, n - 3, k).astype(np.int64), rng.randint(3, n - 3, k).astype(np.int64)
        src[:4] = n - 1
        return torch.from_numpy(np.stack([src, dst])), n
    if name == "lap":                                        # nnz past the 1 048 576-thread lap
        n, k = 300001, ROW_THREAD_LAP + 300
        src, dst = rng.randint(5, n, k).astype(np.int64), rng.randint(5, n - 7, k).astype(np.int64)
        src[0] = n - 1
        return torch.from_numpy(np.stack([src, dst])), n
    raise ValueError(name)
