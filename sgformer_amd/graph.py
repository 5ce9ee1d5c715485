"""The graph side of the autograd-level operators (split out of ops.py in r06): the cached CSR of an edge list (T1,
large/ours.py:26-33), its locality-restoring node order and tile / row-block plans, and T2 — the sum-reduce SpMM with its
A^T backward (large/ours.py:34) on whichever kernel family the graph's structure selects.  `ops` re-exports every name."""
from __future__ import annotations

import dataclasses
import os
from collections import OrderedDict
from typing import Optional

import torch

from . import _lib
from . import coded as _coded
from .kernels import HipKernels, LONG_ROW, _SEGMENT

_F32 = torch.float32


K = _coded.install(HipKernels())


def _has(table, name: str, *args) -> bool:
    """The kernel table has the method `name` — and, given arguments, answers them with yes (the *_supported queries).
    hasattr is the rule on purpose: the CPU table of the tests lacks methods."""
    fn = getattr(table, name, None)
    return fn is not None and (not args or bool(fn(*args)))


def _env(name: str, default: str = "") -> str:     # SGF_SPMM_* / SGF_REORDER as set NOW, never kept: tests flip them between calls
    return os.environ.get(name, default)


# Graphs with fewer stored entries than this are per-batch graphs (mini-batch trainers build one per step): their
# long-row segment count is not read back from the device (a host sync per batch) but bounded from nnz alone.
SMALL_GRAPH_NNZ = 1 << 23


def long_row_segments(rowptr: torch.Tensor, nnz: Optional[int] = None, max_row_len: Optional[int] = None) -> int:
    """sum over rows longer than LONG_ROW of ceil(len / segment): the `long_segments` argument of
    sgf_spmm_split.  One tiny device reduction + host read per CSR (done once, when it is built) — or, for
    small graphs whose nnz is known on the host, the bound  sum ceil(len/seg) <= nnz/seg + nnz/(LONG_ROW+1)
    without any device read (0 when no row can be long at all).  `max_row_len`: a bound on the longest row the caller
    GUARANTEES without looking (a sampled batch: its largest fan-out; NOT the node count — duplicate edges are kept) — at most LONG_ROW means no
    split path at all (no memset, no extra launches) for that CSR."""
    if rowptr.numel() <= 1:
        return 0
    if max_row_len is not None and max_row_len <= LONG_ROW:
        return 0
    if nnz is not None and nnz < SMALL_GRAPH_NNZ:
        return 0 if nnz <= LONG_ROW else nnz // _SEGMENT + nnz // (LONG_ROW + 1) + 1
    lens = rowptr[1:] - rowptr[:-1]
    segs = torch.where(lens > LONG_ROW, (lens + (_SEGMENT - 1)) // _SEGMENT, torch.zeros_like(lens))
    return int(segs.sum())


@dataclasses.dataclass(slots=True)
class EdgeHints:
    """Promises of the producer of an `edge_index` (batching.subgraph, sampling.NeighborSampler, dist.Repartition), stored
    under ONE attribute of the tensor: the reference trainers hand the tensor through code that stays unchanged."""
    trusted: bool = False                    # ids are in range by construction: no range check (a host sync) in CSRGraph
    max_in_degree: Optional[int] = None      # longest CSR row, as a bound the producer GUARANTEES (a sampler's largest fan-out)
    csr: Optional[tuple] = None              # (rowptr, colind, val, deg) built with the edge list: sgf_csr_build's arrays, bit for bit
    csr_t_lazy: bool = False                 # `csr` is directed, rows in ascending source order: sgf_sampled_csr_transpose serves A^T
    symmetric: bool = False                  # A^T == A by construction (an induced subgraph of a parent verified once)
    sharded_graph: object = None             # the dist.ShardedGraph of this (re-partitioned) list

    def attach(self, edge_index: torch.Tensor) -> torch.Tensor:
        edge_index._sgf_hints = self
        return edge_index

    def to(self, device) -> "EdgeHints":        # for a copy of the edge list on `device`: the CSR moves with it, a sharded graph does not
        csr = None if self.csr is None else tuple(t.to(device) for t in self.csr)
        return dataclasses.replace(self, csr=csr, sharded_graph=None)


_NO_HINTS = EdgeHints()


def hints_of(edge_index) -> EdgeHints:      # the record an edge list carries, or the shared all-default one (read only)
    return getattr(edge_index, "_sgf_hints", _NO_HINTS)


# ------------------------------------------------------------------------------------------------
# T1: cached CSR of the normalised adjacency (large/ours.py:26-33)
# ------------------------------------------------------------------------------------------------
class GraphOperand:
    """What spmm / spmm_on / _sharded_spmm read off a graph — the whole interface, with its defaults.  A subclass sets n, nnz,
    device, rowptr / colind / val, long_segments / t_long_segments and `symmetric`, and implements transposed().  The flags are
    plain attributes: GraphView.decide and dist.Repartition assign them from outside.  transposed() -> (rowptr, colind, val) of A^T."""
    blocked = False          # multiply with the LDS-staged row-block plan (GraphView)
    tiled = False            # ... with the matrix-core tile plan (GraphView)
    locality = False         # the gathers mostly hit in L2 (a re-ordered graph): sgf_spmm_stream
    comm_local = None        # int32 [n_local] community of every local row (dist.Repartition): row blocks of the own-block tile plan
    blk_row = None           # int32 [nb + 1] row blocks that follow the communities (GraphView)
    tile_min_count = None    # TilePlan's min_count when not the default (GraphView)
    n_local = None           # rows of a node-sharded row block
    symmetric: Optional[bool] = None
    _t_lazy = False          # the edge list came with a sampled batch's CSR (sgf_sampled_csr_*)

    def __init__(self):
        self._plans, self._tile_plans, self._halo, self._view, self.forward_calls = {}, {}, {}, None, 0

    def _stored(self, transposed: bool) -> bool:
        """The orientation whose arrays serve A (False) or A^T (True): A^T of a symmetric graph is A."""
        if transposed:
            self.transposed()                  # (settles `symmetric` where it is not known yet)
        return bool(transposed) and not self.symmetric

    def arrays(self, transposed: bool = False):
        """(rowptr, colind, val, long_segments) of A, or of A^T."""
        if self._stored(transposed):
            return (*self.transposed(), self.t_long_segments)
        return self.rowptr, self.colind, self.val, self.long_segments

    def plan(self, dtype, transposed: bool = False):      # BlockedPlan for `dtype` storage on A (or A^T), or None
        return None

    def halo(self, shard, transposed: bool):              # dist.HaloPlan of a node-sharded row block, or None: all-gather
        return None

    def view(self, now: bool = False) -> "GraphView":     # how the model should run on this graph: as it is
        return GraphView(self, None, None)


class CSRGraph(GraphOperand):
    """rowptr/colind/val of A = D^-1/2 (edge_index^T) D^-1/2 on the GPU, built by sgf_csr_build.

    The reference rebuilds this (degree + argsort over nnz) in every layer of every forward;
    here it is built once per `edge_index` and reused by all layers and by the backward.
    """

    def __init__(self, edge_index: torch.Tensor, num_nodes: int, validate: bool = True):
        super().__init__()
        K.check(edge_index)
        if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
            raise ValueError("edge_index must be an int64 tensor of shape [2, nnz]")
        if num_nodes >= 2 ** 31:
            raise ValueError("num_nodes must be < 2^31 (int32 column indices)")
        ei = edge_index.contiguous()
        n = int(num_nodes)
        hints = hints_of(edge_index)
        if validate and not hints.trusted and ei.shape[1] > 0:
            lo, hi = torch.aminmax(ei)
            if int(lo) < 0 or int(hi) >= n:
                raise IndexError(f"edge_index has node ids outside [0, {n})")
        self.n, self.nnz, self.device = n, int(ei.shape[1]), ei.device
        self.edge_index = ei
        pre = hints.csr
        if pre is not None and pre[0].numel() == n + 1 and pre[1].numel() == self.nnz:
            # built by the producer in its own pass (batching.subgraph: sgf_subgraph_csr_*, sampling.NeighborSampler:
            # sgf_sampled_csr_build) — bit for bit what sgf_csr_build would return for this list (tests/test_gpu_r05.py)
            self.rowptr, self.colind, self.val, self.deg = pre
            self._t_lazy = bool(hints.csr_t_lazy)
        else:
            self.rowptr, self.colind, self.val, self.deg = K.csr_build(ei, n)
        # The node count is no bound on a row: sgf_csr_build keeps duplicate edges (large/ours.py:33 does not coalesce; ADVICE
        # r04) — without the producer's the nnz-based bound (small graphs) or the exact count from rowptr applies.
        self.long_segments = long_row_segments(self.rowptr, self.nnz, hints.max_in_degree)
        self.t_long_segments = 0
        self._t = None  # (rowptr, colind, val) of A^T, built on first backward
        if hints.symmetric:         # no second sort, no comparison pass and no host read per batch in the first backward
            self.symmetric, self._t, self.t_long_segments = True, (self.rowptr, self.colind, self.val), self.long_segments

    def transposed(self):
        """CSR of A^T for dX = A^T dY; the same arrays when A is symmetric."""
        if self._t is None and self._t_lazy:
            # no second sort of the edge list, no comparison pass, no host read in the middle of the backward: `symmetric` is
            # set without looking (were the batch graph symmetric, these arrays would equal the forward ones)
            self._t = K.sampled_csr_transpose(self.rowptr, self.colind, self.val, self.n)
            self.symmetric = False
            self.t_long_segments = long_row_segments(self._t[0], self.nnz)
        if self._t is None:
            t_rowptr, t_colind, t_val, sym = K.csr_transpose(self.edge_index, self.n, self.deg,
                                                             self.rowptr, self.colind)
            self.symmetric = sym
            self._t = (self.rowptr, self.colind, self.val) if sym else (t_rowptr, t_colind, t_val)
            self.t_long_segments = self.long_segments if sym else long_row_segments(t_rowptr, self.nnz)
        return self._t

    def plan(self, dtype, transposed: bool = False):
        """LDS-staged row-block SpMM: one BlockedPlan per (orientation, storage dtype) while `blocked` is set."""
        if not self.blocked:
            return None
        key = (self._stored(transposed), dtype)
        if key not in self._plans:
            self._plans[key] = BlockedPlan(*self.arrays(key[0])[:3], self.n, dtype)
        return self._plans[key]

    def tile_plan(self, transposed: bool = False):
        """Dense matrix-core tiles + gather remainder (sgf_spmm_tile): one TilePlan per orientation, on `blk_row`."""
        key = self._stored(transposed)
        if key not in self._tile_plans:
            self._tile_plans[key] = TilePlan(*self.arrays(key)[:3], self.n, self.blk_row, min_count=self.tile_min_count)
        return self._tile_plans[key]

    def view(self, now: bool = False) -> "GraphView":
        """How the model should run on this graph: the graph itself, or a re-ordered copy + the row
        permutation to apply at the module boundary (decided once; see GraphView).  now=True: decide
        at this call instead of waiting for the second forward."""
        self.forward_calls += 1
        if self._view is None:
            self._view = GraphView.decide(self, now)       # (None: undecided until the second forward)
        return self._view if self._view is not None else GraphView(self, None, None)


class WeightedCSRGraph(GraphOperand):
    """CSR of A[target, source] = value_e with EXPLICIT per-edge values — the edge-weighted variants of the
    medium recipes: GCNConv(x, edge_index, edge_weight) (medium/models.py:55-62, gcn_norm with weights) and
    DIFFormer's gcn_conv (medium/difformer.py:63-79, value = edge_weight * d_in * d_out).  The caller computes
    the values (one elementwise expression); entries are ordered by (target, source) like sgf_csr_build's, the
    transpose by (source, target).  No gradient flows to the values (edge weights are data, not parameters).
    A GraphOperand without plans or views: the plain kernels."""

    def __init__(self, edge_index: torch.Tensor, values: torch.Tensor, num_nodes: int):
        super().__init__()
        K.check(edge_index, values)
        n = int(num_nodes)
        self.n, self.nnz, self.device = n, int(edge_index.shape[1]), edge_index.device
        self._src, self._tgt = edge_index[0].contiguous(), edge_index[1].contiguous()
        self._values = values.detach().to(_F32).contiguous()
        self.rowptr, self.colind, self.val = self._sorted(self._tgt, self._src)
        self.long_segments = long_row_segments(self.rowptr, self.nnz)
        self._t, self.t_long_segments, self.symmetric = None, 0, False

    def _sorted(self, rows, cols):
        perm = torch.argsort(rows * self.n + cols, stable=True)
        counts = torch.bincount(rows, minlength=self.n)
        rowptr = torch.zeros(self.n + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(counts, 0, out=rowptr[1:])
        return rowptr, cols[perm].to(torch.int32), self._values[perm]

    def transposed(self):
        if self._t is None:
            self._t = self._sorted(self._src, self._tgt)
            self.t_long_segments = long_row_segments(self._t[0], self.nnz)
        return self._t


def weighted_graph(edge_index: torch.Tensor, edge_weight: torch.Tensor, num_nodes: int, value_fn, tag: str):
    """Cached WeightedCSRGraph; `value_fn(edge_index, edge_weight, n)` -> (edge_index', values) builds the
    normalised values once per (edge_index, edge_weight) pair."""
    key_tag = (tag, edge_weight.data_ptr(), edge_weight._version, tuple(edge_weight.shape))

    def build(ei, n):
        ei2, vals = value_fn(ei, edge_weight, n)
        g = WeightedCSRGraph(ei2, vals, n)
        g.edge_weight_ref = edge_weight          # pins the key tensor, like graph_cache pins edge_index
        return g

    return graph_cache.get(edge_index, num_nodes, factory=build, tag=key_tag)


# SGF_SPMM_BLOCK = "rows_per_block,lds_rows" overrides the block shape (default: 128 rows, all 144 KiB of LDS)
def _block_shape(dtype):
    cap = K.lds_rows_max(dtype)
    env = _env("SGF_SPMM_BLOCK")
    if env:
        r, c = (int(t) for t in env.split(","))
        return r, min(c, cap)
    return 128, cap


class BlockedPlan:
    """Row-block plan of one CSR (sgf_spmm_plan): which neighbour rows each block of rows stages in
    LDS, and the entry codes / values re-ordered so that the LDS entries lead every row."""

    def __init__(self, rowptr, colind, val, n: int, dtype, rows_per_block=None, lds_rows=None):
        r, c = _block_shape(dtype)
        self.rows_per_block = int(rows_per_block or r)
        self.lds_rows = int(lds_rows or c)
        (self.ecode, self.eval, self.nlds, self.sh_ptr, self.sh_cols, st) = K.spmm_plan(
            rowptr, colind, val, n, self.rows_per_block, self.lds_rows, LONG_ROW)
        self.lds_entries, self.staged_rows, self.unique_pairs, self.nnz = st
        self.lds_fraction = self.lds_entries / max(self.nnz, 1)


# Tile plan parameters: at most TILE_CAP staged sources per block (whole 32-source chunks), a source is staged when at
# least TILE_MIN_COUNT of the block's entries reference it (a staged source costs one 512-byte row of X plus one
# 512-byte tile column per block, a gathered entry 520 bytes each time; measured at ogbn-products scale: 2 -> 2.16 ms,
# 3 -> 2.21 ms), blocks of at most TILE_MAX_ROWS rows (256-row blocks of 8 waves, one per CU: 2.75 ms; 64: 4.4 ms).
TILE_CAP = 512
TILE_MIN_COUNT = 2
TILE_MAX_ROWS = 128
TILE_SPARSE_DENSITY = 0.12


def _tile_params():
    env = _env("SGF_SPMM_TILE")          # "cap,min_count,max_rows" (experiments)
    if env:
        c, m, r = (int(t) for t in env.split(","))
        return c, m, r
    return TILE_CAP, TILE_MIN_COUNT, TILE_MAX_ROWS


class TilePlan:
    """Plan of sgf_spmm_tile for one CSR: row blocks, the sources each block stages, the dense tiles as matrix-core
    fragments (hi + lo bf16; packed: sparse groups as entries, see K.tile_pack) and the CSR of the entries left on the
    gather path.  keep_dense=True keeps the unpacked fragments as .tiles (tests)."""

    def __init__(self, rowptr, colind, val, n: int, blk_row: torch.Tensor, cap=None, min_count=None, keep_dense=False):
        c, m, _ = _tile_params()
        self.blk_row, self.nb = blk_row, int(blk_row.numel()) - 1
        self.block_rows = int((blk_row[1:] - blk_row[:-1]).max()) if self.nb > 0 else 1
        self.cap, self.min_count = int(cap or c), int(min_count or m)
        (self.sh_ptr, self.sh_cols, self.tile_ptr, self.tiles, self.rem_rowptr, self.rem_col, self.rem_val,
         st) = K.tile_plan(rowptr, colind, val, n, blk_row, self.cap, self.min_count, LONG_ROW)
        self.tile_entries, self.staged_rows, _, self.nnz, self.fragments, self.rem_entries = st[:6]
        self.tile_fraction = self.tile_entries / max(self.nnz, 1)
        # stored entries per tile cell: below ~2 % a tile column moves more bytes than the gathers it replaces
        self.tile_density = self.tile_entries / max(self.fragments * 512, 1)
        self.long_segments = long_row_segments(self.rem_rowptr, None)
        self.grp, self.pool, units = K.tile_pack(blk_row, self.tile_ptr, self.tiles, self.fragments)
        self.tile_bytes = units * 16                       # what a launch reads of them (dense: fragments * 2048)
        if not keep_dense:
            self.tiles = None
        self.bytes = (self.pool.numel() + self.grp.numel() * 4 + self.rem_col.numel() * 8 + self.rem_rowptr.numel() * 8
                      + self.sh_cols.numel() * 4)


# When to re-order (SGF_REORDER): "auto" (default) tries once per cached graph with at least
# REORDER_MIN_NODES nodes, at its second forward (a graph seen once is a mini-batch: planning would cost
# more than it saves) or when prepare_graph() asks for it; "1" tries every graph at first use; "0" never.
# The order is adopted only if the row-block plan on the re-ordered CSR then serves at least
# REORDER_MIN_LDS_FRACTION of the stored entries from LDS — a uniform random graph is an expander, no order
# helps it, and it keeps the plain kernel on its original CSR.
REORDER_MIN_NODES = 100_000
REORDER_MIN_LDS_FRACTION = 0.25
REORDER_ITERS = (6, 6)
_reorder_mode = None


def set_reorder_mode(mode: Optional[str]):
    """'auto' | 'always' | 'never' | None (= read SGF_REORDER).  Returns the previous setting."""
    global _reorder_mode
    prev, _reorder_mode = _reorder_mode, mode
    return prev


def _mode() -> str:
    return _reorder_mode or {"0": "never", "1": "always"}.get(_env("SGF_REORDER", "auto"), "auto")


class GraphView:
    """(graph, perm, inv): `graph` is the CSRGraph the layers multiply with; when perm is not None the
    model's rows are in the re-ordered numbering: row p of every activation is original node perm[p],
    and original node v sits at row inv[v]."""

    def __init__(self, graph, perm, inv, stats=None):
        self.graph, self.perm, self.inv, self.stats = graph, perm, inv, stats or {}

    @staticmethod
    def decide(g: "CSRGraph", now: bool):
        mode = _mode()
        if mode == "never" or K.name != "hip" or g.nnz == 0 or g.nnz >= 2 ** 32 - 1:
            return GraphView(g, None, None, {"reordered": False, "why": "disabled"})
        if mode == "auto":
            if g.n < REORDER_MIN_NODES:
                return GraphView(g, None, None, {"reordered": False, "why": "small graph"})
            if not now and g.forward_calls < 2:
                return None                    # undecided: wait for the second forward on this graph
        perm, inv, comm = K.reorder(g.edge_index, g.n, *REORDER_ITERS)
        g2 = CSRGraph(inv.long()[g.edge_index], g.n, validate=False)
        # how much neighbour sharing the new order exposes: the share of stored entries that fall into the dense
        # tiles of community-aligned row blocks — the adoption criterion, whichever kernel then runs
        g2.blk_row = K.tile_blocks(comm[perm.long()].contiguous(), g.n, _tile_params()[2], g.device)
        try:
            tp = g2.tile_plan(False)
        except (ValueError, _lib.SgfError) as e:
            # a plan the tile kernel cannot take (a row block out of range, nnz beyond its 32-bit offsets): keep the graph
            # as given rather than fail the forward
            return GraphView(g, None, None, {"reordered": False, "why": f"tile plan unsupported: {e}"})
        if tp.tile_density < TILE_SPARSE_DENSITY and tp.min_count == TILE_MIN_COUNT and not _env("SGF_SPMM_TILE"):
            # tiles this sparse (a skewed graph: many sources referenced just twice per block) move more fragment bytes
            # than the gathers they replace: stage only sources with one more reference (power-law community graph at
            # ogbn-products scale: density 0.08 -> 0.11, 3.08 -> 2.92 ms; profiles/r03_spmm_tile.md)
            g2.tile_min_count = TILE_MIN_COUNT + 1
            g2._tile_plans.clear()
            tp = g2.tile_plan(False)
        stats = {"lds_fraction": tp.tile_fraction, "tile_density": tp.tile_density, "blocks": tp.nb,
                 "staged_rows_per_node": tp.staged_rows / max(g.n, 1), "plan_bytes": tp.bytes, "min_count": tp.min_count}
        if tp.tile_fraction < REORDER_MIN_LDS_FRACTION and mode != "always":
            return GraphView(g, None, None, {**stats, "reordered": False, "why": "no reuse to exploit"})
        # Which kernel multiplies with the re-ordered CSR: dense matrix-core tiles + gather remainder (sgf_spmm_tile)
        # for bf16 rows of 128 / 256 features; the flattened stream kernel (sgf_spmm_stream) otherwise and under
        # SGF_SPMM_TILED=0; SGF_SPMM_BLOCKED=1 selects r02's LDS-staged row blocks (profiles/r02_spmm_structured.md).
        g2.locality = True        # its gathers mostly hit in L2: ops.spmm_on picks sgf_spmm_stream
        g2.blocked = _env("SGF_SPMM_BLOCKED", "0") == "1"
        g2.tiled = _env("SGF_SPMM_TILED", "1") == "1" and not g2.blocked
        if not g2.tiled:
            g2._tile_plans.clear()
        stats["kernel"] = ("row-block (LDS-staged)" if g2.blocked else
                           "tiles (matrix cores) + gather remainder for bf16 rows of 128 / 256 features, else stream"
                           if g2.tiled else "stream")
        return GraphView(g2, perm, inv, {**stats, "reordered": True})


def prepare_graph(edge_index: torch.Tensor, num_nodes: int) -> GraphView:
    """Build everything that is per-graph, not per-step: the CSR, and (policy above) the node order and
    row-block plan.  The trainers need not call this — the same work happens lazily in the first two
    forwards — bench.py does, so that it stays outside the timed region like the CSR build."""
    return graph_cache.get(edge_index, num_nodes).view(now=True)


class _GraphCache:
    """edge_index -> CSRGraph, keyed on tensor identity AND version: the
    mini-batch trainers hand in a fresh edge_index every step, so entries are bounded (LRU) and each
    entry pins its key tensor so a recycled data_ptr can never alias a stale graph."""

    def __init__(self, capacity: int = 4):
        self.capacity = capacity
        self._d: "OrderedDict[tuple, CSRGraph]" = OrderedDict()

    def get(self, edge_index: torch.Tensor, num_nodes: int, factory=None, tag=None):
        key = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape),
               tuple(edge_index.stride()), str(edge_index.device), int(num_nodes), tag)
        g = self._d.get(key)
        if g is not None:  # the entry pins its tensor, so an equal key means the same live memory
            self._d.move_to_end(key)
            return g
        g = (factory or CSRGraph)(edge_index, num_nodes)
        g.edge_index_ref = edge_index
        self._d[key] = g
        while len(self._d) > self.capacity:
            self._d.popitem(last=False)
        return g

    def clear(self):
        self._d.clear()


graph_cache = _GraphCache()


# ------------------------------------------------------------------------------------------------
# T2: SpMM (large/ours.py:34)
# ------------------------------------------------------------------------------------------------
def _sharded_spmm(graph, x, shard, transposed: bool):
    """Local rows of A (or of A^T) times the node-sharded operand.

    Halo path (graph.halo(...).enabled): pack the rows the peers need, one all_to_all_single, product on
    [own rows ; halo rows] with the block's relabelled columns — bytes on the links = the distinct cut-edge
    sources only.  Fallback when the cut is (nearly) everything: all-gather of the operand PIPELINED against
    the product — the operand is split into column chunks, every chunk's all-gather is issued up front
    (asynchronously, on the collective's own stream), and the SpMM of chunk c starts as soon as chunk c has
    arrived while chunks c+1.. are still on the xGMI links."""
    rowptr, colind, val, long_segments = graph.arrays(transposed)
    n_local = graph.n_local
    plan = graph.halo(shard, transposed)
    if plan is not None and plan.enabled:
        if plan.n_halo == 0:                      # nothing to exchange (one rank, or a block without cut edges)
            return _own_block_spmm(graph, plan, (rowptr, plan.colind, val, long_segments), x, n_local, transposed)
        if shard.overlap:
            shard.overlapped_exchanges += 1
            # the entries whose source this rank owns are multiplied while the halo rows are on the links; the halo
            # entries follow when they have arrived (their sum is rounded to the storage dtype before it is added: bf16
            # rows with cut edges carry two roundings more than the single-GPU product)
            own, (rp_h, ci_h, va_h, seg_h) = plan.split(rowptr, val, n_local)
            recv, work, keep = shard.halo_exchange_start(x, plan)
            y = _own_block_spmm(graph, plan, own, x, n_local, transposed)
            work.wait()
            y.add_(K.spmm(rp_h, ci_h, va_h, recv, n_local, long_segments=seg_h))
            del keep
            return y
        return K.spmm(rowptr, plan.colind, val, shard.halo_exchange(x, plan), n_local, long_segments=long_segments)
    d = x.shape[1]
    chunks = shard.gather_chunks(d)
    if chunks <= 1:
        return K.spmm(rowptr, colind, val, shard.all_gather_rows(x), n_local, long_segments=long_segments)
    w = d // chunks
    pending = [shard.all_gather_rows(x[:, c * w:(c + 1) * w].contiguous(), async_op=True) for c in range(chunks)]
    y = torch.empty((n_local, d), dtype=x.dtype, device=x.device)
    for c, (buf, work) in enumerate(pending):
        work.wait()                                   # the compute stream waits for THIS chunk only
        K.spmm(rowptr, colind, val, buf, n_local, out=y[:, c * w:(c + 1) * w], long_segments=long_segments)
    return y


def _tile_operand_ok(x: torch.Tensor, out=None) -> bool:
    """sgf_spmm_tile takes x (and `out`): a width and dtype it has kernels for, an operand within its 32-bit byte offsets (= the
    entry's own bound), rows of `out` it can store 16 bytes at a time."""
    return (_has(K, "tile_supported", x.shape[1], x.dtype)
            and x.shape[0] * max(x.stride(0), x.shape[1]) * 2 < 2 ** 32 - 2048
            and (out is None or (out.stride(0) % 8 == 0 and out.data_ptr() % 16 == 0)))


def _own_block_spmm(graph, plan, own, x, n_local: int, transposed: bool):
    """The square block of a rank's rows x the rank's OWN columns (the part of a node-sharded product that needs no
    exchange).  When the partition follows sgf_reorder's order (dist.Repartition sets graph.locality / comm_local) this
    block has the structure the re-ordered single-GPU graph has, and takes the same kernels: the matrix-core tile kernel (bf16
    rows of 128 / 256 features; one plan per HaloPlan: None = undecided, False = no) or the stream kernel; else the row kernel."""
    rp, ci, va, segs = own
    if not graph.locality:
        return K.spmm(rp, ci, va, x, n_local, long_segments=segs)
    if (_tile_operand_ok(x) and graph.comm_local is not None and _env("SGF_SPMM_TILED", "1") == "1" and n_local >= 256):
        if plan.own_tile_plan is None:
            try:
                blk_row = K.tile_blocks(graph.comm_local, n_local, _tile_params()[2], x.device)
                tp = TilePlan(rp, ci, va, n_local, blk_row)
                # too little to put on the matrix cores: stream kernel
                plan.own_tile_plan = tp if tp.tile_fraction >= REORDER_MIN_LDS_FRACTION else False
            except (ValueError, _lib.SgfError):
                plan.own_tile_plan = False
        if plan.own_tile_plan:
            return K.spmm_tile(plan.own_tile_plan, x, n_local)
    return K.spmm(rp, ci, va, x, n_local, long_segments=segs, stream_hint=True)


class _SpMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, graph, shard, packed=None, layer=None):
        K.check(x)
        ctx.graph, ctx.shard, ctx.layer = graph, shard, layer
        if shard is not None:
            # node-sharded: rows of A local, X rows gathered from all ranks (halo all-gather)
            return _sharded_spmm(graph, x, shard, False)
        return spmm_on(graph, x, False, packed=packed, coded_class=None if layer is None else f"fwd{layer}")

    @staticmethod
    def backward(ctx, gy):
        graph, shard = ctx.graph, ctx.shard
        if shard is not None:
            # dX_local = (A^T dY)[local rows]: local rows of the CSR of A^T times the sharded dY
            return _sharded_spmm(graph, gy.contiguous(), shard, True), None, None, None, None
        coded_class = None if ctx.layer is None else f"bwd{ctx.layer}"
        return spmm_on(graph, gy.contiguous(), True, coded_class=coded_class), None, None, None, None


def spmm_packed_slot(graph, x_shape, dtype, slot_bytes: int) -> int:
    """`slot_bytes` if A x for a contiguous x of this shape would gather a packed copy of x with slots of that size
    (K.bn_apply_packed -> spmm(..., packed=...)), else 0: the graph takes the wave-per-row launch and the launcher's own
    rule holds (bf16 rows of 256 columns, SGF_SPMM_PACKED).  Rows on the long-row path are reduced from the dense x."""
    if not slot_bytes or not _has(K, "spmm_packed_supported") or graph.blocked or graph.tiled or graph.locality:
        return 0                   # (spmm_on's last two branches only: no row-block plan, no tile plan, no locality hint)
    return slot_bytes if K.spmm_packed_supported(x_shape, dtype, slot_bytes) else 0


# The plain wave-per-row launches of a full-graph training step may gather a lossless 12-bit coded copy of their operand
# (csrc/spmm_coded.hip, k_spmm_row_coded: 384 bytes per row where the dense row takes 512; SGF_SPMM_CODED=0 turns it off).
# Each such launch first writes the coded rows and a copy of the CSR values with the rows' scales folded in (two streaming
# passes, 0.94 + 0.5 GB of scratch at products size, released after the launch), so it is used only where the gather saves
# more than they cost: CODED_CLASSES names the launch classes — "fwd2", "fwd3" (the forward SpMMs of GCN layers 2 and 3;
# layer 1 gathers its packed copy), "bwd3", "bwd2", "bwd1" — set from the step A/B of profiles/spmm_coded_ab.txt: added one at
# a time only "fwd2" lowers the step by more than three times the spread of its runs; the other four each gain 0.9-1.6 ms
# there, under the bound, and stay off until an A/B resolves them.
# Operands of fewer than CODED_MIN_NODES rows stay dense (mini-batches: the passes are launch-bound there).
CODED_MIN_NODES = 65536
CODED_CLASSES = frozenset({"fwd2"})


def _coded_ok(graph, x: torch.Tensor, out, packed, coded_class) -> bool:
    return (coded_class in CODED_CLASSES and packed is None and out is None and x.dim() == 2 and x.shape[1] == 256
            and x.dtype == torch.bfloat16 and x.shape[0] >= CODED_MIN_NODES and x.is_contiguous()
            and _has(K, "spmm_coded") and not torch.cuda.is_current_stream_capturing()
            and K.spmm_coded_supported(x.shape, x.dtype))


def _spmm_coded(coded_class, rp, ci, va, x: torch.Tensor, n: int, segs: int) -> torch.Tensor:
    slots, scale, n_escaped = K.spmm_code_rows(x)
    if _coded.escape_log is not None:
        _coded.escape_log.append((coded_class, n_escaped, x.shape[0]))
    val_coded, n_unsupported = K.spmm_code_values(ci, va, scale)
    return K.spmm_coded(rp, ci, va, val_coded, x, slots, n_unsupported, n, long_segments=segs)


def spmm_on(graph, x: torch.Tensor, transposed: bool, out=None, packed=None, coded_class=None) -> torch.Tensor:
    """A x or A^T x on one GPU, on the first kernel that applies: the LDS-staged row-block kernel (graph.blocked, rows of at most
    256 columns); matrix-core tiles + gather remainder (graph.tiled and _tile_operand_ok); the stream kernel (graph.locality);
    the wave-per-row launch gathering `packed`, the producer's packed copy of x (K.bn_apply_packed; A x into a fresh tensor
    only); the wave-per-row launch gathering a 12-bit coded copy of x made here (`coded_class` in CODED_CLASSES, _coded_ok);
    else the wave-per-row kernel on x, long rows split over workgroups."""
    rp, ci, va, segs = graph.arrays(transposed)
    plan = graph.plan(x.dtype, transposed) if (graph.blocked and x.shape[1] <= 256) else None
    if plan is not None:
        return K.spmm_blocked(rp, plan, x, graph.n, out=out, long_segments=segs)
    if graph.tiled:
        if _tile_operand_ok(x, out):
            return K.spmm_tile(graph.tile_plan(transposed), x, graph.n, out=out)
        if not K.tile_supported(x.shape[1], x.dtype) and graph._tile_plans:
            # this graph is being multiplied in a storage dtype / width the tile kernel does not take (fp32 runs): the plan
            # GraphView.decide built for its adoption statistics (about the size of the CSR) is dropped, not kept resident
            graph._tile_plans.clear()
    if graph.locality:
        return K.spmm(rp, ci, va, x, graph.n, out=out, long_segments=segs, stream_hint=True)
    if packed is not None and not transposed and out is None:
        return K.spmm_packed(rp, ci, va, x, packed, graph.n, long_segments=segs)
    if _coded_ok(graph, x, out, packed, coded_class):
        return _spmm_coded(coded_class, rp, ci, va, x, graph.n, segs)
    return K.spmm(rp, ci, va, x, graph.n, out=out, long_segments=segs)


def spmm(graph, x: torch.Tensor, shard=None, packed=None, layer=None) -> torch.Tensor:
    """Y = A X with A the cached normalised adjacency (torch_sparse.matmul(adj, x) in the reference).  `packed`: a packed
    copy of X for the forward gathers (spmm_packed_slot says when one is of use); the backward never reads it.  `layer`:
    the 1-based GCN layer of this product, which names its forward and backward launch classes (CODED_CLASSES)."""
    return _SpMM.apply(x, graph, shard, packed, layer)
