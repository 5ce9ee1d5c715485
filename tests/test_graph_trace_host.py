"""What the graph layer (sgformer_amd/graph.py and the graph code of dist.py, batching.py, sampling.py, graphed.py) asks of
the kernel table, pinned without a GPU and compared with tests/golden/graph_trace.json.  Every case is a list of lines:

  * every kernel-table call in order (K.check left out): the method name, every positional and every keyword argument
    (`long_segments`, `stream_hint`, `out`, `packed`).  A tensor is shown as dtype[shape]#k, with /s[strides] when it is a view
    that is not contiguous and +offset when it does not start its storage: k numbers the storages of ONE case in order of
    first appearance, so the lines say which of the graph's arrays a launch was handed (`note graph ...` lines give the numbers
    of rowptr / colind / val).  A plan object is shown as its class and a number of the same kind;
  * the collectives of the stand-in shard;
  * `note` lines the case writes itself: flags, `GraphView.stats` key by key, hints, SHA-256 digests of results.

Two tables.  Cases that compute run on tests/cpu_kernels.CpuKernels (plus the two entries it lacks that the graph layer
probes for: sampled_csr_transpose, subgraph_csr — restated here on top of the CPU table).  GraphView.decide and the tile,
row-block, stream and packed arms are reachable only when K.name == "hip": their table is `FakeHip`, whose planning entries
return canned small tensors and statistics chosen per case and whose SpMM entries return zeros of the right shape — what these
cases pin is which call is made, in which order, with which arguments; their result is not pinned.

The node-sharded cases use ONE process: `Rank0` owns the first n_local of n rows, its only peer never asks for a row
(torch.distributed's all_reduce / all_to_all_single are replaced for the case: identity / "nothing asked"), it reports world = 1
so that the degree and symmetry reductions of dist.ShardedGraph see every edge.  dist.ShardContext itself cannot be built without
a process group: its constructor, for_batch, repartition_for and its collectives stay with tests/test_dist.py (gloo);
ShardContext.graph_for is called here as a plain function on the stand-in.

Edge hints are written and read through `_hint` / `_hints`, which use graph.EdgeHints; on a commit from before that record the
same six fields were loose attributes of the edge list named "_sgf_" + field, which the two helpers fall back to — so this file
and its golden file pass on the parent of the refactor as they pass after it.

Functions of the six modules this file does not reach, and the test that covers each:
  graph.py      _block_shape's SGF_SPMM_BLOCK arm, _tile_params' SGF_SPMM_TILE parsing beyond "set": tests/test_gpu_blocked.py,
                tests/test_gpu_tile.py; prepare_graph: tests/test_gpu_scale.py, bench.py; TilePlan(keep_dense=True):
                tests/test_gpu_tile.py
  dist.py       _mix64, ShardedGraph._init_from_local_edges, RowExchange, _Exchange, Repartition,
                ShardContext (all but graph_for), shard_model, sharded_nll_loss, sharded_bce_loss: tests/test_dist.py
  batching.py   _on_gpu, subgraph's prep-stream arm, graph_prologue, to_undirected, remove_self_loops, add_self_loops:
                tests/test_gpu_r05.py, tests/test_gpu_staging.py, tests/test_host.py
  sampling.py   _DeviceGraph, _shared_get, _sampled_csr, NeighborSampler, NeighborLoader: tests/test_gpu_sampler.py,
                tests/test_gpu_sampled_csr.py
  graphed.py    collect, _PerModel, enabled, graph_dropout, draw_seeds, _drop_state, _fused_dropout_sites, StaticCSR.load,
                _Core, _Entry, _eligible, _capture, maybe_step, _Done: tests/test_gpu_graphed.py,
                tests/test_gpu_graphed_dropout.py
  ours.py       everything but the graph resolution of GraphConvLayer.propagate / GraphConv.pack_request / SGFormer.forward,
                which tests/test_model_trace_host.py pins (CPU table) and tests/test_gpu_spmm_packed_model.py,
                tests/test_gpu_graphed*.py run on the device

`python tests/test_graph_trace_host.py --write` regenerates the golden file from the code as it stands.
"""
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "graph_trace.json")

from tests.cpu_kernels import CpuKernels  # noqa: E402

_SHORT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float64: "f64", torch.int64: "i64", torch.int32: "i32",
          torch.bool: "b8", torch.uint8: "u8"}
_BF16, _F32 = torch.bfloat16, torch.float32
FIELDS = ("trusted", "max_in_degree", "csr", "csr_t_lazy", "symmetric", "sharded_graph")
SWITCHES = ("SGF_REORDER", "SGF_SPMM_TILE", "SGF_SPMM_TILED", "SGF_SPMM_BLOCKED", "SGF_SPMM_BLOCK", "SGF_SUBGRAPH_CSR")


# ------------------------------------------------------------------------------------------------
# the log
# ------------------------------------------------------------------------------------------------
class Trace:
    def __init__(self):
        self.lines, self._ids, self._keep = [], {}, []

    def _num(self, key, obj):
        if key not in self._ids:
            self._ids[key] = len(self._ids) + 1
            self._keep.append(obj)                    # pinned: an address is never handed out twice within a case
        return self._ids[key]

    def fmt(self, v, depth=2):
        if isinstance(v, torch.Tensor):
            s = f"{_SHORT.get(v.dtype, str(v.dtype))}{list(v.shape)}"
            ptr = v.untyped_storage().data_ptr()
            s += f"#{self._num(('t', ptr), v)}" if ptr else "#-"
            if v.storage_offset():
                s += f"+{v.storage_offset()}"
            return s if v.is_contiguous() else f"{s}/s{list(v.stride())}"
        if v is None or isinstance(v, (bool, int, float, str)):
            return repr(v)
        if isinstance(v, (torch.dtype, torch.device)):
            return _SHORT.get(v, str(v))
        if isinstance(v, (list, tuple)):
            return "[" + (", ".join(self.fmt(w, depth - 1) for w in v) if depth else "...") + "]"
        return f"{type(v).__name__}#{self._num(('o', id(v)), v)}"

    def note(self, text):
        self.lines.append(f"note {text}")

    def graph(self, name, g):
        self.note(f"graph {name}: {type(g).__name__} n={g.n} rowptr={self.fmt(g.rowptr)} colind={self.fmt(g.colind)} "
                  f"val={self.fmt(g.val)} long_segments={g.long_segments}")

    def sha(self, name, t):
        h = hashlib.sha256()
        t = t.detach().contiguous()
        h.update(f"{_SHORT.get(t.dtype, str(t.dtype))}{list(t.shape)};".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
        self.note(f"sha256 {name} {h.hexdigest()[:24]}")


class Recording:
    """A kernel table behind a log.  A method the table lacks stays missing (hasattr is the product's rule)."""

    def __init__(self, table, tr):
        self._table, self._tr = table, tr

    def __getattr__(self, name):
        attr = getattr(self._table, name)
        if not callable(attr) or name == "check":
            return attr

        def call(*args, **kwargs):
            shown = [self._tr.fmt(a) for a in args] + [f"{k}={self._tr.fmt(v)}" for k, v in sorted(kwargs.items())]
            self._tr.lines.append(f"{name}({', '.join(shown)})")
            return attr(*args, **kwargs)
        return call


class CpuTable(CpuKernels):
    """CpuKernels plus the two optional entries the graph layer probes for."""

    def __init__(self, with_subgraph_csr=False, canned_csr=False):
        if with_subgraph_csr:
            self.subgraph_csr = self._subgraph_csr
        if canned_csr:                                                 # (an edge list the CPU oracle could not index)
            self.csr_build = lambda ei, n: (torch.zeros(n + 1, dtype=torch.int64), torch.zeros(ei.shape[1], dtype=torch.int32),
                                            torch.zeros(ei.shape[1]), torch.zeros(n, dtype=torch.int32))

    @staticmethod
    def sampled_csr_transpose(rowptr, colind, val, n):
        rows = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
        order = torch.argsort(colind.long() * n + rows, stable=True)
        t_rowptr = torch.zeros(n + 1, dtype=torch.int64)
        torch.cumsum(torch.bincount(colind.long(), minlength=n), 0, out=t_rowptr[1:])
        return t_rowptr, rows[order].to(torch.int32), val[order].clone()

    @staticmethod
    def _subgraph_csr(rowptr, colind, n, subset, local_of, want_edges):
        rows = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
        out, _ = CpuKernels.subgraph(torch.stack([colind.long(), rows]), n, subset, True, False)
        m = int(subset.numel())
        rp, ci, va, deg = CpuKernels.csr_build(out, m)
        return rp, ci, va, deg, out, (int((rp[1:] - rp[:-1]).max()) if m else 0)


class FakeHip:
    """The stand-in for HipKernels: named "hip", plans canned per case, products zeros.  The CSR entries are the CPU table's."""
    name = "hip"
    csr_build, csr_transpose, reorder = (staticmethod(f) for f in (CpuKernels.csr_build, CpuKernels.csr_transpose, CpuKernels.reorder))
    sampled_csr_transpose = staticmethod(CpuTable.sampled_csr_transpose)

    def __init__(self, tile=(251, 1), plan_error=None, packed=True):
        # tile = (entries in tiles per 1000 stored entries, fragments): tile_fraction = tile[0] / 1000, density = tile[0] / (512 * tile[1])
        self.tile, self.plan_error = tile, plan_error
        if packed:
            self.spmm_packed_supported = lambda x_shape, dtype, slot_bytes: dtype == _BF16 and x_shape[1] == 256

    @staticmethod
    def check(*tensors):
        return None

    @staticmethod
    def lds_rows_max(dtype):
        return 288 if dtype == _BF16 else 144

    @staticmethod
    def tile_supported(d, dtype):
        return dtype == _BF16 and d in (128, 256)

    @staticmethod
    def tile_blocks(comm_sorted, n, max_rows, device):
        return torch.tensor([0, n // 2, n], dtype=torch.int32)

    def tile_plan(self, rowptr, colind, val, n, blk_row, cap, min_count, long_len):
        if self.plan_error is not None:
            raise self.plan_error
        nb = int(blk_row.numel()) - 1
        z = lambda k, dt=torch.int32: torch.zeros(k, dtype=dt)   # noqa: E731
        return (z(nb + 1), z(4), z(nb + 1), z(16, _BF16), z(n + 1, torch.int64), z(0), z(0, _F32),
                [self.tile[0], 7, 0, 1000, self.tile[1], 1000 - self.tile[0], 0, 0])

    @staticmethod
    def tile_pack(blk_row, tile_ptr, tiles, n_frag):
        return torch.zeros((1, 2), dtype=torch.int32), torch.zeros(16, dtype=torch.uint8), 3

    @staticmethod
    def spmm_plan(rowptr, colind, val, n, rows_per_block, lds_rows, long_len):
        nnz, nb = int(colind.numel()), (n + rows_per_block - 1) // rows_per_block
        z = lambda k, dt=torch.int32: torch.zeros(k, dtype=dt)   # noqa: E731
        return z(nnz), z(nnz, _F32), z(max(n, 1)), z(nb + 1), z(4), [nnz // 2, 5, 9, nnz]

    @staticmethod
    def _zeros(x, n_rows, out):
        return out if out is not None else torch.zeros((n_rows, x.shape[1]), dtype=x.dtype, device=x.device)

    @staticmethod
    def spmm(rowptr, colind, val, x, n_rows, out=None, long_segments=0, stream_hint=False):
        return FakeHip._zeros(x, n_rows, out)

    @staticmethod
    def spmm_tile(plan, x, n_rows, out=None):
        return FakeHip._zeros(x, n_rows, out)

    @staticmethod
    def spmm_blocked(rowptr, plan, x, n_rows, out=None, long_segments=0):
        return FakeHip._zeros(x, n_rows, out)

    @staticmethod
    def spmm_packed(rowptr, colind, val, x, packed, n_rows, long_segments=0):
        return FakeHip._zeros(x, n_rows, None)


# ------------------------------------------------------------------------------------------------
# edge lists, hints
# ------------------------------------------------------------------------------------------------
def sym_edges(n=24):
    """Ring + chords of stride 5, both directions, self loops: A^T == A."""
    i = torch.arange(n)
    src = torch.cat([i, (i + 1) % n, i, (i + 5) % n, i])
    dst = torch.cat([(i + 1) % n, i, (i + 5) % n, i, i])
    return torch.stack([src, dst]).long()


def dir_edges(n=24):
    """Directed ring + chords of stride 7 + a few parallel edges: A^T != A."""
    i = torch.arange(n)
    return torch.stack([torch.cat([i, i, i[:3]]), torch.cat([(i + 1) % n, (i + 7) % n, (i[:3] + 1) % n])]).long()


def _hint(ei, **fields):
    """Mark an edge list as a producer would (module docstring)."""
    from sgformer_amd import graph
    assert set(fields) <= set(FIELDS)
    if hasattr(graph, "EdgeHints"):
        graph.EdgeHints(**fields).attach(ei)
    else:
        for k, v in fields.items():
            setattr(ei, "_sgf_" + k, v)
    return ei


def _hints(ei):
    """{field: value} of the hints an edge list carries, defaults included."""
    from sgformer_amd import graph
    if hasattr(graph, "EdgeHints"):
        h = graph.hints_of(ei)
        return {k: getattr(h, k) for k in FIELDS}
    default = {"trusted": False, "csr_t_lazy": False, "symmetric": False}
    return {k: getattr(ei, "_sgf_" + k, default.get(k)) for k in FIELDS}


def _note_hints(tr, name, ei):
    h = _hints(ei)
    tr.note(f"hints {name}: " + ", ".join(f"{k}={tr.fmt(h[k]) if k != 'sharded_graph' else type(h[k]).__name__}" for k in FIELDS))


def _flags(g):
    return (f"blocked={getattr(g, 'blocked', False)} tiled={getattr(g, 'tiled', False)} locality={getattr(g, 'locality', False)} "
            f"tile_min_count={getattr(g, 'tile_min_count', None)}")


# ------------------------------------------------------------------------------------------------
# CSRGraph construction
# ------------------------------------------------------------------------------------------------
def case_build(tr, mp, table, kind):
    from sgformer_amd import ops
    ei = sym_edges() if kind == "symmetric" else dir_edges()
    g = ops.CSRGraph(ei, 24)
    tr.graph("g", g)
    tr.note(f"symmetric={g.symmetric} t_long_segments={g.t_long_segments}")
    t1 = g.transposed()
    tr.note(f"transposed: {tr.fmt(list(t1))} symmetric={g.symmetric} t_long_segments={g.t_long_segments}")
    before = len(tr.lines)
    t2 = g.transposed()
    tr.note(f"transposed again: {len(tr.lines) - before} table calls, same arrays: {all(a is b for a, b in zip(t1, t2))}")
    tr.sha("rowptr", g.rowptr), tr.sha("colind", g.colind), tr.sha("val", g.val), tr.sha("t val", t1[2])


def case_long_segments(tr, mp, table):
    from sgformer_amd import graph, ops
    L = ops.LONG_ROW
    rowptr = torch.tensor([0, 3, L + 8, L + 9])
    tr.note(f"empty rowptr: {ops.long_row_segments(torch.zeros(1, dtype=torch.int64))}")
    tr.note(f"hint == LONG_ROW: {ops.long_row_segments(rowptr, L + 9, L)}")
    tr.note(f"hint LONG_ROW + 1, small nnz: {ops.long_row_segments(rowptr, L + 9, L + 1)}")
    tr.note(f"nnz == LONG_ROW: {ops.long_row_segments(rowptr, L)}")
    tr.note(f"nnz 5 * LONG_ROW + 3: {ops.long_row_segments(rowptr, 5 * L + 3)}")
    tr.note(f"exact, no nnz: {ops.long_row_segments(rowptr)}")
    # the exact count through CSRGraph: a multigraph row of LONG_ROW + 5 duplicate edges, no longer a "small graph"
    mp.setattr(graph, "SMALL_GRAPH_NNZ", 64)
    dup = torch.stack([torch.full((L + 5,), 2), torch.full((L + 5,), 4)]).long()
    ei = torch.cat([sym_edges(), dup], dim=1)
    g = ops.CSRGraph(ei, 24)
    tr.graph("multigraph", g)
    g.transposed()
    tr.note(f"symmetric={g.symmetric} t_long_segments={g.t_long_segments}")
    g = ops.CSRGraph(_hint(ei.clone(), max_in_degree=L), 24)
    tr.note(f"the same list with max_in_degree == LONG_ROW: long_segments={g.long_segments}")
    g = ops.CSRGraph(_hint(ei.clone(), max_in_degree=L + 5), 24)
    tr.note(f"with max_in_degree == LONG_ROW + 5: long_segments={g.long_segments}")


def case_hint_trusted(tr, mp, table):
    from sgformer_amd import ops
    bad = sym_edges()
    bad[0, 3] = 24
    for ei in (bad, torch.where(bad == 24, -1, bad)):
        with pytest.raises(IndexError, match=r"edge_index has node ids outside \[0, 24\)"):
            ops.CSRGraph(ei, 24)
    tr.note(f"out-of-range id, no hint: IndexError twice, table calls so far: {len(tr.lines)}")
    g = ops.CSRGraph(_hint(bad, trusted=True), 24)             # (the canned csr_build: nothing indexes with the bad id)
    tr.note(f"trusted: built, nnz={g.nnz}")
    g = ops.CSRGraph(bad.clone(), 24, validate=False)
    tr.note(f"validate=False: built, nnz={g.nnz}")
    for args, err in ((((sym_edges().int()), 24), ValueError), ((sym_edges()[0], 24), ValueError), ((sym_edges(), 2 ** 31), ValueError)):
        with pytest.raises(err) as info:
            ops.CSRGraph(*args)
        tr.note(f"{err.__name__}: {info.value}")


def case_hint_csr(tr, mp, table):
    from sgformer_amd import ops
    ei = dir_edges()
    pre = CpuKernels.csr_build(ei, 24)
    tr.note(f"producer's CSR: {tr.fmt(list(pre), 1)}")
    g = ops.CSRGraph(_hint(ei.clone(), csr=pre), 24)
    tr.graph("adopted", g)
    tr.note(f"deg is the producer's: {g.deg is pre[3]}")
    g.transposed()
    tr.note(f"symmetric={g.symmetric}")
    g = ops.CSRGraph(_hint(ei.clone(), csr=pre), 25)
    tr.graph("another node count", g)
    g = ops.CSRGraph(_hint(ei[:, :-1].clone(), csr=pre), 24)
    tr.graph("another edge count", g)
    g = ops.CSRGraph(_hint(ei[:, :-1].clone(), csr=pre, csr_t_lazy=True), 24)
    g.transposed()
    tr.note(f"lazy flag with a CSR that is not adopted: symmetric={g.symmetric}")


def case_hint_lazy(tr, mp, table, combo):
    from sgformer_amd import ops
    ei = dir_edges()
    pre = CpuKernels.csr_build(ei, 24)
    extra = dict(trusted=True, max_in_degree=3) if combo else {}
    g = ops.CSRGraph(_hint(ei.clone(), csr=pre, csr_t_lazy=True, **extra), 24)
    tr.graph("sampled", g)
    t = g.transposed()
    tr.note(f"transposed: {tr.fmt(list(t))} symmetric is False: {g.symmetric is False} t_long_segments={g.t_long_segments}")
    g.transposed()
    want = CpuKernels.csr_transpose(ei, 24, None, None, None)
    tr.note(f"equal to csr_transpose's arrays: {all(torch.equal(a, b) for a, b in zip(t, want[:3]))}")
    g = ops.CSRGraph(_hint(ei.clone(), csr_t_lazy=True), 24)
    g.transposed()
    tr.note(f"lazy flag without a CSR: symmetric={g.symmetric}")


def case_hint_symmetric(tr, mp, table, combo):
    from sgformer_amd import ops
    ei = sym_edges()
    extra = dict(trusted=True, max_in_degree=3, csr=CpuKernels.csr_build(ei, 24)) if combo else {}
    g = ops.CSRGraph(_hint(ei.clone(), symmetric=True, **extra), 24)
    tr.graph("promised", g)
    tr.note(f"symmetric={g.symmetric} t_long_segments={g.t_long_segments}")
    t = g.transposed()
    tr.note(f"transposed: {tr.fmt(list(t))}")
    g = ops.CSRGraph(_hint(ei.clone(), symmetric=False), 24)
    tr.note(f"symmetric=False is no promise: {g.symmetric}")


# ------------------------------------------------------------------------------------------------
# CSRGraph.view
# ------------------------------------------------------------------------------------------------
def _note_view(tr, g, v, name="view"):
    tr.note(f"{name}: graph is the caller's: {v.graph is g} perm={tr.fmt(v.perm)} inv={tr.fmt(v.inv)} {_flags(v.graph)} "
            f"blk_row={tr.fmt(getattr(v.graph, 'blk_row', None))} tile plans kept: {len(getattr(v.graph, '_tile_plans', None) or {})}")
    for k in sorted(v.stats):
        tr.note(f"  stats[{k!r}] = {v.stats[k]!r}")


def case_view(tr, mp, table, env=None, mode="unset", min_nodes=16, calls=(False,), kind="symmetric"):
    from sgformer_amd import graph, ops
    for k, val in (env or {}).items():
        mp.setenv(k, val)
    if min_nodes is not None:
        mp.setattr(graph, "REORDER_MIN_NODES", min_nodes)
    prev = ops.set_reorder_mode(mode) if mode != "unset" else None
    try:
        g = ops.CSRGraph(sym_edges() if kind == "symmetric" else dir_edges(), 24)
        tr.graph("g", g)
        views = []
        for i, now in enumerate(calls):
            v = g.view(now=now) if now else g.view()
            views.append(v)
            _note_view(tr, g, v, f"view call {i + 1} (now={now})")
        before = len(tr.lines)
        v = g.view()
        tr.note(f"one more call: {len(tr.lines) - before} table calls, the same view: {v is views[-1]}, forward_calls={g.forward_calls}")
    finally:
        if mode != "unset":
            ops.set_reorder_mode(prev)


# ------------------------------------------------------------------------------------------------
# spmm_on / spmm / spmm_packed_slot
# ------------------------------------------------------------------------------------------------
class _Packed:
    """Stands for kernels.PackedRows (spmm_on hands it through)."""


def case_spmm_on(tr, mp, table, kind):
    from sgformer_amd import ops
    n = 24
    big = torch.empty_strided((n, 128), (2 ** 27, 1), dtype=_BF16, device="meta")      # 24 * 2^27 * 2 bytes > 2^32: never allocated

    def fresh(**flags):
        g = ops.CSRGraph(sym_edges() if kind == "symmetric" else dir_edges(), n)
        for k, v in flags.items():
            setattr(g, k, v)
        return g

    def run(title, g, x, **kw):
        for transposed in (False, True):
            tr.note(f"-- {title}, {'A^T' if transposed else 'A'} x{list(x.shape)}")
            y = ops.spmm_on(g, x, transposed, **kw)
            tr.note(f"-> {tr.fmt(y)}" + (" (is out)" if kw.get("out") is y else ""))

    x64, x128, x260 = (torch.zeros(n, d, dtype=_BF16) for d in (64, 128, 260))
    blk = torch.tensor([0, 12, 24], dtype=torch.int32)
    g = fresh()
    tr.graph("plain", g)
    run("plain", g, x64)
    run("plain, out", g, x64, out=torch.zeros(n, 64, dtype=_BF16))
    run("packed", g, x64, packed=_Packed())
    run("packed and out", g, x64, packed=_Packed(), out=torch.zeros(n, 64, dtype=_BF16))
    g = fresh(locality=True)
    tr.graph("locality", g)
    run("locality", g, x64)
    run("locality, packed", g, x64, packed=_Packed())
    g = fresh(blocked=True, locality=True)
    tr.graph("blocked", g)
    run("row-block plan", g, x64)
    run("row-block plan again, out", g, x64, out=torch.zeros(n, 64, dtype=_BF16))
    run("row-block plan, fp32", g, x64.float())
    run("row-block graph, d > 256", g, x260)
    g = fresh(tiled=True, locality=True, blk_row=blk)
    tr.graph("tiled", g)
    run("tile", g, x128)
    run("tile again, aligned out", g, x128, out=torch.zeros(n, 128, dtype=_BF16))
    run("tile, misaligned out", g, x128, out=torch.zeros(n, 134, dtype=_BF16)[:, 3:131])
    run("tile, operand beyond the 32-bit bound", g, big)
    tr.note(f"tile plans kept: {len(g._tile_plans)}")
    run("tile refused by width", g, x64)
    tr.note(f"tile plans kept: {len(g._tile_plans)}")
    run("tile after the plans were dropped", g, x128)
    run("tile refused by dtype", g, x128.float())
    tr.note(f"tile plans kept: {len(g._tile_plans)}")
    g = fresh(tiled=True, blk_row=blk, tile_min_count=3)
    tr.graph("tiled, no locality, min_count 3", g)
    run("tile", g, x128)
    run("tile refused by width", g, x64, packed=_Packed())


def case_packed_slot(tr, mp, table):
    from sgformer_amd import graphed, ops
    ei = sym_edges()
    graphs = {"CSRGraph": ops.CSRGraph(ei, 24), "blocked": ops.CSRGraph(ei, 24), "tiled": ops.CSRGraph(ei, 24),
              "locality": ops.CSRGraph(ei, 24), "WeightedCSRGraph": ops.WeightedCSRGraph(ei, torch.ones(ei.shape[1]), 24),
              "StaticCSR": graphed.StaticCSR(24, 256, torch.device("cpu"), 0)}
    graphs["blocked"].blocked = graphs["tiled"].tiled = graphs["locality"].locality = True
    for name, g in graphs.items():
        got = [ops.spmm_packed_slot(g, shape, dt, slot) for shape, dt, slot in
               (((24, 256), _BF16, 384), ((24, 256), _BF16, 0), ((24, 128), _BF16, 384), ((24, 256), _F32, 384))]
        tr.note(f"{name}: {got}")


def case_autograd(tr, mp, table):
    from sgformer_amd import ops
    torch.manual_seed(3)
    x0 = torch.randn(24, 8)
    for name, ei in (("symmetric", sym_edges()), ("directed", dir_edges())):
        tr.note(f"-- {name}")
        g = ops.graph_cache.get(ei, 24)
        tr.graph(name, g)
        x = x0.clone().requires_grad_(True)
        y = ops.spmm(g, x)
        (y * torch.arange(8.0)).sum().backward()
        tr.sha("y", y), tr.sha("dx", x.grad)
        xb = x0.to(_BF16).requires_grad_(True)
        y = ops.spmm(ops.graph_cache.get(ei, 24), xb)
        y.float().sum().backward()
        tr.sha("y bf16", y), tr.sha("dx bf16", xb.grad)
    tr.note("-- weighted")
    ei = dir_edges()
    g = ops.WeightedCSRGraph(ei, torch.linspace(0.5, 2.0, ei.shape[1]), 24)
    tr.graph("weighted", g)
    tr.note(f"plan={g.plan(_F32)} symmetric={g.symmetric}")
    x = x0.clone().requires_grad_(True)
    y = ops.spmm(g, x)
    (y * torch.arange(8.0)).sum().backward()
    tr.sha("y", y), tr.sha("dx", x.grad)
    tr.note("packed is None for the table: " + str(ops.spmm_packed_slot(g, (24, 256), _BF16, 384)))


# ------------------------------------------------------------------------------------------------
# _sharded_spmm / _own_block_spmm
# ------------------------------------------------------------------------------------------------
class _Work:
    def __init__(self, tr):
        self._tr = tr

    def wait(self):
        self._tr.lines.append("work.wait()")


class Rank0:
    """One process standing for rank 0 of a node-sharded run (module docstring): what dist.ShardedGraph, dist.HaloPlan and
    ops._sharded_spmm touch of dist.ShardContext.  The rows of the silent peer are zeros."""
    group, rank, world, local_edges, halo_max, overlapped_exchanges = None, 0, 1, False, 0.5, 0

    def __init__(self, tr, n_global, n_local, overlap, chunks=1):
        self._tr, self.n_global, self.n_local, self.n_max, self.r0, self.r1 = tr, n_global, n_local, n_local, 0, n_local
        self.overlap, self._chunks, self.last_halo = overlap, chunks, None

    def all_reduce_exact(self, t):
        self._tr.lines.append(f"shard.all_reduce_exact({t.numel()})")
        return t

    def gather_chunks(self, d):
        self._tr.lines.append(f"shard.gather_chunks({d})")
        return self._chunks

    def all_gather_rows(self, x, async_op=False):
        self._tr.lines.append(f"shard.all_gather_rows({self._tr.fmt(x)}, async_op={async_op})")
        out = torch.zeros((self.n_global, x.shape[1]), dtype=x.dtype)
        out[:self.n_local] = x
        return (out, _Work(self._tr)) if async_op else out

    def halo_exchange(self, x, plan):
        self._tr.lines.append(f"shard.halo_exchange({self._tr.fmt(x)}, n_halo={plan.n_halo})")
        ext = torch.zeros((plan.n_ext, x.shape[1]), dtype=x.dtype)
        ext[:self.n_local] = x
        return ext

    def halo_exchange_start(self, x, plan):
        self._tr.lines.append(f"shard.halo_exchange_start({self._tr.fmt(x)}, n_halo={plan.n_halo})")
        return torch.zeros((plan.n_halo, x.shape[1]), dtype=x.dtype), _Work(self._tr), None


def _one_process_collectives(tr, mp):
    import torch.distributed as td

    def all_reduce(t, op=None, group=None):
        tr.lines.append(f"dist.all_reduce({t.numel()})")

    def all_to_all_single(out, inp, *a, **k):
        tr.lines.append(f"dist.all_to_all_single({out.numel()}, {inp.numel()})")
        out.zero_()                                   # the peer asks for nothing

    mp.setattr(td, "all_reduce", all_reduce)
    mp.setattr(td, "all_to_all_single", all_to_all_single)


def case_sharded(tr, mp, table, kind, n_local, overlap=True, chunks=1, halo_max=1.0):
    """Halo path (n_local < n: the columns beyond are the peer's) or, with halo_max = 0, the all-gather fallback."""
    from sgformer_amd import dist, ops
    _one_process_collectives(tr, mp)
    n = 24
    shard = Rank0(tr, n, n_local, overlap, chunks)
    shard.halo_max = halo_max
    g = dist.ShardedGraph(sym_edges() if kind == "symmetric" else dir_edges(), shard)
    tr.graph("row block", g)
    tr.note(f"symmetric={g.symmetric} n_local={g.n_local} t: {tr.fmt(list(g.transposed()))} t_long_segments={g.t_long_segments}")
    torch.manual_seed(4)
    x = torch.randn(n_local, 8).requires_grad_(True)
    for step in (1, 2):
        tr.note(f"-- step {step}")
        y = ops.spmm(g, x, shard)
        (y * torch.arange(8.0)).sum().backward()
        tr.sha("y", y), tr.sha("dx", x.grad)
        x.grad = None
    tr.note(f"last_halo={shard.last_halo} overlapped_exchanges={shard.overlapped_exchanges}")


def case_own_block(tr, mp, table, n_local=256, comm=True, locality=True, env=None):
    """The own block of a rank that holds every row (n_halo == 0), marked as dist.Repartition marks its graph."""
    from sgformer_amd import dist, ops
    for k, val in (env or {}).items():
        mp.setenv(k, val)
    _one_process_collectives(tr, mp)
    shard = Rank0(tr, n_local, n_local, True)
    g = dist.ShardedGraph(sym_edges(n_local), shard)
    if locality:
        g.locality = True
        g.comm_local = (torch.arange(n_local, dtype=torch.int32) // 64).contiguous() if comm else None
    tr.graph("row block", g)
    x = torch.zeros(n_local, 128, dtype=_BF16)
    for title, xx in (("first", x), ("second", x), ("fp32", x.float()), ("transposed", None)):
        tr.note(f"-- {title} call")
        if xx is None:
            ops._sharded_spmm(g, x, shard, True)
        else:
            ops._sharded_spmm(g, xx, shard, False)


# ------------------------------------------------------------------------------------------------
# hints of the producers, caches
# ------------------------------------------------------------------------------------------------
def case_subgraph(tr, mp, table, env=None):
    from sgformer_amd import batching, ops
    for k, val in (env or {}).items():
        mp.setenv(k, val)
    batching._parents.clear()
    subset = torch.tensor([3, 4, 5, 8, 9, 10, 20])
    for name, ei in (("symmetric parent", sym_edges()), ("directed parent", dir_edges())):
        tr.note(f"-- {name}")
        out, attr = batching.subgraph(subset, ei, relabel_nodes=True, num_nodes=24)
        tr.note(f"edges {tr.fmt(out)} attr={attr}")
        _note_hints(tr, "relabelled", out)
        g = ops.CSRGraph(out, int(subset.numel()))
        g.transposed()
        tr.graph("batch", g), tr.sha("val", g.val)
        tr.note(f"symmetric={g.symmetric}")
    out, attr = batching.subgraph(subset, sym_edges(), relabel_nodes=False, num_nodes=24)
    _note_hints(tr, "not relabelled", out)
    out, attr = batching.subgraph(subset.tolist(), sym_edges(), torch.arange(120.0), relabel_nodes=True, num_nodes=24)
    tr.note(f"with attributes: {tr.fmt(attr)}")
    _note_hints(tr, "with attributes", out)
    batching._parents.clear()


def case_sampled_batch_to(tr, mp, table):
    from sgformer_amd import sampling
    ei = dir_edges()
    pre = CpuKernels.csr_build(ei, 24)
    _hint(ei, trusted=True, max_in_degree=3, csr=pre, csr_t_lazy=True)
    b = sampling.SampledBatch(torch.zeros(24, 4), ei, torch.zeros(24, dtype=torch.int64), 5, torch.arange(24))
    same = b.to("cpu")
    tr.note(f"to(cpu): the same edge list: {same.edge_index is ei}, batch_size={same.batch_size} num_nodes={same.num_nodes}")
    _note_hints(tr, "to(cpu)", same.edge_index)
    moved = b.to("meta")
    h = _hints(moved.edge_index)
    tr.note(f"to(meta): edge list on {moved.edge_index.device.type}, x on {moved.x.device.type}")
    tr.note("hints to(meta): " + ", ".join(
        f"{k}={[(t.device.type, list(t.shape)) for t in h[k]] if k == 'csr' else h[k]}" for k in FIELDS))
    plain = sampling.SampledBatch(torch.zeros(24, 4), dir_edges(), None, 5, torch.arange(24)).to("meta")
    _note_hints(tr, "no hints, to(meta)", plain.edge_index)


def case_long_bound(tr, mp, table):
    from sgformer_amd import graphed, ops
    L = ops.LONG_ROW
    for name, ei in (("no hint", dir_edges()), ("hint LONG_ROW", _hint(dir_edges(), max_in_degree=L)),
                     ("hint LONG_ROW + 1", _hint(dir_edges(), max_in_degree=L + 1)), ("hint 0", _hint(dir_edges(), max_in_degree=0))):
        tr.note(f"_long_bound, {name}: {[graphed._long_bound(ei, cap) for cap in (1024, 5000, 131072)]}")


def case_weighted_cache(tr, mp, table):
    from sgformer_amd import ops
    ei, w = dir_edges(), torch.linspace(0.5, 2.0, 51)
    built = []

    def value_fn(e, ew, n):
        built.append(n)
        return e, ew * 2.0

    def keys():
        return [(k[1:6], k[6] and (k[6][0],) + k[6][2:]) for k in ops.graph_cache._d]

    g1 = ops.weighted_graph(ei, w, 24, value_fn, "gcn")
    g2 = ops.weighted_graph(ei, w, 24, value_fn, "gcn")
    tr.note(f"same pair twice: one graph: {g1 is g2}, built {len(built)}; keys {keys()}")
    g3 = ops.weighted_graph(ei, w, 24, value_fn, "dif")
    tr.note(f"another tag: new graph: {g3 is not g1}, built {len(built)}; keys {keys()}")
    w.mul_(2.0)
    g4 = ops.weighted_graph(ei, w, 24, value_fn, "gcn")
    tr.note(f"weights changed in place: new graph: {g4 is not g1}, built {len(built)}; keys {keys()}")
    tr.note(f"pins: {g4.edge_weight_ref is w} {g4.edge_index_ref is ei}")
    plain = ops.graph_cache.get(ei, 24)
    tr.note(f"the unweighted graph of the same list is another entry: {type(plain).__name__}; entries {len(ops.graph_cache._d)} "
            f"of {ops.graph_cache.capacity}")
    ops.graph_cache.get(ei.clone(), 24)
    tr.note(f"a fifth key: entries {len(ops.graph_cache._d)}, oldest gone: {all(g is not g1 for g in ops.graph_cache._d.values())}")


def case_graph_for(tr, mp, table):
    from sgformer_amd import dist, ops
    _one_process_collectives(tr, mp)
    shard = Rank0(tr, 24, 24, True)
    carried = dist.ShardedGraph(sym_edges(), shard)
    ei = _hint(sym_edges(), trusted=True, sharded_graph=carried)
    tr.note(f"carried graph returned: {dist.ShardContext.graph_for(shard, ei) is carried}, cache entries {len(ops.graph_cache._d)}")
    other = sym_edges()
    g = dist.ShardContext.graph_for(shard, other)
    tr.note(f"no hint: {type(g).__name__} from the cache, the same again: {dist.ShardContext.graph_for(shard, other) is g}; "
            f"key node count {[k[5] for k in ops.graph_cache._d]}")


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
def _c(fn, table="cpu", **kw):
    return fn, table, kw


_SGF_ERROR = "SgfError"
CASES = {
    "build-symmetric": _c(case_build, kind="symmetric"),
    "build-directed": _c(case_build, kind="directed"),
    "long-segments": _c(case_long_segments),
    "hint-trusted": _c(case_hint_trusted, table=dict(canned_csr=True)),
    "hint-csr": _c(case_hint_csr),
    "hint-lazy": _c(case_hint_lazy, combo=False),
    "hint-lazy-sampler-combination": _c(case_hint_lazy, combo=True),
    "hint-symmetric": _c(case_hint_symmetric, combo=False),
    "hint-symmetric-subgraph-combination": _c(case_hint_symmetric, combo=True),
    # CSRGraph.view / GraphView.decide
    "view-cpu-table": _c(case_view, mode="always"),
    "view-env-0": _c(case_view, table=FakeHip(), env={"SGF_REORDER": "0"}, calls=(False, True)),
    "view-env-1": _c(case_view, table=FakeHip(), env={"SGF_REORDER": "1"}, min_nodes=None),
    "view-unset-small-graph": _c(case_view, table=FakeHip(), min_nodes=None, calls=(False, False, True)),
    "view-mode-never-over-env-1": _c(case_view, table=FakeHip(), env={"SGF_REORDER": "1"}, mode="never"),
    "view-mode-always-over-env-0": _c(case_view, table=FakeHip(), env={"SGF_REORDER": "0"}, mode="always", min_nodes=None),
    "view-mode-auto-over-env-1": _c(case_view, table=FakeHip(), env={"SGF_REORDER": "1"}, mode="auto", min_nodes=None),
    "view-auto-second-forward": _c(case_view, table=FakeHip(), calls=(False, False)),
    "view-auto-now": _c(case_view, table=FakeHip(), calls=(True,)),
    "view-auto-directed": _c(case_view, table=FakeHip(), calls=(True,), kind="directed"),
    "view-fraction-below": _c(case_view, table=FakeHip(tile=(249, 1)), calls=(True,)),
    "view-fraction-above": _c(case_view, table=FakeHip(tile=(251, 1)), calls=(True,)),
    "view-always-fraction-below": _c(case_view, table=FakeHip(tile=(249, 1)), mode="always", min_nodes=None),
    "view-sparse-tiles": _c(case_view, table=FakeHip(tile=(300, 5)), calls=(True,)),
    "view-sparse-tiles-env-tile": _c(case_view, table=FakeHip(tile=(300, 5)), env={"SGF_SPMM_TILE": "512,2,128"}, calls=(True,)),
    "view-plan-value-error": _c(case_view, table=FakeHip(plan_error=ValueError("row block out of range")), calls=(True,)),
    "view-plan-sgf-error": _c(case_view, table=FakeHip(plan_error=_SGF_ERROR), calls=(True,)),
    "view-env-blocked": _c(case_view, table=FakeHip(), env={"SGF_SPMM_BLOCKED": "1"}, calls=(True,)),
    "view-env-tiled-0": _c(case_view, table=FakeHip(), env={"SGF_SPMM_TILED": "0"}, calls=(True,)),
    "view-env-blocked-and-tiled": _c(case_view, table=FakeHip(), env={"SGF_SPMM_BLOCKED": "1", "SGF_SPMM_TILED": "1"}, calls=(True,)),
    # spmm_on / spmm / spmm_packed_slot
    "spmm-on-symmetric": _c(case_spmm_on, table=FakeHip(), kind="symmetric"),
    "spmm-on-directed": _c(case_spmm_on, table=FakeHip(), kind="directed"),
    "packed-slot-hip": _c(case_packed_slot, table=FakeHip()),
    "packed-slot-hip-no-entry": _c(case_packed_slot, table=FakeHip(packed=False)),
    "packed-slot-cpu-table": _c(case_packed_slot),
    "autograd": _c(case_autograd),
    # _sharded_spmm / _own_block_spmm
    "sharded-halo-overlap": _c(case_sharded, kind="symmetric", n_local=16),
    "sharded-halo-overlap-directed": _c(case_sharded, kind="directed", n_local=16),
    "sharded-halo-no-overlap": _c(case_sharded, kind="directed", n_local=16, overlap=False),
    "sharded-halo-empty": _c(case_sharded, kind="directed", n_local=24),
    "sharded-all-gather": _c(case_sharded, kind="directed", n_local=16, halo_max=0.0),
    "sharded-all-gather-chunks": _c(case_sharded, kind="symmetric", n_local=16, halo_max=0.0, chunks=2),
    "own-block-tile-adopted": _c(case_own_block, table=FakeHip(tile=(251, 1))),
    "own-block-fraction-low": _c(case_own_block, table=FakeHip(tile=(249, 1))),
    "own-block-plan-value-error": _c(case_own_block, table=FakeHip(plan_error=ValueError("row block out of range"))),
    "own-block-plan-sgf-error": _c(case_own_block, table=FakeHip(plan_error=_SGF_ERROR)),
    "own-block-small": _c(case_own_block, table=FakeHip(), n_local=255),
    "own-block-env-tiled-0": _c(case_own_block, table=FakeHip(), env={"SGF_SPMM_TILED": "0"}),
    "own-block-no-labels": _c(case_own_block, table=FakeHip(), comm=False),
    "own-block-no-locality": _c(case_own_block, table=FakeHip(), locality=False),
    "own-block-cpu-table": _c(case_own_block, n_local=256),
    # hints of the producers, caches
    "subgraph-no-entry": _c(case_subgraph),
    "subgraph-csr": _c(case_subgraph, table=dict(with_subgraph_csr=True)),
    "subgraph-csr-env-0": _c(case_subgraph, table=dict(with_subgraph_csr=True), env={"SGF_SUBGRAPH_CSR": "0"}),
    "sampled-batch-to": _c(case_sampled_batch_to),
    "long-bound": _c(case_long_bound),
    "weighted-graph-cache": _c(case_weighted_cache),
    "graph-for": _c(case_graph_for),
}


def run_case(name, monkeypatch):
    from sgformer_amd import _lib, ops
    fn, table, kw = CASES[name]
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    if isinstance(table, FakeHip):
        table = FakeHip(table.tile, table.plan_error, hasattr(table, "spmm_packed_supported"))     # (a fresh one per run)
        if table.plan_error is _SGF_ERROR:
            table.plan_error = _lib.SgfError("sgf_spmm_tile_plan: nnz beyond 32-bit offsets")
    else:
        table = CpuTable(**(table if isinstance(table, dict) else {}))
    tr = Trace()
    threads = torch.get_num_threads()
    prev = ops.set_kernels(Recording(table, tr))
    torch.set_num_threads(1)
    try:
        fn(tr, monkeypatch, table, **kw)
        return tr.lines
    finally:
        torch.set_num_threads(threads)
        ops.set_kernels(prev)


def _load():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("name", list(CASES))
def test_trace_matches_the_golden_file(name, monkeypatch):
    want = _load()[name]
    got = run_case(name, monkeypatch)
    first = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (f"{name}: {len(got)} lines for {len(want)}; first difference at line {first}: "
                         f"{got[first:first + 1]} for {want[first:first + 1]}")


def test_golden_file_holds_exactly_the_cases():
    assert sorted(_load()) == sorted(CASES)


def test_arms_the_issue_names_are_reached():
    """Every kernel-table entry of the graph layer and every arm of spmm_on is in the pinned traces, and the decisions the
    cases are named after were the ones taken."""
    golden = _load()

    def names(case):
        return {line.split("(")[0] for line in golden[case] if not line.startswith("note")}

    def has(case, text):
        return any(text in line for line in golden[case])

    assert {"spmm", "spmm_blocked", "spmm_tile", "spmm_packed", "spmm_plan", "tile_plan", "tile_pack", "tile_supported",
            "lds_rows_max", "csr_build", "csr_transpose"} <= names("spmm-on-directed")
    assert has("spmm-on-symmetric", "stream_hint=True") and "csr_transpose" in names("spmm-on-symmetric")
    assert {"reorder", "tile_blocks", "tile_plan", "tile_pack", "csr_build"} <= names("view-auto-now")
    for case in ("hint-lazy", "hint-lazy-sampler-combination"):
        assert sum(line.startswith("sampled_csr_transpose") for line in golden[case]) == 1 and has(case, "symmetric is False: True")
    assert names("hint-symmetric") == {"csr_build"} == names("hint-symmetric-subgraph-combination")      # (no csr_transpose)
    assert [sum(line.startswith("csr_build") for line in golden[case])
            for case in ("hint-symmetric", "hint-symmetric-subgraph-combination")] == [2, 1]
    assert sum(line.startswith("csr_build") for line in golden["hint-csr"]) == 3
    assert sum(line.startswith("tile_plan") for line in golden["view-sparse-tiles"]) == 2
    assert sum(line.startswith("tile_plan") for line in golden["view-sparse-tiles-env-tile"]) == 1
    assert has("view-fraction-below", "'no reuse to exploit'") and has("view-fraction-above", "stats['reordered'] = True")
    assert has("view-always-fraction-below", "stats['reordered'] = True") and has("view-unset-small-graph", "'small graph'")
    assert has("view-plan-sgf-error", "tile plan unsupported") and has("view-plan-value-error", "tile plan unsupported")
    assert has("view-env-blocked", "row-block (LDS-staged)") and has("view-env-tiled-0", "stats['kernel'] = 'stream'")
    assert "shard.halo_exchange_start" in names("sharded-halo-overlap") and "shard.halo_exchange" in names("sharded-halo-no-overlap")
    assert "shard.all_gather_rows" in names("sharded-all-gather") and has("sharded-all-gather-chunks", "async_op=True")
    assert names("sharded-halo-empty").isdisjoint({"shard.halo_exchange", "shard.halo_exchange_start", "shard.all_gather_rows"})
    assert sum(line.startswith("tile_plan") for line in golden["own-block-tile-adopted"]) == 1 and \
        sum(line.startswith("spmm_tile") for line in golden["own-block-tile-adopted"]) == 3
    for case in ("own-block-fraction-low", "own-block-plan-value-error", "own-block-plan-sgf-error"):
        assert "spmm_tile" not in names(case) and sum(line.startswith("tile_blocks") for line in golden[case]) == 1
    for case in ("own-block-small", "own-block-env-tiled-0", "own-block-no-labels", "own-block-no-locality"):
        assert "tile_blocks" not in names(case)
    assert not has("own-block-no-locality", "stream_hint=True") and has("own-block-small", "stream_hint=True")
    assert "subgraph_csr" in names("subgraph-csr") and "subgraph_csr" not in names("subgraph-csr-env-0")


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_graph_trace_host.py --write")
    out = {}
    for case_name in CASES:
        with pytest.MonkeyPatch.context() as mp:
            out[case_name] = run_case(case_name, mp)
    with open(GOLDEN, "w") as fh:
        fh.write("{\n" + ",\n".join(f"{json.dumps(k)}: [\n" + ",\n".join(json.dumps(s) for s in v) + "\n]"
                                    for k, v in out.items()) + "\n}\n")
    print(f"wrote {os.path.relpath(GOLDEN, ROOT)}: {len(out)} cases, {sum(len(v) for v in out.values())} lines, "
          f"{os.path.getsize(GOLDEN)} bytes")
