"""The kernel table: one thin ctypes method per entry point of the libsgf C ABI (include/sgf.h), tensors in / tensors out,
on the current HIP stream.  Split out of ops.py in r05 (ops.py keeps the autograd-level operators built on this table).
PyTorch supplies memory and streams only; a CPU tensor or a missing library raises — there is no eager fallback.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

from . import _lib

_F32 = torch.float32
_BF16 = torch.bfloat16

# rows of the normalised adjacency longer than this are split into segments reduced by whole workgroups (sgf_spmm_split)
LONG_ROW = 1024
_SEGMENT = 1024   # = sgf_spmm_segment_len()

# launches by entry, for the tests that have to see which path a step took
counters = {"spmm_packed": 0, "spmm_coded": 0}


class PackedRows:
    """The packed copy of a bf16 [n, 256] operand (include/sgf.h, sgf_spmm_packed): `slots` uint8, slot_bytes per row plus
    the tail the gather may read; `overflow` device int32 [1], the rows that did not fit their slot."""
    __slots__ = ("slots", "slot_bytes", "n", "overflow")

    def __init__(self, slots, slot_bytes, n, overflow):
        self.slots, self.slot_bytes, self.n, self.overflow = slots, slot_bytes, n, overflow


# ------------------------------------------------------------------------------------------------
# plumbing
# ------------------------------------------------------------------------------------------------
def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream_handle(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _stream(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(_stream_handle(device))


def _dtype_code(dtype) -> int:
    if dtype == _F32:
        return _lib.SGF_F32
    if dtype == _BF16:
        return _lib.SGF_BF16
    raise TypeError(f"sgformer_amd kernels take float32 or bfloat16 storage, got {dtype}")


def _code(t: torch.Tensor) -> int:
    return _dtype_code(t.dtype)


# torch.set_float32_matmul_precision('high' | 'medium') (also set by torch.backends.cuda.matmul.allow_tf32 = True and by
# TORCH_ALLOW_TF32_CUBLAS_OVERRIDE=1) allows fp32 matrix products "as the sum of two bfloat16 numbers": the entries that
# accept SGF_F32_BF16X3 then form them as three bf16 matrix-core products (include/sgf.h).  This module is the only place
# that reads the setting.  torch.get_float32_matmul_precision() is the source of truth: on torch 2.10 the newer
# torch.backends.cuda.matmul.fp32_precision = 'ieee' does not reset it, so set the precision itself to go back.
_X3_PRECISIONS = ("high", "medium")


def f32_matmul_code() -> int:
    """The dtype code of fp32 matrix products under the current torch setting: SGF_F32_BF16X3 or SGF_F32."""
    return _lib.SGF_F32_BF16X3 if torch.get_float32_matmul_precision() in _X3_PRECISIONS else _lib.SGF_F32


_x3_cache: "dict[tuple, bool]" = {}


def _mm_code(t: torch.Tensor, query: Optional[str] = None, *shape) -> int:
    """_code(t) for an operand of a matrix product: fp32 storage asks for SGF_F32_BF16X3 when the setting allows it and
    the entry's *_supported query (if it has one) accepts the code for this shape; otherwise SGF_F32."""
    code = _code(t)
    if code != _lib.SGF_F32 or f32_matmul_code() != _lib.SGF_F32_BF16X3:
        return code
    if query is None:
        return _lib.SGF_F32_BF16X3
    key = (query,) + tuple(int(v) for v in shape)
    ok = _x3_cache.get(key)
    if ok is None:
        ok = _x3_cache[key] = bool(getattr(_lib.load(), query)(*key[1:], _lib.SGF_F32_BF16X3))
    return _lib.SGF_F32_BF16X3 if ok else _lib.SGF_F32


def _ld(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.stride(0)


def _rows(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """A view/copy of a 2-D tensor whose rows are contiguous and 4-element aligned."""
    if t is None:
        return None
    if t.stride(-1) != 1 or t.stride(0) % 4 != 0 or t.data_ptr() % (4 * t.element_size()) != 0:
        t = t.contiguous()
        if t.shape[0] > 1 and t.stride(0) % 4 != 0:
            raise ValueError(f"feature dimension {t.shape[-1]} must be a multiple of 4")
    return t


_workspaces: "dict[tuple, torch.Tensor]" = {}


_capture_scope = None      # {(device index, name): tensor} while sgformer_amd.graphed captures a step, else None


def begin_capture_scope() -> dict:
    """Scratch requested while a step is being captured comes out of the graph's PRIVATE pool and its address is baked into
    the captured launches: it must live exactly as long as those graphs.  A process-wide cache keyed on the stream does the
    opposite — every capture runs on torch's one capture stream, so a later capture (another model, another batch size)
    would be handed scratch from an earlier graph's pool, and once that graph is destroyed the captured kernels write into
    unmapped memory (r06: `Memory access fault` in the eighth test of tests/test_gpu_graphed.py, never in isolation).  The
    caller keeps the returned dict with the captured step."""
    global _capture_scope
    _capture_scope = {}
    return _capture_scope


def end_capture_scope():
    global _capture_scope
    _capture_scope = None


class SeedBank:
    """The dropout seeds of ONE captured step (sgformer_amd.graphed): a device int64 tensor, one slot per dropout call of the
    forward in call order.  While a bank is the active seed scope, ops.dropout_res draws nothing from torch's generator: it
    takes the next slot and launches sgf_dropout_dev, which reads the seed from that slot when the kernel runs.  The owner
    rewrites slots [0, used) before every replay."""

    def __init__(self, device, capacity: int = 64):
        self.seeds = torch.zeros(int(capacity), dtype=torch.int64, device=device)
        self.used = 0

    def take(self) -> int:
        if self.used >= self.seeds.numel():
            raise RuntimeError(f"sgformer_amd: more than {self.seeds.numel()} dropout calls in one captured step")
        self.used += 1
        return self.used - 1


_seed_scope = None         # the SeedBank of the step being captured, else None


def begin_seed_scope(bank: SeedBank) -> SeedBank:
    global _seed_scope
    _seed_scope = bank
    return bank


def end_seed_scope():
    global _seed_scope
    _seed_scope = None


def seed_scope():
    return _seed_scope


def _fresh_bytes(device, nbytes: int) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _workspace(device, name: str, nbytes: int) -> torch.Tensor:
    """Per-device, per-stream scratch reused across calls (users run on that stream, in order)."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        if _capture_scope is None:           # somebody else's capture: fresh scratch from ITS pool, not cached here
            return _fresh_bytes(device, nbytes)
        cache, key = _capture_scope, (device.index, name)
    else:
        cache, key = _workspaces, (device.index, name, _stream_handle(device))
    ws = cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = cache[key] = _fresh_bytes(device, nbytes)
    return ws


_NO_SCRATCH = (None, 0)

_constant_bytes: "dict[str, int]" = {}


def _const_bytes(query: str, *args) -> int:
    """A byte count the library documents as constant (a block-partial buffer), asked once: the query is a measurable part
    of the host cost of the loss on a mini-batch (profiles/kernel_table_host_cost.md).  For those two only -- other
    *_workspace_bytes and *_supported answers depend on their arguments or on switches that sgf_reload_env() re-reads."""
    n = _constant_bytes.get(query)
    if n is None:
        n = _constant_bytes[query] = int(getattr(_lib.load(), query)(*args))
    return n


def _scratch(device, name: Optional[str], nbytes: int):
    """The (buffer, bytes) pair an entry takes as its scratch of `nbytes` for one call, to be spliced into _launch's
    arguments.  With a name: the cached buffer of that name (_workspace) -- the name is part of the contract, entries that
    run back to back share one on purpose and attn_h_bwd_pre leaves data in "attn_h_part" for attn_h_bwd_post.  With None:
    taken from the caching allocator and given back after the call, for buffers that are large and rarely needed (the
    once-per-graph plans, the evaluation metric).  An entry that needs none this time takes _NO_SCRATCH."""
    ws = _fresh_bytes(device, nbytes) if name is None else _workspace(device, name, nbytes)
    return ws, ws.numel()


def _long_row_scratch(device, long_segments: int, d: int):
    """The segment partials of the rows longer than LONG_ROW: one buffer for every SpMM family."""
    if long_segments <= 0:
        return _NO_SCRATCH
    return _scratch(device, "spmm_long", _lib.load().sgf_spmm_split_workspace_bytes(long_segments, d))


def _stats_scratch(device, n: int, d: int, want_stats: bool):
    """The block partials of the BatchNorm column sums that the Linear epilogues form on request."""
    if not want_stats:
        return _NO_SCRATCH
    return _scratch(device, "gcn_epi", _lib.load().sgf_gcn_epilogue_workspace_bytes(n, d))


_PLAIN = frozenset((int, float, bool, type(None)))
_Tensor = torch.Tensor


def _launch(device, name: str, *args):
    """Every call of a compute entry of libsgf leaves the package here: a tensor becomes its address and None stays the
    null pointer (the entry's c_void_p parameter type, _lib.SIGNATURES, converts both), everything else (ints, floats,
    ctypes arrays and byref, a pointer computed by hand) passes through, the current stream of `device` goes last.
    Some entries sit on paths whose GPU work is a few microseconds at mini-batch sizes, so the host side is one pass
    over the arguments (plain scalars, the majority, are recognised by their type alone; no ctypes object is built per
    pointer) and one ctypes call, with no device context switch when the tensors' device is already current."""
    argv = [a if type(a) in _PLAIN else (a.data_ptr() if isinstance(a, _Tensor) else a) for a in args]
    argv.append(_stream_handle(device))
    if torch.cuda.current_device() == device.index:
        _lib.call(name, *argv)
    else:
        with torch.cuda.device(device):
            _lib.call(name, *argv)


def _rows16(t: torch.Tensor) -> torch.Tensor:
    """Rows contiguous and 16-byte aligned (what the streaming row-GEMM loads as matrix-core fragments)."""
    if t.stride(-1) != 1 or (t.stride(0) * t.element_size()) % 16 != 0 or t.data_ptr() % 16 != 0:
        t = t.contiguous()
    return t


def _pair_gram() -> bool:
    return os.environ.get("SGF_GRAM_PAIR", "1") != "0"


def _one_pass_cat() -> bool:
    return os.environ.get("SGF_GCN_CAT", "1") != "0"


# ------------------------------------------------------------------------------------------------
# the kernel table: one method per C-ABI entry point, tensors in / tensors out
# ------------------------------------------------------------------------------------------------
class HipKernels:
    """libsgf.so on the current HIP stream.  Inputs must be GPU tensors."""

    name = "hip"

    @staticmethod
    def check(*tensors):
        for t in tensors:
            if t is not None and not t.is_cuda:
                raise RuntimeError(
                    "sgformer_amd runs on MI355X only: got a CPU tensor.  There is no CPU fallback; "
                    "move the model and its inputs to the GPU (the reference's CPU evaluation path, "
                    "large/eval.py:36-65, is outside this library's scope).")

    # ---- T1 ----
    @staticmethod
    def csr_build(ei: torch.Tensor, n: int):
        dev, nnz = ei.device, int(ei.shape[1])
        rowptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
        colind = torch.empty(nnz, dtype=torch.int32, device=dev)
        val = torch.empty(nnz, dtype=_F32, device=dev)
        deg = torch.empty(n, dtype=torch.int32, device=dev)
        _launch(dev, "sgf_csr_build", ei, nnz, n, rowptr, colind, val, deg,
                *_scratch(dev, None, _lib.load().sgf_csr_workspace_bytes(nnz, n)))
        return rowptr, colind, val, deg

    @staticmethod
    def csr_transpose(ei: torch.Tensor, n: int, deg, rowptr, colind):
        dev, nnz = ei.device, int(ei.shape[1])
        t_rowptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
        t_colind = torch.empty(nnz, dtype=torch.int32, device=dev)
        t_val = torch.empty(nnz, dtype=_F32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        _launch(dev, "sgf_csr_transpose", ei, nnz, n, deg, rowptr, colind, t_rowptr, t_colind, t_val, flag,
                *_scratch(dev, None, _lib.load().sgf_csr_workspace_bytes(nnz, n)))
        return t_rowptr, t_colind, t_val, bool(int(flag.item()))  # one host sync, once per graph

    # ---- N1: induced subgraph ----
    @staticmethod
    def subgraph(ei: torch.Tensor, n: int, subset: torch.Tensor, relabel_nodes: bool, want_eid: bool):
        """ei int64 [2, nnz] and subset int64 [m] on the GPU -> (edge_index_sub [2, k], eid [k] | None)."""
        dev, nnz, m = ei.device, int(ei.shape[1]), int(subset.numel())
        relabel = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        scratch = _scratch(dev, "subgraph", _lib.load().sgf_subgraph_workspace_bytes(nnz, n))
        _launch(dev, "sgf_subgraph_plan", ei, nnz, n, subset, m, relabel, total, *scratch)
        k = int(total.item())              # the one host sync: the output size
        out = torch.empty((2, k), dtype=torch.int64, device=dev)
        eid = torch.empty(k, dtype=torch.int64, device=dev) if want_eid else None
        _launch(dev, "sgf_subgraph_emit", ei, nnz, n, relabel, int(relabel_nodes), k, out, eid, *scratch)
        return out, eid

    @staticmethod
    def subgraph_csr(rowptr, colind, n: int, subset: torch.Tensor, local_of: torch.Tensor, want_edges: bool):
        """Induced subgraph + its normalised CSR from the parent CSR (sgf_subgraph_csr_*): (rowptr_b, colind_b, val_b, deg_b,
        edge_index_b | None, longest row), or None when `subset` repeats a node / leaves the graph (the caller takes
        sgf_subgraph_*)."""
        dev, m = rowptr.device, int(subset.numel())
        lib = _lib.load()
        rowptr_b = torch.empty(m + 1, dtype=torch.int64, device=dev)
        deg_b = torch.empty(m + 1, dtype=torch.int32, device=dev)
        total = torch.empty(3, dtype=torch.int64, device=dev)
        _launch(dev, "sgf_subgraph_csr_plan", rowptr, colind, n, subset, m, local_of, rowptr_b, deg_b, total,
                *_scratch(dev, "subgraph_csr_plan", lib.sgf_subgraph_csr_plan_workspace_bytes(m)))
        # the plan MARKED the parent's shared `local_of` table; only the emit call clears the marks again.  Whatever fails
        # in between (the host read, an allocation) must not leave them behind: later batches would pick up stale local
        # ids for nodes outside their subset.
        try:
            t, bad, longest = total.tolist()            # the one host read of the batch
            t = 0 if bad else int(t)
            colind_b = torch.empty(t, dtype=torch.int32, device=dev)
            val_b = torch.empty(t, dtype=_F32, device=dev)
            ei_b = torch.empty((2, t), dtype=torch.int64, device=dev) if want_edges else None
            scratch = _scratch(dev, "subgraph_csr_emit", lib.sgf_subgraph_csr_emit_workspace_bytes(m, t))
        except BaseException:
            local_of.fill_(-1)
            raise
        _launch(dev, "sgf_subgraph_csr_emit", rowptr, colind, n, subset, m, local_of, rowptr_b, deg_b, t, colind_b, val_b,
                ei_b, *scratch)
        if bad:
            return None
        return rowptr_b, colind_b, val_b, deg_b[:m], ei_b, int(longest)

    # ---- N2 + T1: the CSR of a neighbour-sampled batch and its transpose (csrc/sampled_csr.hip) ----
    @staticmethod
    def sampled_csr_supported(max_fanout: int) -> bool:
        return bool(_lib.load().sgf_sampled_csr_supported(int(max_fanout)))

    @staticmethod
    def sampled_csr_build(e_src: torch.Tensor, e_dst: torch.Tensor, counts: torch.Tensor, node_cap: int, edge_cap: int,
                          max_fanout: int):
        """Capacity-sized (rowptr_b [node_cap + 1], colind_b [edge_cap], val_b [edge_cap], deg_b [node_cap + 1]) of the batch
        sgf_neighbor_sample_batch left in e_src / e_dst / counts (all on the device: no host read here).  The caller slices
        the prefixes [:nn + 1], [:ne], [:ne], [:nn] once it has read the counts: those equal csr_build's arrays bit for bit."""
        dev = e_src.device
        rowptr_b = torch.empty(node_cap + 1, dtype=torch.int64, device=dev)
        colind_b = torch.empty(max(edge_cap, 1), dtype=torch.int32, device=dev)
        val_b = torch.empty(max(edge_cap, 1), dtype=_F32, device=dev)
        deg_b = torch.empty(node_cap + 1, dtype=torch.int32, device=dev)
        _launch(dev, "sgf_sampled_csr_build", e_src, e_dst, counts, node_cap, edge_cap, int(max_fanout), rowptr_b, colind_b,
                val_b, deg_b,
                *_scratch(dev, "sampled_csr_build", _lib.load().sgf_sampled_csr_build_workspace_bytes(node_cap, edge_cap)))
        return rowptr_b, colind_b, val_b, deg_b

    @staticmethod
    def sampled_csr_transpose(rowptr, colind, val, n: int):
        """(t_rowptr, t_colind, t_val) of a CSR whose rows are in ascending source order — csr_transpose's arrays bit for bit,
        without its symmetry flag: no host read."""
        dev, nnz = rowptr.device, int(colind.numel())
        t_rowptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
        t_colind = torch.empty(nnz, dtype=torch.int32, device=dev)
        t_val = torch.empty(nnz, dtype=_F32, device=dev)
        _launch(dev, "sgf_sampled_csr_transpose", rowptr, colind, val, n, nnz, t_rowptr, t_colind, t_val,
                *_scratch(dev, "sampled_csr_transpose", _lib.load().sgf_sampled_csr_transpose_workspace_bytes(n, nnz)))
        return t_rowptr, t_colind, t_val

    # ---- N2: trainer prologue (to_undirected / remove_self_loops / add_self_loops) ----
    @staticmethod
    def graph_prologue(ei: torch.Tensor, n: int, undirected: bool, remove_loops: bool, add_loops: bool):
        dev, m = ei.device, int(ei.shape[1])
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        scratch = _scratch(dev, None, _lib.load().sgf_graph_prologue_workspace_bytes(m, n))
        _launch(dev, "sgf_graph_prologue_plan", ei, m, n, int(undirected), int(remove_loops), int(add_loops), total, *scratch)
        k = int(total.item())              # the one host sync: the output size
        out = torch.empty((2, k), dtype=torch.int64, device=dev)
        _launch(dev, "sgf_graph_prologue_emit", m, n, int(undirected), int(add_loops), k, out, *scratch)
        return out

    # ---- T2 ----
    @staticmethod
    def spmm(rowptr, colind, val, x: torch.Tensor, n_rows: int, out: Optional[torch.Tensor] = None,
             long_segments: int = 0, stream_hint: bool = False) -> torch.Tensor:
        """`out`: optional [n_rows, d] destination, possibly a column slice of a wider buffer.
        `long_segments` > 0 (see long_row_segments): rows longer than LONG_ROW are split across
        workgroups (sgf_spmm_split).  `stream_hint`: the CSR's gathers mostly hit in L2 (re-ordered graph):
        sgf_spmm_stream."""
        x = _rows(x)
        d = x.shape[1]
        y = torch.empty((n_rows, d), dtype=x.dtype, device=x.device) if out is None else out
        if out is not None and (out.shape != (n_rows, d) or out.dtype != x.dtype or out.stride(1) != 1
                                or out.stride(0) % 4 != 0 or out.data_ptr() % (4 * out.element_size()) != 0):
            raise ValueError("spmm: `out` must be [n_rows, d], same dtype, row-contiguous and 4-element aligned")
        if n_rows == 0 or d == 0:
            return y
        if long_segments > 0 or stream_hint:
            _launch(x.device, "sgf_spmm_stream" if stream_hint else "sgf_spmm_split", rowptr, colind, val, x, x.stride(0),
                    x.shape[0], y, y.stride(0), n_rows, d, _code(x), LONG_ROW, long_segments,
                    *_long_row_scratch(x.device, long_segments, d))
        else:
            _launch(x.device, "sgf_spmm", rowptr, colind, val, x, x.stride(0), x.shape[0], y, y.stride(0), n_rows, d, _code(x))
        return y

    # ---- T2 gathering zero-elided operand rows (bf16, d = 256; csrc/spmm.hip: k_spmm_row_packed) ----
    @staticmethod
    def spmm_packed_supported(x_shape, dtype, slot_bytes: int) -> bool:
        """Would sgf_spmm_packed gather the slots for a contiguous operand of this shape (else it runs sgf_spmm_split's
        kernels on the dense rows)?  The launcher's own rule, SGF_SPMM_PACKED included."""
        n, d = int(x_shape[0]), int(x_shape[1])
        if dtype != _BF16 or n == 0:
            return False
        return bool(_lib.load().sgf_spmm_packed_supported(d, _dtype_code(dtype), d, d, n, 1, int(slot_bytes)))

    @staticmethod
    def spmm_packed(rowptr, colind, val, x: torch.Tensor, packed: "PackedRows", n_rows: int, long_segments: int = 0) -> torch.Tensor:
        """K.spmm(rowptr, colind, val, x, n_rows, long_segments=...) bit for bit, gathering `packed` (bn_apply_packed's copy of
        x) instead of x wherever the launch allows and no row overflowed its slot (decided on the device)."""
        x = _rows(x)
        d = x.shape[1]
        if packed.n != x.shape[0]:
            raise ValueError("spmm_packed: the packed copy has another number of rows than x")
        y = torch.empty((n_rows, d), dtype=x.dtype, device=x.device)
        if n_rows == 0 or d == 0:
            return y
        _launch(x.device, "sgf_spmm_packed", rowptr, colind, val, x, x.stride(0), x.shape[0], packed.slots, packed.slot_bytes,
                packed.overflow, y, y.stride(0), n_rows, d, _code(x), LONG_ROW, long_segments,
                *_long_row_scratch(x.device, long_segments, d))
        counters["spmm_packed"] += 1
        return y

    # ---- T2 with on-chip reuse: node order, row-block plan, LDS-staged SpMM ----
    @staticmethod
    def reorder(ei: torch.Tensor, n: int, iters1: int, iters2: int):
        """perm (new position -> old id), inv (old id -> new position), community: int32 [n] each."""
        dev, nnz = ei.device, int(ei.shape[1])
        perm = torch.empty(n, dtype=torch.int32, device=dev)
        inv = torch.empty(n, dtype=torch.int32, device=dev)
        comm = torch.empty(n, dtype=torch.int32, device=dev)
        _launch(dev, "sgf_reorder", ei, nnz, n, int(iters1), int(iters2), perm, inv, comm,
                *_scratch(dev, None, _lib.load().sgf_reorder_workspace_bytes(nnz, n)))
        return perm, inv, comm

    @staticmethod
    def spmm_plan(rowptr, colind, val, n: int, rows_per_block: int, lds_rows: int, long_len: int):
        dev, nnz = rowptr.device, int(colind.numel())
        nb = (n + rows_per_block - 1) // rows_per_block
        ecode = torch.empty(nnz, dtype=torch.int32, device=dev)
        ev = torch.empty(nnz, dtype=_F32, device=dev)
        nlds = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        sh_ptr = torch.empty(nb + 1, dtype=torch.int32, device=dev)
        sh_cols = torch.empty(max(nb * lds_rows, 1), dtype=torch.int32, device=dev)
        stats = torch.zeros(4, dtype=torch.int64, device=dev)
        _launch(dev, "sgf_spmm_plan", rowptr, colind, val, n, nnz, int(rows_per_block), int(lds_rows), int(long_len), ecode, ev,
                nlds, sh_ptr, sh_cols, stats,
                *_scratch(dev, None, _lib.load().sgf_spmm_plan_workspace_bytes(nnz, n, rows_per_block)))
        st = [int(v) for v in stats.tolist()]                      # one host sync, once per plan
        return ecode, ev, nlds, sh_ptr, sh_cols[: max(st[1], 1)].clone(), st

    @staticmethod
    def spmm_blocked(rowptr, plan, x: torch.Tensor, n_rows: int, out: Optional[torch.Tensor] = None,
                     long_segments: int = 0) -> torch.Tensor:
        x = _rows(x)
        d = x.shape[1]
        y = torch.empty((n_rows, d), dtype=x.dtype, device=x.device) if out is None else out
        if n_rows == 0 or d == 0:
            return y
        _launch(x.device, "sgf_spmm_blocked", rowptr, plan.ecode, plan.eval, plan.nlds, plan.sh_ptr, plan.sh_cols, x, x.stride(0),
                y, y.stride(0), n_rows, d, _code(x), plan.rows_per_block, plan.lds_rows, LONG_ROW, long_segments,
                *_long_row_scratch(x.device, long_segments, d))
        return y

    # ---- T2 on a re-ordered graph: dense matrix-core tiles + gather remainder (csrc/spmm_tile.hip) ----
    @staticmethod
    def tile_supported(d: int, dtype) -> bool:
        return dtype in (_BF16, _F32) and bool(_lib.load().sgf_spmm_tile_supported(int(d), _dtype_code(dtype)))

    @staticmethod
    def tile_blocks(comm_sorted: Optional[torch.Tensor], n: int, max_rows: int, device) -> torch.Tensor:
        """blk_row int32 [nb + 1]: row blocks that follow the communities (comm_sorted[p] = community of new row p)."""
        cap = 4 * n // int(max_rows) + 4
        blk = torch.empty(cap + 1, dtype=torch.int32, device=device)
        nb = ctypes.c_int64(0)
        _launch(device, "sgf_spmm_tile_blocks", comm_sorted, n, int(max_rows), blk, cap, ctypes.byref(nb))
        return blk[: nb.value + 1].clone()

    @staticmethod
    def tile_plan(rowptr, colind, val, n: int, blk_row: torch.Tensor, cap: int, min_count: int, long_len: int):
        """(sh_ptr, sh_cols, tile_ptr, tiles, rem_rowptr, rem_col, rem_val, stats) — see include/sgf.h."""
        dev, nnz, nb = rowptr.device, int(colind.numel()), int(blk_row.numel()) - 1
        ecode = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
        ev = torch.empty(max(nnz, 1), dtype=_F32, device=dev)
        nlds = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        sh_ptr = torch.empty(nb + 1, dtype=torch.int32, device=dev)
        sh_cols = torch.empty(max(nb * cap, 1), dtype=torch.int32, device=dev)
        tile_ptr = torch.empty(nb + 1, dtype=torch.int64, device=dev)
        rem_rowptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
        stats = torch.zeros(8, dtype=torch.int64, device=dev)
        _launch(dev, "sgf_spmm_tile_plan", rowptr, colind, val, n, nnz, blk_row, nb, int(cap), int(min_count), int(long_len),
                ecode, ev, nlds, sh_ptr, sh_cols, tile_ptr, rem_rowptr, stats,
                *_scratch(dev, None, _lib.load().sgf_spmm_tile_plan_workspace_bytes(nnz, n, nb)))
        st = [int(v) for v in stats.tolist()]                      # one host sync, once per plan; the scratch is free again
        if st[7]:
            raise ValueError("tile_plan: a row block is empty or longer than 256 rows")
        n_frag, n_rem = st[4], st[5]
        tiles = torch.empty(max(n_frag, 1) * 512, dtype=torch.int32, device=dev)     # 2 KiB per fragment
        rem_col = torch.empty(max(n_rem, 1), dtype=torch.int32, device=dev)
        rem_val = torch.empty(max(n_rem, 1), dtype=_F32, device=dev)
        _launch(dev, "sgf_spmm_tile_fill", rowptr, ecode, ev, nlds, n, nnz, blk_row, nb, tile_ptr, n_frag, rem_rowptr, tiles,
                rem_col, rem_val)
        return sh_ptr, sh_cols[: max(st[1], 1)].clone(), tile_ptr, tiles, rem_rowptr, rem_col, rem_val, st

    @staticmethod
    def tile_pack(blk_row: torch.Tensor, tile_ptr: torch.Tensor, tiles: torch.Tensor, n_frag: int):
        """(grp int32 [n_frag / 2, 2], pool uint8): the fragments as the kernel streams them — sparse groups as 8-byte
        entries, dense ones as they are (csrc/spmm_pack.hip, include/sgf.h)."""
        dev, nb = tiles.device, int(blk_row.numel()) - 1
        ng = n_frag // 2
        grp = torch.zeros((max(ng, 1), 2), dtype=torch.int32, device=dev)
        units = torch.zeros(1, dtype=torch.int64, device=dev)
        _launch(dev, "sgf_spmm_tile_pack_layout", blk_row, nb, tile_ptr, tiles, n_frag, grp, units,
                *_scratch(dev, None, _lib.load().sgf_spmm_tile_pack_workspace_bytes(n_frag)))
        nu = int(units.item())                                      # one host sync, once per plan
        pool = torch.zeros(nu * 16 + 4096, dtype=torch.uint8, device=dev)   # the kernel fetches whole KiB
        _launch(dev, "sgf_spmm_tile_pack", blk_row, nb, tile_ptr, tiles, n_frag, grp, pool, nu)
        return grp, pool, nu

    @staticmethod
    def spmm_tile(plan, x: torch.Tensor, n_rows: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _rows16(x)
        d = x.shape[1]
        y = torch.empty((n_rows, d), dtype=x.dtype, device=x.device) if out is None else out
        if n_rows == 0 or d == 0:
            return y
        segs = plan.long_segments
        _launch(x.device, "sgf_spmm_tile", plan.blk_row, plan.nb, plan.block_rows, plan.sh_ptr, plan.sh_cols, plan.tile_ptr,
                plan.grp, plan.pool, plan.rem_rowptr, plan.rem_col, plan.rem_val, x, x.stride(0), x.shape[0], y, y.stride(0),
                n_rows, d, _code(x), LONG_ROW, segs, *_long_row_scratch(x.device, segs, d))
        return y

    @staticmethod
    def lds_rows_max(dtype) -> int:
        code = _dtype_code(dtype)
        return int(_lib.load().sgf_spmm_lds_rows_len(code))

    @staticmethod
    def gather_rows(src: torch.Tensor, idx: torch.Tensor, out_dtype=None) -> torch.Tensor:
        """out[i] = src[idx[i]] (idx int32 / int64 on the GPU), optionally cast fp32 <-> bf16 on the way."""
        if src.stride(-1) != 1:
            src = src.contiguous()
        n_out, d = int(idx.numel()), src.shape[1]
        out = torch.empty((n_out, d), dtype=out_dtype or src.dtype, device=src.device)
        _launch(src.device, "sgf_gather_rows", src, src.stride(0), _code(src), src.shape[0], idx, int(idx.dtype == torch.int64),
                n_out, d, out, out.stride(0), _code(out))
        return out

    @staticmethod
    def pad_rows(src: torch.Tensor, idx: Optional[torch.Tensor], d_pad: int, out_dtype=None) -> torch.Tensor:
        """out[i, :d] = src[idx[i] if idx is given else i, :d], out[i, d:d_pad] = 0, optionally cast fp32 <-> bf16 — the
        aligned copy of features whose width is not a multiple of 4 (sgf_pad_rows)."""
        if src.stride(-1) != 1:
            src = src.contiguous()
        n_out = int(src.shape[0] if idx is None else idx.numel())
        d = src.shape[1]
        out = torch.empty((n_out, d_pad), dtype=out_dtype or src.dtype, device=src.device)
        _launch(src.device, "sgf_pad_rows", src, src.stride(0), _code(src), src.shape[0], idx,
                int(idx is not None and idx.dtype == torch.int64), n_out, d, d_pad, out, out.stride(0), _code(out))
        return out

    # ---- T4: the general Linear (any shape, any alignment; csrc/gemm.hip) ----
    @staticmethod
    def gemm(a: torch.Tensor, b: torch.Tensor, bias=None, out=None, out_dtype=None, alpha: float = 1.0, alpha_dev=None,
             beta: float = 0.0, addend=None) -> torch.Tensor:
        """out[m, n] = alpha * a[m, k] @ b[k, n] + bias + beta * addend — a, b any 2-D VIEWS (strides are passed on, so
        x @ w.t() costs no copy), fp32 or bf16 storage each; out: given, or new in out_dtype (default: a's dtype)."""
        m, k = a.shape
        k2, n = b.shape
        if k != k2:
            raise RuntimeError(f"gemm: inner dimensions differ: {tuple(a.shape)} x {tuple(b.shape)}")
        dev = a.device
        if out is None:
            out = torch.empty((m, n), dtype=out_dtype or a.dtype, device=dev)
        elif out.stride(-1) != 1 and n > 1:
            raise RuntimeError("gemm: out must have contiguous rows")
        if addend is not None and (addend.stride(-1) != 1 and n > 1):
            addend = addend.contiguous()
        _launch(dev, "sgf_gemm", a, a.stride(0), a.stride(1), _code(a), b, b.stride(0), b.stride(1), _code(b), m, n, k,
                float(alpha), alpha_dev, bias, float(beta), addend, 0 if addend is None else max(addend.stride(0), n),
                0 if addend is None else _code(addend), out, max(out.stride(0), n), _code(out))
        return out

    # ---- T3: the d x d algebra of the attention as one call each way (csrc/attn_small.hip) ----
    @staticmethod
    def attn_h_small_fwd(G, s, n_rows: float, n_total: float, wq, bq, wk, bk, wv, bv):
        """(M [D, d], m [d], w [D], beta [1], saved) from the Gram matrix G = h^T h [D, D], s = sum_n h_n and the three
        projections' fp32 weights [d, D] / biases [d] (wv None: V = h)."""
        d, D = wq.shape
        dev = G.device
        wb = [t if (t is None or (t.dtype == _F32 and t.is_contiguous())) else t.float().contiguous()
              for t in (wq, bq, wk, bk, wv, bv)]
        G = G if (G.dtype == _F32 and G.stride(-1) == 1) else G.float().contiguous()
        s = s if (s.dtype == _F32 and s.is_contiguous()) else s.float().contiguous()
        M = torch.empty((D, d), dtype=_F32, device=dev)
        mwb = torch.empty(d + D + 1, dtype=_F32, device=dev)
        saved = torch.empty(_lib.load().sgf_attn_h_small_saved_bytes(D, d), dtype=torch.uint8, device=dev)
        m, w, beta = mwb[:d], mwb[d:d + D], mwb[d + D:]
        _launch(dev, "sgf_attn_h_small_fwd", G, G.stride(0), s, float(n_rows), float(n_total), *wb, D, D, d, M, d, m, w, beta,
                saved, saved.numel())
        return M, m, w, beta, saved

    @staticmethod
    def attn_h_small_bwd(dM, dw, dm, dbeta, n_total: float, saved, d_in: int, d_out: int, want_v: bool = True):
        """(D = dG + dG^T [D, D], ds [D], gwq, gbq, gwk, gbk, gwv | None, gbv | None) from the reduced gradients of
        M, w, m, beta (the blocks of hstats) and what attn_h_small_fwd saved."""
        D, d = d_in, d_out
        dev = dM.device
        scratch = _scratch(dev, "attn_small", _lib.load().sgf_attn_h_small_workspace_bytes(D, d))
        Dm = torch.empty((D, D), dtype=_F32, device=dev)
        ds = torch.empty(D, dtype=_F32, device=dev)
        gw = torch.empty((3 if want_v else 2, d, D), dtype=_F32, device=dev)
        gb = torch.empty((3 if want_v else 2, d), dtype=_F32, device=dev)
        gwv, gbv = (gw[2], gb[2]) if want_v else (None, None)
        _launch(dev, "sgf_attn_h_small_bwd", dM, dM.stride(0), dw, dm, dbeta, float(n_total), D, d, saved, saved.numel(), Dm, D,
                ds, gw[0], gb[0], gw[1], gb[1], gwv, gbv, D, *scratch)
        return Dm, ds, gw[0], gb[0], gw[1], gb[1], gwv, gbv

    # ---- T3 ----  q, k: [n, H*d] views (ld = stride(0)); v: [n, Hv*d]
    @staticmethod
    def attn_fwd_reduce(q, k, v, heads: int, v_heads: int, d: int) -> torch.Tensor:
        n, dev = q.shape[0], q.device
        lib = _lib.load()
        stats = torch.empty(lib.sgf_attn_stats_len(heads, d), dtype=_F32, device=dev)
        _launch(dev, "sgf_attn_fwd_reduce", q, _ld(q), k, _ld(k), v, _ld(v), n, heads, v_heads, d, _code(q), stats,
                *_scratch(dev, "attn", lib.sgf_attn_workspace_bytes(n, heads, d)))
        return stats

    @staticmethod
    def attn_fwd_apply(q, v, stats, n_total: float, heads: int, v_heads: int, d: int):
        n, dev = q.shape[0], q.device
        out = torch.empty((n, d), dtype=q.dtype, device=dev)
        den = torch.empty((n, heads), dtype=_F32, device=dev)
        o_heads = torch.empty((n, heads * d), dtype=q.dtype, device=dev) if heads > 1 else None
        _launch(dev, "sgf_attn_fwd_apply", q, _ld(q), v, _ld(v), n, float(n_total), heads, v_heads, d, _code(q), stats, out,
                out.stride(0), den, o_heads)
        return out, den, o_heads

    @staticmethod
    def attn_bwd_reduce(q, g, o, den, heads: int, d: int, per_head: bool = False) -> torch.Tensor:
        """per_head: g is [n, H * d], the gradients of the per-head outputs (no 1/H), instead of the head mean's [n, d]"""
        n, dev = q.shape[0], q.device
        lib = _lib.load()
        bstats = torch.empty(lib.sgf_attn_bstats_len(heads, d), dtype=_F32, device=dev)
        _launch(dev, "sgf_attn_bwd_reduce_heads" if per_head else "sgf_attn_bwd_reduce", q, _ld(q), g, _ld(g), o, _ld(o), den, n,
                heads, d, _code(q), bstats, *_scratch(dev, "attn", lib.sgf_attn_workspace_bytes(n, heads, d)))
        return bstats

    @staticmethod
    def attn_bwd_apply(q, k, v, g, o, den, stats, bstats, n_total: float, heads: int, v_heads: int,
                       d: int, dq, dk, dv, per_head: bool = False):
        """Writes dq, dk, dv (views with row stride = stride(0)) in place."""
        n, dev = q.shape[0], q.device
        _launch(dev, "sgf_attn_bwd_apply_heads" if per_head else "sgf_attn_bwd_apply", q, _ld(q), k, _ld(k), v, _ld(v), g, _ld(g),
                o, _ld(o), den, n, float(n_total), heads, v_heads, d, _code(q), stats, bstats, dq, _ld(dq), dk, _ld(dk), dv,
                _ld(dv))

    # ---- T3+T4 fused: attention from the un-projected input (H = 1) ----
    @staticmethod
    def attn_h_fwd(h, M, m, w, beta):
        n, d = h.shape
        dev = h.device
        out = torch.empty((n, d), dtype=h.dtype, device=dev)
        den = torch.empty((n, 1), dtype=_F32, device=dev)
        _launch(dev, "sgf_attn_h_fwd", h, _ld(h), n, d, _mm_code(h, "sgf_attn_h_supported", d), M, m, w, beta, out,
                out.stride(0), den)
        return out, den

    @staticmethod
    def attn_h_bwd_reduce(h, g, o, den):
        n, d = h.shape
        dev = h.device
        lib = _lib.load()
        hstats = torch.empty(lib.sgf_attn_h_bstats_len(d), dtype=_F32, device=dev)
        scratch = _scratch(dev, "attn", lib.sgf_attn_workspace_bytes(n, 1, d))
        _launch(dev, "sgf_attn_h_bwd_reduce", h, _ld(h), g, _ld(g), o, _ld(o), den, n, d,
                _mm_code(h, "sgf_attn_h_supported", d), hstats, *scratch)
        return hstats

    @staticmethod
    def attn_h_bwd_apply(h, g, o, den, M, w, D, ds):
        n, d = h.shape
        dev = h.device
        dh = torch.empty((n, d), dtype=h.dtype, device=dev)
        code = _mm_code(h, "sgf_attn_h_supported", d)
        nb = _lib.load().sgf_attn_h_bwd_apply_workspace_bytes(n, d, code)
        _launch(dev, "sgf_attn_h_bwd_apply", h, _ld(h), g, _ld(g), o, _ld(o), den, n, d, code, M, w, D, ds, dh, dh.stride(0),
                *(_scratch(dev, "attn_h_part", nb) if nb else _NO_SCRATCH))
        return dh

    @staticmethod
    def attn_h_bwd_split_supported(h, g, o) -> bool:
        d = h.shape[1]
        return (h.dtype == _BF16 and bool(_lib.load().sgf_attn_h_bwd_split_supported(d, _code(h)))
                and all(t.stride(-1) == 1 and (t.stride(0) * 2) % 16 == 0 and t.data_ptr() % 16 == 0 for t in (h, g, o)))

    @staticmethod
    def attn_h_bwd_pre(g, o, den, M, w):
        """First apply pass of the backward (dnum M^T + dden w -> scratch) + the per-row scalars (1/den, dden)."""
        n, d = g.shape
        dev = g.device
        scratch = _scratch(dev, "attn_h_part", _lib.load().sgf_attn_h_bwd_apply_workspace_bytes(n, d, _code(g)))
        rowscal = torch.empty((n, 2), dtype=_F32, device=dev)
        _launch(dev, "sgf_attn_h_bwd_pre", g, _ld(g), o, _ld(o), den, n, d, _code(g), M, w, *scratch, rowscal)
        return rowscal

    @staticmethod
    def attn_h_bwd_reduce_scaled(h, g, rowscal):
        n, d = h.shape
        dev = h.device
        lib = _lib.load()
        hstats = torch.empty(lib.sgf_attn_h_bstats_len(d), dtype=_F32, device=dev)
        _launch(dev, "sgf_attn_h_bwd_reduce_scaled", h, _ld(h), g, _ld(g), rowscal, n, d, _code(h), hstats,
                *_scratch(dev, "attn", lib.sgf_attn_workspace_bytes(n, 1, d)))
        return hstats

    @staticmethod
    def attn_h_bwd_post(h, D, ds, addend=None):
        """dh = h D + ds + the scratch attn_h_bwd_pre left on this stream [+ addend, a second gradient of h]."""
        n, d = h.shape
        dev = h.device
        scratch = _scratch(dev, "attn_h_part", _lib.load().sgf_attn_h_bwd_apply_workspace_bytes(n, d, _code(h)))
        dh = torch.empty((n, d), dtype=h.dtype, device=dev)
        _launch(dev, "sgf_attn_h_bwd_post", h, _ld(h), n, d, _code(h), D, ds, *scratch, addend, _ld(addend), dh, dh.stride(0))
        return dh

    # ---- T4: dW = a^T b, db = colsum(a) ----
    @staticmethod
    def gram(a, b, out=None, want_colsum=True):
        """out[m, k] (fp32, may be a column-sliced view) = a[n, m]^T b[n, k]; colsum(a) fp32 [m]."""
        n, m = a.shape
        k = b.shape[1]
        dev = a.device
        if out is None:
            out = torch.empty((m, k), dtype=_F32, device=dev)
        cs = torch.empty(m, dtype=_F32, device=dev) if want_colsum else None
        _launch(dev, "sgf_gram", a, _ld(a), m, b, _ld(b), k, n, _mm_code(a), out, out.stride(0), cs,
                *_scratch(dev, "attn", _lib.load().sgf_gram_workspace_bytes(n, m, k)))
        return out, cs

    @staticmethod
    def gram2(a, b1, b2, out1, out2, want_colsum=True):
        """out1 = a^T b1, out2 = a^T b2 (fp32, may be column-sliced views of one matrix) from one paired launch; colsum(a)."""
        n, m = a.shape
        k = b1.shape[1]
        dev = a.device
        cs = torch.empty(m, dtype=_F32, device=dev) if want_colsum else None
        _launch(dev, "sgf_gram2", a, _ld(a), m, b1, _ld(b1), b2, _ld(b2), k, n, _mm_code(a), out1, out1.stride(0), out2,
                out2.stride(0), cs, *_scratch(dev, "attn", _lib.load().sgf_gram_workspace_bytes(n, m, k)))
        return cs

    # ---- T5 ----
    @staticmethod
    def ln_fwd(x, res, a: float, b: float, gamma, beta, relu: bool, eps: float):
        n, d = x.shape
        dev = x.device
        y = torch.empty((n, d), dtype=x.dtype, device=dev)
        mean = torch.empty(n, dtype=_F32, device=dev) if gamma is not None else None
        rstd = torch.empty(n, dtype=_F32, device=dev) if gamma is not None else None
        _launch(dev, "sgf_ln_fwd", x, _ld(x), res, _ld(res), float(a), float(b), gamma, beta, int(relu), float(eps), n, d,
                _code(x), y, y.stride(0), mean, rstd)
        return y, mean, rstd

    @staticmethod
    def ln_bwd(gy, y, x, res, a: float, b: float, gamma, relu: bool, mean, rstd):
        """(dx, dres, dgamma, dbeta).  a == b (the large variant's (x + res) / 2): dx and dres are the same values —
        ONE tensor is written and returned for both."""
        n, d = x.shape
        dev = x.device
        dx = torch.empty_like(x)
        shared = res is not None and float(a) == float(b)
        dres = torch.empty_like(res) if (res is not None and not shared) else None
        dgamma = torch.empty(d, dtype=_F32, device=dev) if gamma is not None else None
        dbeta = torch.empty(d, dtype=_F32, device=dev) if gamma is not None else None
        _launch(dev, "sgf_ln_bwd", gy, _ld(gy), y, _ld(y), x, _ld(x), res, _ld(res), float(a), float(b), gamma, int(relu), mean,
                rstd, n, d, _code(x), dx, _ld(dx), dres, _ld(dres), dgamma, dbeta,
                *_scratch(dev, "ln", _lib.load().sgf_ln_bwd_workspace_bytes(n, d)))
        return dx, (dx if shared else dres), dgamma, dbeta

    # ---- T6 ----
    @staticmethod
    def colstats(x, shift) -> torch.Tensor:
        n, d = x.shape
        dev = x.device
        stats = torch.empty(2 * d, dtype=_F32, device=dev)
        _launch(dev, "sgf_colstats", x, _ld(x), shift, n, d, _code(x), stats,
                *_scratch(dev, "col", _lib.load().sgf_colstats_workspace_bytes(n, d)))
        return stats

    @staticmethod
    def bn_finalize(sums, shift, n_total: float, eps: float, momentum: float, running_mean, running_var):
        """(mean, rstd) fp32 [d] from the shifted sums; running_mean / running_var (fp32, or None) updated in place."""
        d = sums.numel() // 2
        mean = torch.empty(d, dtype=_F32, device=sums.device)
        rstd = torch.empty(d, dtype=_F32, device=sums.device)
        _launch(sums.device, "sgf_bn_finalize", sums, shift, float(n_total), float(eps), float(momentum), running_mean,
                running_var, d, mean, rstd)
        return mean, rstd

    @staticmethod
    def bn_apply(x, mean, rstd, gamma, beta, res, relu: bool) -> torch.Tensor:
        n, d = x.shape
        dev = x.device
        y = torch.empty((n, d), dtype=x.dtype, device=dev)
        _launch(dev, "sgf_bn_apply", x, _ld(x), mean, rstd, gamma, beta, res, _ld(res), int(relu), n, d, _code(x), y, y.stride(0))
        return y

    @staticmethod
    def bn_apply_packed(x, mean, rstd, gamma, beta, res, relu: bool, slot_bytes: int):
        """(bn_apply's y, its rows in packed form for spmm_packed).  bf16 rows of 256 columns."""
        n, d = x.shape
        dev = x.device
        y = torch.empty((n, d), dtype=x.dtype, device=dev)
        nbytes = _lib.load().sgf_spmm_packed_bytes(n, int(slot_bytes))
        packed = PackedRows(torch.empty(nbytes, dtype=torch.uint8, device=dev), int(slot_bytes), n,
                            torch.empty(1, dtype=torch.int32, device=dev))
        _launch(dev, "sgf_bn_apply_packed", x, _ld(x), mean, rstd, gamma, beta, res, _ld(res), int(relu), n, d, _code(x), y,
                y.stride(0), packed.slots, packed.slot_bytes, packed.overflow)
        return y, packed

    @staticmethod
    def bn_bwd_stats(gy, x, mean, rstd, gamma, beta, relu: bool) -> torch.Tensor:
        n, d = x.shape
        dev = x.device
        stats = torch.empty(2 * d, dtype=_F32, device=dev)
        _launch(dev, "sgf_bn_bwd_stats", gy, _ld(gy), x, _ld(x), mean, rstd, gamma, beta, int(relu), n, d, _code(x), stats,
                *_scratch(dev, "col", _lib.load().sgf_colstats_workspace_bytes(n, d)))
        return stats

    @staticmethod
    def bn_bwd_stats2(gy, gy2, x, mean, rstd, gamma, beta, relu: bool) -> torch.Tensor:
        """bn_bwd_stats of the gradient gy + gy2 (two consumers of the BatchNorm's output; gy2 may be None)."""
        n, d = x.shape
        dev = x.device
        stats = torch.empty(2 * d, dtype=_F32, device=dev)
        _launch(dev, "sgf_bn_bwd_stats2", gy, _ld(gy), gy2, _ld(gy2), x, _ld(x), mean, rstd, gamma, beta, int(relu), n, d,
                _code(x), stats, *_scratch(dev, "col", _lib.load().sgf_colstats_workspace_bytes(n, d)))
        return stats

    @staticmethod
    def gram_ln_bwd_supported(m: int, k: int, dtype) -> bool:
        return dtype == _BF16 and bool(_lib.load().sgf_gram_ln_bwd_supported(int(m), int(k), _dtype_code(dtype)))

    @staticmethod
    def gram_ln_bwd(g, xin, mean, rstd, gamma, beta, relu: bool, b):
        """(dl^T b [m, k], sum dl [m], dgamma [m], dbeta [m]) with dl = the LayerNorm's input gradient, never written."""
        n, m = xin.shape
        k = b.shape[1]
        dev = xin.device
        out = torch.empty((m, k), dtype=_F32, device=dev)
        cs = torch.empty(m, dtype=_F32, device=dev)
        dg = torch.empty(m, dtype=_F32, device=dev)
        db = torch.empty(m, dtype=_F32, device=dev)
        _launch(dev, "sgf_gram_ln_bwd", g, _ld(g), xin, _ld(xin), mean, rstd, gamma, beta, int(relu), m, b, _ld(b), k, n,
                _code(xin), out, out.stride(0), cs, dg, db, *_scratch(dev, "attn", _lib.load().sgf_gram_workspace_bytes(n, m, k)))
        return out, cs, dg, db

    @staticmethod
    def gram_bn_bwd_supported(m: int, k: int, dtype) -> bool:
        return dtype == _BF16 and bool(_lib.load().sgf_gram_bn_bwd_supported(int(m), int(k), _dtype_code(dtype)))

    @staticmethod
    def gram_bn_bwd(gy, gy2, z, mean, rstd, gamma, beta, relu: bool, stats, inv_n: float, training: bool, b):
        """(dz^T b [m, k] fp32, colsum(dz) [m]) with dz = bn_bwd_apply(gy + gy2, z, ...) never written (sgf_gram_bn_bwd)."""
        n, m = z.shape
        k = b.shape[1]
        dev = z.device
        out = torch.empty((m, k), dtype=_F32, device=dev)
        cs = torch.empty(m, dtype=_F32, device=dev)
        _launch(dev, "sgf_gram_bn_bwd", gy, _ld(gy), gy2, _ld(gy2), z, _ld(z), mean, rstd, gamma, beta, int(relu), stats,
                float(inv_n), int(training), m, b, _ld(b), k, n, _code(z), out, out.stride(0), cs,
                *_scratch(dev, "attn", _lib.load().sgf_gram_workspace_bytes(n, m, k)))
        return out, cs

    @staticmethod
    def gram2_bn_bwd_supported(g, z, b1, b2) -> bool:
        """sgf_gram2_bn_bwd serves these operands (bf16, sizes, 16-byte aligned rows)?"""
        n, m = z.shape
        ok = all(t.dtype == _BF16 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0
                 for t in (g, z, b1, b2))
        return (ok and b1.shape == b2.shape and g.shape == z.shape
                and bool(_lib.load().sgf_gram2_bn_bwd_supported(int(m), int(b1.shape[1]), int(n), _code(z))))

    @staticmethod
    def gram2_bn_bwd(g, z, mean, rstd, gamma, beta, relu: bool, stats, inv_n: float, training: bool, b1, b2, out1, out2):
        """(dz, colsum(dz)); out1 = dz^T b1, out2 = dz^T b2 (fp32, may be column slices of one matrix): the BatchNorm backward
        and both weight-gradient blocks of a GraphConv layer from one pass over (g, z) (sgf_gram2_bn_bwd)."""
        n, m = z.shape
        k = b1.shape[1]
        dev = z.device
        dz = torch.empty((n, m), dtype=z.dtype, device=dev)
        cs = torch.empty(m, dtype=_F32, device=dev)
        _launch(dev, "sgf_gram2_bn_bwd", g, _ld(g), z, _ld(z), mean, rstd, gamma, beta, int(relu), stats, float(inv_n),
                int(training), m, b1, _ld(b1), b2, _ld(b2), k, n, _code(z), dz, dz.stride(0), out1, out1.stride(0), out2,
                out2.stride(0), cs, *_scratch(dev, "attn", _lib.load().sgf_gram_workspace_bytes(n, m, k)))
        return dz, cs

    @staticmethod
    def bn_bwd_apply(gy, x, mean, rstd, gamma, beta, relu: bool, stats, inv_n: float,
                     training: bool) -> torch.Tensor:
        n, d = x.shape
        dev = x.device
        dx = torch.empty_like(x)
        _launch(dev, "sgf_bn_bwd_apply", gy, _ld(gy), x, _ld(x), mean, rstd, gamma, beta, int(relu), stats, float(inv_n),
                int(training), n, d, _code(x), dx, _ld(dx))
        return dx

    @staticmethod
    def colsum(x) -> torch.Tensor:
        n, d = x.shape
        dev = x.device
        out = torch.empty(d, dtype=_F32, device=dev)
        _launch(dev, "sgf_colsum", x, _ld(x), n, d, _code(x), out,
                *_scratch(dev, "colsum", _lib.load().sgf_colsum_workspace_bytes(n, d)))
        return out

    # ---- dropout (+ residual), mask recomputed from the seed ----
    @staticmethod
    def dropout(x, res, p: float, seed: int) -> torch.Tensor:
        n, d = x.shape
        y = torch.empty((n, d), dtype=x.dtype, device=x.device)
        _launch(x.device, "sgf_dropout", x, _ld(x), res, _ld(res), float(p), int(seed), n, d, _code(x), y, y.stride(0))
        return y

    @staticmethod
    def dropout_dev(x, res, p: float, seeds: torch.Tensor, slot: int) -> torch.Tensor:
        """K.dropout with the seed read from seeds[slot] (contiguous int64 on x's device) when the kernel runs."""
        if not (seeds.dtype == torch.int64 and seeds.dim() == 1 and seeds.is_contiguous() and seeds.device == x.device):
            raise ValueError("dropout_dev: seeds must be a contiguous 1-D int64 tensor on x's device")
        if not 0 <= int(slot) < seeds.numel():
            raise IndexError(f"dropout_dev: slot {slot} outside a bank of {seeds.numel()}")
        n, d = x.shape
        y = torch.empty((n, d), dtype=x.dtype, device=x.device)
        _launch(x.device, "sgf_dropout_dev", x, _ld(x), res, _ld(res), float(p), seeds.data_ptr() + 8 * int(slot), n, d,
                _code(x), y, y.stride(0))
        return y

    # ---- N4: log_softmax + NLL on the training rows ----
    @staticmethod
    def nll_fwd(logits, labels, idx) -> torch.Tensor:
        n, c = logits.shape
        dev = logits.device
        out = torch.empty(1, dtype=_F32, device=dev)
        _launch(dev, "sgf_nll_fwd", logits, logits.stride(0), n, c, _code(logits), labels, idx, idx.numel(), out,
                *_scratch(dev, "nll", _lib.load().sgf_nll_workspace_bytes(idx.numel())))
        return out

    @staticmethod
    def nll_bwd(logits, labels, idx, gout, inv_denom: float) -> torch.Tensor:
        n, c = logits.shape
        dev = logits.device
        d = torch.empty((n, c), dtype=logits.dtype, device=dev)
        _launch(dev, "sgf_nll_bwd", logits, logits.stride(0), n, c, _code(logits), labels, idx, idx.numel(), gout,
                float(inv_denom), d, d.stride(0))
        return d

    # ---- N4b: BCEWithLogitsLoss on the training rows (idx None: the dense form, every row) ----
    # These two sit on a path whose GPU work is a few microseconds at mini-batch sizes: one pass over the arguments and one
    # allocation each on top of what _launch does.
    @staticmethod
    def _bce_args(logits, target, idx):
        """(n, c, m, target, kind, ldt) after the checks both entries share: logits [n, c] fp32 / bf16 with unit inner stride
        and rows that do not overlap; target fp32 or int64 [n, c] (contiguous rows) or int64 [n] class indices; idx int64
        [m] contiguous or None."""
        if logits.dim() != 2 or logits.stride(1) != 1 or (logits.stride(0) < logits.shape[1] and logits.shape[0] > 1):
            raise ValueError(f"bce: logits must be [n, c] with unit inner stride and a row stride >= c, got shape "
                             f"{tuple(logits.shape)} strides {logits.stride()}")
        n, c = logits.shape
        tdt = target.dtype
        if target.device != logits.device or (idx is not None and idx.device != logits.device):
            raise ValueError("bce: logits, target and idx must be on the same device")
        if target.dim() == 2 and target.shape == logits.shape and (tdt == _F32 or tdt == torch.int64):
            if target.stride(1) != 1 or (target.stride(0) < c and n > 1):
                raise ValueError(f"bce: target rows must be contiguous, got strides {target.stride()}")
            kind = _lib.SGF_BCE_TARGET_F32 if tdt == _F32 else _lib.SGF_BCE_TARGET_I64
            ldt = max(target.stride(0), c)
        elif target.dim() == 1 and target.shape[0] == n and tdt == torch.int64:
            kind, ldt = _lib.SGF_BCE_TARGET_CLASS, 0
            target = target.contiguous()
        else:
            raise ValueError(f"bce: target must be float32 / int64 {tuple(logits.shape)} or int64 class indices [{n}], got "
                             f"{tdt} {tuple(target.shape)}")
        if idx is None:
            m = n
        else:
            if idx.dim() != 1 or idx.dtype != torch.int64 or not idx.is_contiguous():
                raise ValueError(f"bce: idx must be a contiguous int64 vector, got {idx.dtype} {tuple(idx.shape)}")
            m = idx.numel()
            if m > n:
                raise ValueError(f"bce: idx holds {m} rows of a {n}-row matrix (rows must be distinct)")
        return n, c, m, target, kind, ldt

    @staticmethod
    def bce_fwd(logits, target, idx, inv_denom: float = 1.0) -> torch.Tensor:
        """inv_denom * sum of the element losses over the rows idx, as a 0-dim fp32 tensor."""
        n, c, m, target, kind, ldt = HipKernels._bce_args(logits, target, idx)
        dev = logits.device
        code = _code(logits)
        out = torch.empty((), dtype=_F32, device=dev)
        _launch(dev, "sgf_bce_fwd", logits, max(logits.stride(0), c), n, c, code, target, ldt, kind, idx, m, float(inv_denom),
                out, *_scratch(dev, "bce", _const_bytes("sgf_bce_workspace_bytes", m, c)))
        return out

    @staticmethod
    def bce_bwd(logits, target, idx, gout, inv_denom: float) -> torch.Tensor:
        n, c, m, target, kind, ldt = HipKernels._bce_args(logits, target, idx)
        dev = logits.device
        if gout.dtype != _F32 or gout.numel() != 1 or gout.device != dev:
            raise ValueError("bce: gout must be one float32 on the logits' device")
        d = torch.empty((n, c), dtype=logits.dtype, device=dev)
        _launch(dev, "sgf_bce_bwd", logits, max(logits.stride(0), c), n, c, _code(logits), target, ldt, kind, idx, m, gout,
                float(inv_denom), d, c)
        return d

    # ---- N5: the evaluation metrics as integer counts (idx None: every row) ----
    @staticmethod
    def _metric_args(what, logits, labels, idx, per_column: bool):
        """(n, c, m, labels, kind, label stride) after the checks both entries share: logits [n, c] fp32 / bf16 with unit inner
        stride and rows that do not overlap; labels fp32 or int64, [n, c] with contiguous rows (per_column) or one per node
        as [n] / [n, 1] with any stride; idx int64 [m] contiguous or None."""
        if logits.dim() != 2 or logits.stride(1) != 1 or (logits.stride(0) < logits.shape[1] and logits.shape[0] > 1):
            raise ValueError(f"{what}: logits must be [n, c] with unit inner stride and a row stride >= c, got shape "
                             f"{tuple(logits.shape)} strides {logits.stride()}")
        n, c = logits.shape
        if c < 1:
            raise ValueError(f"{what}: logits need at least one column, got shape {tuple(logits.shape)}")
        if labels.device != logits.device or (idx is not None and idx.device != logits.device):
            raise ValueError(f"{what}: logits, labels and idx must be on the same device")
        if labels.dtype == _F32:
            kind = _lib.SGF_METRIC_TARGET_F32
        elif labels.dtype == torch.int64:
            kind = _lib.SGF_METRIC_TARGET_I64
        else:
            raise ValueError(f"{what}: labels must be float32 or int64, got {labels.dtype}")
        if per_column:
            if labels.dim() != 2 or labels.shape != logits.shape:
                raise ValueError(f"{what}: labels must be {tuple(logits.shape)}, got {tuple(labels.shape)}")
            if labels.stride(1) != 1 or (labels.stride(0) < c and n > 1):
                raise ValueError(f"{what}: label rows must be contiguous, got strides {labels.stride()}")
            stride = max(labels.stride(0), c)
        else:
            if labels.shape not in ((n,), (n, 1)):
                raise ValueError(f"{what}: labels must be [{n}] or [{n}, 1], got {tuple(labels.shape)}")
            stride = max(labels.stride(0), 1)
            if n > 1 and labels.stride(0) < 1:
                raise ValueError(f"{what}: labels must have a positive stride, got {labels.stride()}")
        if idx is None:
            m = n
        else:
            if idx.dim() != 1 or idx.dtype != torch.int64 or not idx.is_contiguous():
                raise ValueError(f"{what}: idx must be a contiguous int64 vector, got {idx.dtype} {tuple(idx.shape)}")
            m = idx.numel()
        if m >= 2 ** 31:
            raise ValueError(f"{what}: {m} rows, the limit is 2^31 - 1")
        return n, c, m, labels, kind, stride

    @staticmethod
    def rocauc_counts(logits, target, idx) -> torch.Tensor:
        """int64 [c, 6] on the device: per column P, Nn, U2, other, nan_scores, unlabelled (include/sgf.h block N5)."""
        n, c, m, target, kind, ldt = HipKernels._metric_args("rocauc_counts", logits, target, idx, True)
        dev = logits.device
        counts = torch.empty((c, 6), dtype=torch.int64, device=dev)
        nbytes = int(_lib.load().sgf_rocauc_workspace_bytes(m, c)) if m else 0
        if m and c >= 1 and nbytes == 0:
            _lib.check(_lib.SGF_E_HIP, "sgf_rocauc_workspace_bytes")
        # some 24 m c bytes (230 MB at the ogbn-proteins train split) for a call made once every eval_step epochs:
        # taken from the caching allocator and given back, not kept in the per-stream scratch cache
        _launch(dev, "sgf_rocauc_counts", logits, max(logits.stride(0), c), n, c, _code(logits), target, ldt, kind, idx, m,
                counts, *_scratch(dev, None, nbytes))
        return counts

    @staticmethod
    def argmax_count(logits, labels, idx) -> torch.Tensor:
        """int64 [2] on the device: { labelled rows, rows whose argmax equals the label } (include/sgf.h block N5)."""
        n, c, m, labels, kind, stride = HipKernels._metric_args("argmax_count", logits, labels, idx, False)
        dev = logits.device
        counts = torch.empty((2,), dtype=torch.int64, device=dev)
        _launch(dev, "sgf_argmax_count", logits, max(logits.stride(0), c), n, c, _code(logits), labels, stride, kind, idx, m,
                counts, *_scratch(dev, "argmax", _const_bytes("sgf_argmax_workspace_bytes", m, c)))
        return counts

    @staticmethod
    def sum_n(xs) -> torch.Tensor:
        """sum of up to 8 equally shaped [n, d] tensors in one pass."""
        xs = [_rows(x) for x in xs]
        n, d = xs[0].shape
        y = torch.empty((n, d), dtype=xs[0].dtype, device=xs[0].device)
        k = len(xs)
        ptrs = (ctypes.c_void_p * k)(*[x.data_ptr() for x in xs])
        lds = (ctypes.c_int64 * k)(*[x.stride(0) for x in xs])
        _launch(y.device, "sgf_sum_n", ptrs, lds, k, n, d, _code(y), y, y.stride(0))
        return y

    # ---- T7 fused: logits = (a x1 + b x2) W^T + bias ----
    @staticmethod
    def combine_fc_supported(d: int, classes: int, dtype) -> bool:
        """bf16: d % 32 == 0, d <= 256, classes <= 64 (csrc/head.hip); fp32: d % 4 == 0, d <= 256 and the class count
        PADDED to a multiple of 4 (ops.combine_fc pads W / bias with zero rows) up to 256 (csrc/linear_f32.hip)."""
        if dtype not in (_F32, _BF16):
            return False
        # bf16 with more than 64 classes: the same exact-fp32 kernel with bf16 rows on the wire (C = 172: papers100M)
        if dtype == _F32 or classes > 64:
            classes = (classes + 3) // 4 * 4
        return bool(_lib.load().sgf_combine_fc_supported(d, classes, _dtype_code(dtype)))

    @staticmethod
    def combine_fc_mapped_supported(d: int, classes: int, dtype) -> bool:
        """the row-mapped forms (sgf_combine_fc_*_mapped): the bf16 kernels of csrc/head.hip only"""
        return dtype == _BF16 and classes <= 64 and bool(_lib.load().sgf_combine_fc_supported(d, classes, _dtype_code(dtype)))

    @staticmethod
    def combine_fc_fwd(x1, a: float, x2, b: float, w, bias, row_map=None) -> torch.Tensor:
        """row_map (int32 permutation): row j of the product is stored as row row_map[j]"""
        n, d = x1.shape
        c = w.shape[0]
        HipKernels._check_row_map(row_map, n, x1.device)
        logits = torch.empty((n, c), dtype=_F32, device=x1.device)
        if row_map is None:
            _launch(x1.device, "sgf_combine_fc_fwd", x1, _ld(x1), float(a), x2, _ld(x2), float(b), w, bias, n, d, c,
                    _mm_code(x1, "sgf_combine_fc_supported", d, c), logits, logits.stride(0))
        else:
            _launch(x1.device, "sgf_combine_fc_fwd_mapped", x1, _ld(x1), float(a), x2, _ld(x2), float(b), w, bias, n, d, c,
                    _code(x1), logits, logits.stride(0), row_map)
        return logits

    @staticmethod
    def combine_fc_bwd(g, w, a: float, b: float, dtype, row_map=None):
        """row_map: row j of dx1 / dx2 comes from row row_map[j] of g"""
        n, c = g.shape
        d = w.shape[1]
        HipKernels._check_row_map(row_map, n, g.device)
        dx1 = torch.empty((n, d), dtype=dtype, device=g.device)
        dx2 = torch.empty((n, d), dtype=dtype, device=g.device)
        if row_map is None:
            _launch(g.device, "sgf_combine_fc_bwd", g, g.stride(0), w, n, d, c, float(a), float(b),
                    _mm_code(dx1, "sgf_combine_fc_supported", d, c), dx1, dx1.stride(0), dx2, dx2.stride(0))
        else:
            _launch(g.device, "sgf_combine_fc_bwd_mapped", g, g.stride(0), w, n, d, c, float(a), float(b), _lib.SGF_BF16, dx1,
                    dx1.stride(0), dx2, dx2.stride(0), row_map)
        return dx1, dx2

    @staticmethod
    def combine_fc_bwd_g(g, w, a: float, b: float, row_map=None):
        """(dx1, dx2, gp): combine_fc_bwd for bf16 storage and at most 64 classes that also returns gp = the logits' gradient
        in bf16, [n, 16 ceil(c / 16)], zero-padded, in the module's row order (sgf_combine_fc_bwd_g)."""
        n, c = g.shape
        d = w.shape[1]
        HipKernels._check_row_map(row_map, n, g.device)
        dx1 = torch.empty((n, d), dtype=_BF16, device=g.device)
        dx2 = torch.empty((n, d), dtype=_BF16, device=g.device)
        gp = torch.empty((n, (c + 15) // 16 * 16), dtype=_BF16, device=g.device)
        _launch(g.device, "sgf_combine_fc_bwd_g", g, g.stride(0), w, n, d, c, float(a), float(b), _code(dx1), dx1, dx1.stride(0),
                dx2, dx2.stride(0), row_map, gp, gp.stride(0))
        return dx1, dx2, gp

    @staticmethod
    def _check_row_map(row_map, n: int, device):
        """The *_mapped kernels read `const int32_t*`: anything else would scatter rows out of bounds."""
        if row_map is not None and not (row_map.dtype == torch.int32 and row_map.is_contiguous() and row_map.numel() == n
                                        and row_map.device == device):
            raise RuntimeError(f"combine_fc: row_map must be a contiguous int32 permutation of {n} rows on {device}, got "
                               f"{row_map.dtype} x {tuple(row_map.shape)} on {row_map.device}")

    # ---- T6 / K8: Linear (+ BatchNorm statistics) as one streaming pass ----
    @staticmethod
    def gcn_epilogue_supported(d_in: int, d_out: int, dtype) -> bool:
        """bf16 storage: square layers of 64 / 128 / 256 (csrc/rowgemm.hip); fp32 storage: any widths % 4 == 0 up to
        256 (csrc/linear_f32.hip, exact-fp32 matrix cores)."""
        return dtype in (_BF16, _F32) and bool(_lib.load().sgf_gcn_epilogue_supported(d_in, d_out, _dtype_code(dtype)))

    @staticmethod
    def gcn_epilogue_stats(a, w, bias, shift=None, want_stats=False):
        """y = a w^T + bias; with want_stats also [sum(y - shift) | sum((y - shift)^2)] per column of the
        rounded y.  w in a's dtype [d_out, d_in], bias / shift fp32."""
        n, d_in = a.shape
        d_out = w.shape[0]
        dev = a.device
        y = torch.empty((n, d_out), dtype=a.dtype, device=dev)
        stats = torch.empty(2 * d_out, dtype=_F32, device=dev) if want_stats else None
        scratch = _stats_scratch(dev, n, d_out, want_stats)
        _launch(dev, "sgf_gcn_epilogue_stats", a, _ld(a), w, w.stride(0), bias, n, d_in, d_out,
                _mm_code(a, "sgf_gcn_epilogue_supported", d_in, d_out), y, _ld(y), shift, stats, *scratch)
        return y, stats

    @staticmethod
    def gcn_epilogue_cat(a1, a2, w, bias, shift=None, want_stats=False):
        """y = [a1 | a2] w^T + bias (w [d, 2 d]).  bf16, square blocks: ONE pass over a1 and a2 (sgf_gcn_epilogue_cat: W
        resident in LDS for d <= 128, a paired launch for d = 256; SGF_GCN_CAT=0 keeps the two-pass form).  Otherwise two
        streaming passes: a1's product stays in the matrix cores' accumulator layout (an opaque scratch buffer) and is
        added in a2's pass."""
        n, d1 = a1.shape
        d2, d = a2.shape[1], w.shape[0]
        dev = a1.device
        lib = _lib.load()
        one_pass = (a1.dtype == _BF16 and d1 == d2 == d and _one_pass_cat() and lib.sgf_gcn_epilogue_cat_supported(d, _code(a1))
                    and w.stride(1) == 1 and w.shape[1] == 2 * d)
        part = None if one_pass else _scratch(dev, "gcn_part", lib.sgf_gcn_epilogue_dtype_partial_bytes(n, d, _code(a1)))
        y = torch.empty((n, d), dtype=a1.dtype, device=dev)
        stats = torch.empty(2 * d, dtype=_F32, device=dev) if want_stats else None
        scratch = _stats_scratch(dev, n, d, want_stats)
        if one_pass:
            _launch(dev, "sgf_gcn_epilogue_cat", a1, _ld(a1), a2, _ld(a2), w, w.stride(0), bias, n, d, _code(a1), y, _ld(y),
                    shift, stats, *scratch)
            return y, stats
        _launch(dev, "sgf_gcn_epilogue_partial", a1, _ld(a1), w[:, :d1], w.stride(0), bias, n, d1, d,
                _mm_code(a1, "sgf_gcn_epilogue_supported", d1, d), *part)
        _launch(dev, "sgf_gcn_epilogue_stats_add", a2, _ld(a2), w[:, d1:], w.stride(0), *part, n, d2, d,
                _mm_code(a2, "sgf_gcn_epilogue_supported", d2, d), y, _ld(y), shift, stats, *scratch)
        return y, stats

    @staticmethod
    def stem_pair_supported(d_in: int, d_out: int, dtype) -> bool:
        return dtype == _BF16 and bool(_lib.load().sgf_stem_pair_supported(d_in, d_out, _dtype_code(dtype)))

    @staticmethod
    def stem_pair(x, w0, b0, w1, b1, shift0=None, want_stats0=False):
        """y0 = x w0^T + b0 (+ its BatchNorm column sums), y1 = x w1^T + b1 from one read of x (w1 None: y1 None)."""
        n, d_in = x.shape
        d_out = w0.shape[0]
        dev = x.device
        y0 = torch.empty((n, d_out), dtype=x.dtype, device=dev)
        y1 = torch.empty((n, d_out), dtype=x.dtype, device=dev) if w1 is not None else None
        stats = torch.empty(2 * d_out, dtype=_F32, device=dev) if want_stats0 else None
        _launch(dev, "sgf_stem_pair", x, _ld(x), n, d_in, w0, w0.stride(0), b0, w1, _ld(w1), b1, d_out, _code(x), y0, _ld(y0), y1,
                _ld(y1), shift0, stats, *_stats_scratch(dev, n, d_out, want_stats0))
        return y0, y1, stats

    @staticmethod
    def gcn_epilogue_dx(dy, w):
        """dx = dy w  (w [d_out, d_in] in dy's dtype; may be a column slice of a wider matrix)."""
        n, d_out = dy.shape
        d_in = w.shape[1]
        dx = torch.empty((n, d_in), dtype=dy.dtype, device=dy.device)
        _launch(dy.device, "sgf_gcn_epilogue_dx", dy, _ld(dy), w, w.stride(0), n, d_in, d_out,
                _mm_code(dy, "sgf_gcn_epilogue_supported", d_out, d_in), dx, _ld(dx))
        return dx

    @staticmethod
    def gcn_epilogue_dx2_acc_supported(d: int, dtype) -> bool:
        return dtype == _BF16 and bool(_lib.load().sgf_gcn_epilogue_dx2_acc_supported(int(d), _dtype_code(dtype)))

    @staticmethod
    def gcn_epilogue_dx2_acc(dz, w, gadd, acc_in):
        """(dz W[:, :d], dz W[:, d:] + gadd + acc_in): both input gradients of the two-operand Linear, the second one added to
        the running gradient of x0 (sgf_gcn_epilogue_dx2_acc); gadd / acc_in may be None."""
        n, d = dz.shape
        dy = torch.empty_like(dz)
        acc = torch.empty_like(dz)
        _launch(dz.device, "sgf_gcn_epilogue_dx2_acc", dz, _ld(dz), w, _ld(w), n, d, _code(dz), dy, _ld(dy), gadd, _ld(gadd),
                acc_in, _ld(acc_in), acc, _ld(acc))
        return dy, acc

    @staticmethod
    def gcn_bn_bwd_dx_supported(d: int, dtype) -> bool:
        return dtype == _BF16 and bool(_lib.load().sgf_gcn_bn_bwd_dx_supported(int(d), _dtype_code(dtype)))

    @staticmethod
    def gcn_bn_bwd_dx(gy, z, mean, rstd, gamma, beta, relu: bool, stats, inv_n: float, training: bool, w, acc_in,
                      last: bool, add_gy: bool):
        """(dz, dy, acc): BatchNorm backward + both input gradients of W [Ax | x0] in one launch (sgf_gcn_bn_bwd_dx).
        `acc_in`: the running gradient of x0 from the layers processed so far (opaque uint8 tensor) or None; `acc`: the
        new running sum (opaque) or, with last=True, the total as a row-major [n, d] tensor."""
        n, d = z.shape
        dev = z.device
        dz = torch.empty((n, d), dtype=z.dtype, device=dev)
        dy = torch.empty((n, d), dtype=z.dtype, device=dev)
        nbytes = _lib.load().sgf_gcn_epilogue_partial_bytes(n, d)
        acc_out = None if last else torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        dx0 = torch.empty((n, d), dtype=z.dtype, device=dev) if last else None
        _launch(dev, "sgf_gcn_bn_bwd_dx", gy, _ld(gy), z, _ld(z), mean, rstd, gamma, beta, int(relu), stats, float(inv_n),
                int(training), w, w.stride(0), n, d, _code(z), dz, _ld(dz), dy, _ld(dy), acc_in, acc_out, nbytes, dx0, _ld(dx0),
                int(add_gy), *_scratch(dev, "gcn_bwd_sync", _lib.load().sgf_gcn_bn_bwd_dx_workspace_bytes(n, d)))
        return dz, dy, (dx0 if last else acc_out)

    @staticmethod
    def gcn_epilogue_dx2(dy, w1, w2, pair: bool = True):
        """(dy w1, dy w2) for two [d, d] column blocks of one weight matrix, dy read from HBM once (paired launch)."""
        n, d = dy.shape
        dx1 = torch.empty((n, d), dtype=dy.dtype, device=dy.device)
        dx2 = torch.empty((n, d), dtype=dy.dtype, device=dy.device)
        assert w1.stride(0) == w2.stride(0)
        _launch(dy.device, "sgf_gcn_epilogue_dx2", dy, _ld(dy), w1, w2, w1.stride(0), n, d,
                _mm_code(dy, "sgf_gcn_epilogue_supported", d, d), dx1, _ld(dx1), dx2, _ld(dx2), int(pair))
        return dx1, dx2

    # ---- T7 ----
    @staticmethod
    def axpby(x1, a: float, x2, b: float) -> torch.Tensor:
        n, d = x1.shape
        y = torch.empty((n, d), dtype=x1.dtype, device=x1.device)
        _launch(x1.device, "sgf_axpby", x1, _ld(x1), float(a), x2, _ld(x2), float(b), n, d, _code(x1), y, y.stride(0))
        return y
