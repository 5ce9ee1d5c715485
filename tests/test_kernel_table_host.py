"""What every method of kernels.HipKernels (and the neighbour sampler's four call sites) hands libsgf, pinned without a GPU
and without libsgf.so: a recording stand-in built from _lib.SIGNATURES takes the library's place, small CPU tensors take
the device tensors' place, and the recorded calls are compared with tests/golden/kernel_table_calls.json.

A wrong pointer, leading dimension, length or workspace name in one of these marshalling sites is a memory fault on the
device, not a failed assertion; ctypes itself checks only arity and scalar-versus-pointer, and only when the call runs.

Every recorded argument is one of: an int, a float, None, ["in", i, byte offset] (a pointer into the i-th tensor argument of
the method, plan and PackedRows fields included, in argument order), ["ret", j, byte offset] (into the j-th returned tensor),
["ws", name, numel] (a tensor of kernels._workspaces), "host" (a ctypes array or byref), "stream", or ["tmp", k] (any other
non-null pointer: a one-off scratch buffer, a contiguous copy; k numbers the distinct addresses of one case in order of
appearance, so that two calls are seen to share a temporary).  Returned tensors are recorded as shape, dtype and strides.

`python tests/test_kernel_table_host.py --write` regenerates the golden file from the code as it stands.
"""
import ast
import contextlib
import ctypes
import inspect
import json
import os
import sys
from types import SimpleNamespace as NS

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_table_calls.json")
STREAM = 0x5717EA00            # what the stand-in for torch.cuda.current_stream() reports as its handle

# wrappers that cannot be driven on CPU tensors: {method: (reason, the GPU test that covers it)} -- at most 4
NOT_DRIVEN = {}


# ------------------------------------------------------------------------------------------------
# the stand-in library
# ------------------------------------------------------------------------------------------------
def _poke(ctype, index, values):
    """The stand-in writes `values` through the pointer argument `index` (host memory here): what the wrapper reads back
    between its first call and its second."""
    def write(args):
        arr = (ctype * len(values)).from_address(getattr(args[index], "value", args[index]))
        arr[:] = values
    return write


def _poke_byref(pairs):
    def write(args):
        for index, value in pairs:
            args[index]._obj.value = value
    return write


_WRITES = {
    "sgf_csr_transpose": _poke(ctypes.c_int32, 9, [1]),                          # the symmetry flag
    "sgf_subgraph_plan": _poke(ctypes.c_int64, 6, [5]),                          # k, the number of kept edges
    "sgf_subgraph_csr_plan": _poke(ctypes.c_int64, 8, [6, 0, 3]),                # entries, bad subset, longest row
    "sgf_graph_prologue_plan": _poke(ctypes.c_int64, 6, [7]),
    "sgf_spmm_plan": _poke(ctypes.c_int64, 13, [1, 3, 0, 0]),
    "sgf_spmm_tile_blocks": _poke_byref([(5, 2)]),                               # nb
    "sgf_spmm_tile_plan": _poke(ctypes.c_int64, 17, [0, 3, 0, 0, 4, 5, 0, 0]),    # .., sh_cols used, .., n_frag, n_rem, .., bad
    "sgf_spmm_tile_pack_layout": _poke(ctypes.c_int64, 6, [3]),                  # 16-byte units of the pool
    "sgf_neighbor_sample_batch_workspace_bytes": _poke_byref([(3, 16), (4, 32)]),    # node / edge capacity
    "sgf_neighbor_sample_batch": _poke(ctypes.c_int64, 14, [5, 6]),              # nodes, edges of the batch
    "sgf_neighbor_sample_hop": _poke(ctypes.c_int64, 16, [4, 3]),                # edges, new nodes of the hop
}
_FLOATS = (ctypes.c_float, ctypes.c_double)


def _result(name, restype):
    if name.endswith("_supported"):
        return 1
    if restype is ctypes.c_size_t:
        return 4096
    if name.endswith("_len") or restype is ctypes.c_int64:
        return 64
    return 0


def _tensors_of(v, depth=2):
    if isinstance(v, torch.Tensor):
        yield v
    elif depth and isinstance(v, (list, tuple)):
        for w in v:
            yield from _tensors_of(w, depth - 1)


class Recorder:
    """`calls`: (name, raw arguments) in call order; `keep`: every tensor a frame between the call and the test held when
    the call was made, kept alive until the arguments are normalised so that no later allocation can take its address."""

    def __init__(self):
        self.calls, self.keep, self.results = [], [], {}

    def library(self, signatures):
        lib = NS()
        for name, (restype, argtypes) in signatures.items():
            setattr(lib, name, self._entry(name, restype, argtypes))
        return lib

    def _entry(self, name, restype, argtypes):
        def entry(*args):
            assert len(args) == len(argtypes), f"{name}: {len(args)} arguments for {len(argtypes)} parameters"
            raw = []
            for i, (a, t) in enumerate(zip(args, argtypes)):
                try:
                    t.from_param(a)                      # what ctypes would accept for this parameter
                except (TypeError, ctypes.ArgumentError) as e:
                    raise AssertionError(f"{name}: argument {i} ({a!r}) is no {t.__name__}: {e}")
                raw.append(self._raw(name, i, a, t))
            frame = sys._getframe(1)
            while frame is not None and frame.f_code.co_filename != __file__:
                for v in frame.f_locals.values():
                    self.keep.extend(_tensors_of(v))
                frame = frame.f_back
            self.calls.append((name, raw))
            if name in _WRITES:
                _WRITES[name](args)
            return self.results.get(name, _result(name, restype))
        return entry

    @staticmethod
    def _raw(name, i, a, t):
        if t is ctypes.c_void_p:
            if a is None:
                return None
            if isinstance(a, ctypes.c_void_p):
                return ("ptr", a.value) if a.value else None
            if isinstance(a, int):
                return ("ptr", a) if a else None
            assert isinstance(a, ctypes.Array) or type(a).__name__ == "CArgObject", f"{name}: argument {i}: {a!r}"
            return "host"
        v = getattr(a, "value", a)
        return float(v) if t in _FLOATS else int(v)


def _span(t):
    s = t.untyped_storage()
    return s.data_ptr(), s.data_ptr() + s.nbytes()


def _normalise(raw, ins, rets, workspaces, others):
    if not isinstance(raw, tuple):
        return raw
    p = raw[1]
    if p == STREAM:
        return "stream"
    for key, ws in workspaces.items():
        if ws.data_ptr() == p:
            return ["ws", key[1], ws.numel()]
    for exact in (True, False):
        for tag, group in (("in", ins), ("ret", rets)):
            for i, t in enumerate(group):
                if t.numel() == 0:
                    continue
                lo, hi = _span(t)
                if (t.data_ptr() == p) if exact else (lo <= p < hi):
                    return [tag, i, p - t.data_ptr()]
    return ["tmp", others.setdefault(p, len(others))]


def _flatten(v, out):
    """The tensors of an argument list or a return value, in order: plan objects and PackedRows by their fields."""
    if isinstance(v, torch.Tensor):
        out.append(v)
    elif isinstance(v, (list, tuple)):
        for w in v:
            _flatten(w, out)
    elif isinstance(v, dict):
        for w in v.values():
            _flatten(w, out)
    elif isinstance(v, NS):
        _flatten(list(vars(v).values()), out)
    elif hasattr(type(v), "__slots__") and not isinstance(v, (torch.dtype, torch.device)):
        _flatten([getattr(v, s) for s in type(v).__slots__], out)
    return out


def _describe(v):
    if isinstance(v, torch.Tensor):
        return {"shape": list(v.shape), "dtype": str(v.dtype), "strides": list(v.stride())}
    if isinstance(v, (list, tuple)):
        return [_describe(w) for w in v]
    if v is None or isinstance(v, (bool, int, float)):
        return v
    if hasattr(type(v), "__slots__"):
        return {type(v).__name__: {s: _describe(getattr(v, s)) for s in type(v).__slots__}}
    raise AssertionError(f"a wrapper returned {type(v).__name__}")


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
def F(*shape):
    return torch.zeros(*shape, dtype=torch.float32)


def B(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16)


def L(*shape):
    return torch.zeros(*shape, dtype=torch.int64)


def I(*shape):    # noqa: E743
    return torch.zeros(*shape, dtype=torch.int32)


def U(*shape):
    return torch.zeros(*shape, dtype=torch.uint8)


def A(*args, **kwargs):
    return args, kwargs


CPU = torch.device("cpu")
CASES = []          # (id, method name or None, builder -> (args, kwargs[, callable, extra inputs]), options)


def case(method, label, build, **options):
    CASES.append((f"{method}[{label}]", method, build, options))


def _csr(n=4, nnz=7):
    return L(n + 1), I(nnz), F(nnz)


def _qkv(dtype=torch.bfloat16, n=6, heads=2, d=4):
    t = torch.zeros(n, 3 * heads * d, dtype=dtype)
    hd = heads * d
    return t[:, :hd], t[:, hd:2 * hd], t[:, 2 * hd:]


def _bn(d=8):
    return F(d), F(d), F(d), F(d)          # mean, rstd, gamma, beta


def _blocked_plan():
    return NS(ecode=I(7), eval=F(7), nlds=I(4), sh_ptr=I(3), sh_cols=I(8), rows_per_block=2, lds_rows=4)


def _tile_plan(segs):
    return NS(blk_row=I(3), nb=2, block_rows=4, sh_ptr=I(3), sh_cols=I(8), tile_ptr=L(3), grp=I(2, 2), pool=U(4144),
              rem_rowptr=L(9), rem_col=I(5), rem_val=F(5), long_segments=segs)


def _packed(n=6):
    from sgformer_amd.kernels import PackedRows
    return PackedRows(U(4096), 384, n, I(1))


HIGH = dict(precision="high")

# ---- graph structure ----
case("csr_build", "", lambda: A(L(2, 5), 4))
case("csr_transpose", "", lambda: A(L(2, 5), 4, I(4), L(5), I(5)))
case("subgraph", "eid", lambda: A(L(2, 5), 4, L(3), True, True))
case("subgraph", "no_eid", lambda: A(L(2, 5), 4, L(3), False, False))
case("subgraph_csr", "edges", lambda: A(L(5), I(7), 4, L(3), I(4), True))
case("subgraph_csr", "no_edges", lambda: A(L(5), I(7), 4, L(3), I(4), False))
case("sampled_csr_supported", "", lambda: A(5))
case("sampled_csr_build", "", lambda: A(I(8), I(8), L(8), 4, 8, 5))
case("sampled_csr_transpose", "", lambda: A(*_csr(), 4))
case("graph_prologue", "", lambda: A(L(2, 5), 4, True, True, False))
case("reorder", "", lambda: A(L(2, 5), 4, 2, 3))
# ---- SpMM ----
case("spmm", "plain_f32", lambda: A(*_csr(), F(6, 8), 4))
case("spmm", "plain_bf16_out_slice", lambda: A(*_csr(), B(6, 8), 4, out=B(4, 16)[:, 8:]))
case("spmm", "long_segments", lambda: A(*_csr(), B(6, 8), 4, long_segments=3))
case("spmm", "stream_hint", lambda: A(*_csr(), B(6, 8), 4, stream_hint=True))
case("spmm", "stream_hint_long", lambda: A(*_csr(), F(6, 8), 4, long_segments=2, stream_hint=True))
case("spmm", "rows_copy", lambda: A(*_csr(), F(6, 16)[:, ::2], 4))
case("spmm", "rows_view", lambda: A(*_csr(), F(6, 16)[:, 4:12], 4))
case("spmm", "no_rows", lambda: A(*_csr(), F(6, 8), 0))
case("spmm_packed_supported", "bf16", lambda: A((6, 256), torch.bfloat16, 384))
case("spmm_packed_supported", "f32", lambda: A((6, 256), torch.float32, 384))
case("spmm_packed", "plain", lambda: A(*_csr(), B(6, 8), _packed(), 4))
case("spmm_packed", "long_segments", lambda: A(*_csr(), B(6, 8), _packed(), 4, long_segments=2))
case("spmm_plan", "", lambda: A(*_csr(), 4, 2, 4, 1024))
case("spmm_blocked", "plain", lambda: A(L(5), _blocked_plan(), F(6, 8), 4))
case("spmm_blocked", "long_out", lambda: A(L(5), _blocked_plan(), B(6, 8), 4, out=B(4, 8), long_segments=2))
case("tile_supported", "bf16", lambda: A(64, torch.bfloat16))
case("tile_supported", "f32", lambda: A(64, torch.float32))
case("tile_supported", "f16", lambda: A(64, torch.float16))
case("tile_blocks", "communities", lambda: A(I(8), 8, 4, CPU))
case("tile_blocks", "none", lambda: A(None, 8, 4, CPU))
case("tile_plan", "", lambda: A(*_csr(8, 10), 8, I(3), 4, 2, 1024))
case("tile_pack", "", lambda: A(I(3), L(3), I(2048), 4))
case("spmm_tile", "plain", lambda: A(_tile_plan(0), B(8, 16), 8))
case("spmm_tile", "long_out", lambda: A(_tile_plan(2), B(8, 16), 8, out=B(8, 16)))
case("spmm_tile", "rows16_copy", lambda: A(_tile_plan(0), B(8, 20)[:, :16], 8))
case("lds_rows_max", "bf16", lambda: A(torch.bfloat16))
case("lds_rows_max", "f32", lambda: A(torch.float32))
case("lds_rows_max", "f16", lambda: A(torch.float16))
# ---- rows in, rows out ----
case("gather_rows", "i64", lambda: A(F(6, 8), L(3)))
case("gather_rows", "i32_cast", lambda: A(F(6, 8), I(3), out_dtype=torch.bfloat16))
case("gather_rows", "copy", lambda: A(F(6, 16)[:, ::2], L(3)))
case("pad_rows", "no_idx", lambda: A(F(6, 6), None, 8))
case("pad_rows", "idx_cast", lambda: A(F(6, 6), L(3), 8, out_dtype=torch.bfloat16))
case("pad_rows", "idx_i32", lambda: A(B(6, 6), I(3), 8))
case("gemm", "plain", lambda: A(F(6, 8), F(8, 5)))
case("gemm", "transposed_bias", lambda: A(B(6, 8), B(5, 8).t(), bias=F(5), out_dtype=torch.float32))
case("gemm", "addend", lambda: A(F(6, 8), F(8, 5), alpha=0.5, beta=0.25, addend=F(6, 10)[:, :5]))
case("gemm", "addend_copy", lambda: A(F(6, 8), F(8, 5), beta=1.0, addend=F(6, 10)[:, ::2]))
case("gemm", "alpha_dev_out", lambda: A(F(6, 8), B(8, 5), alpha_dev=F(1), out=F(6, 16)[:, :5]))
# ---- attention ----
case("attn_h_small_fwd", "v", lambda: A(F(8, 8), F(8), 6.0, 12.0, F(4, 8), F(4), F(4, 8), F(4), F(4, 8), F(4)))
case("attn_h_small_fwd", "no_v", lambda: A(F(8, 8), F(8), 6.0, 12.0, F(4, 8), F(4), F(4, 8), F(4), None, None))
case("attn_h_small_fwd", "bf16_weights", lambda: A(B(8, 8), B(8), 6.0, 12.0, B(4, 8), F(4), B(4, 8), F(4), None, None))
case("attn_h_small_bwd", "v", lambda: A(F(8, 4), F(8), F(4), F(1), 12.0, U(4096), 8, 4))
case("attn_h_small_bwd", "no_v", lambda: A(F(8, 4), F(8), F(4), F(1), 12.0, U(4096), 8, 4, want_v=False))
case("attn_fwd_reduce", "bf16", lambda: A(*_qkv(), 2, 2, 4))
case("attn_fwd_reduce", "f32_one_v_head", lambda: A(F(6, 8), F(6, 8), F(6, 4), 2, 1, 4))
case("attn_fwd_apply", "heads2", lambda: A(_qkv()[0], _qkv()[2], F(64), 6.0, 2, 2, 4))
case("attn_fwd_apply", "heads1", lambda: A(F(6, 4), F(6, 4), F(64), 6.0, 1, 1, 4))
case("attn_bwd_reduce", "mean", lambda: A(_qkv()[0], B(6, 4), B(6, 8), F(6, 2), 2, 4))
case("attn_bwd_reduce", "per_head", lambda: A(_qkv()[0], B(6, 8), B(6, 8), F(6, 2), 2, 4, per_head=True))
case("attn_bwd_apply", "mean", lambda: A(*_qkv(), B(6, 4), B(6, 8), F(6, 2), F(64), F(64), 6.0, 2, 2, 4, *_qkv()))
case("attn_bwd_apply", "per_head",
     lambda: A(*_qkv(), B(6, 8), B(6, 8), F(6, 2), F(64), F(64), 6.0, 2, 2, 4, *_qkv(), per_head=True))
case("attn_h_fwd", "bf16", lambda: A(B(6, 8), F(8, 8), F(8), F(8), F(1)))
case("attn_h_fwd", "f32", lambda: A(F(6, 8), F(8, 8), F(8), F(8), F(1)))
case("attn_h_fwd", "f32_high", lambda: A(F(6, 8), F(8, 8), F(8), F(8), F(1)), **HIGH)
case("attn_h_fwd", "f32_high_unsupported", lambda: A(F(6, 8), F(8, 8), F(8), F(8), F(1)), **HIGH,
     results={"sgf_attn_h_supported": 0})
case("attn_h_bwd_reduce", "bf16", lambda: A(B(6, 16)[:, :8], B(6, 8), B(6, 8), F(6, 1)))
case("attn_h_bwd_reduce", "f32_high", lambda: A(F(6, 8), F(6, 8), F(6, 8), F(6, 1)), **HIGH)
case("attn_h_bwd_apply", "bf16", lambda: A(B(6, 8), B(6, 8), B(6, 8), F(6, 1), F(8, 8), F(8), F(8, 8), F(8)))
case("attn_h_bwd_apply", "f32_high", lambda: A(F(6, 8), F(6, 8), F(6, 8), F(6, 1), F(8, 8), F(8), F(8, 8), F(8)), **HIGH)
case("attn_h_bwd_apply", "no_scratch", lambda: A(B(6, 8), B(6, 8), B(6, 8), F(6, 1), F(8, 8), F(8), F(8, 8), F(8)),
     results={"sgf_attn_h_bwd_apply_workspace_bytes": 0})
case("attn_h_bwd_split_supported", "bf16", lambda: A(B(6, 8), B(6, 8), B(6, 8)))
case("attn_h_bwd_split_supported", "f32", lambda: A(F(6, 8), F(6, 8), F(6, 8)))
case("attn_h_bwd_pre", "", lambda: A(B(6, 8), B(6, 8), F(6, 1), F(8, 8), F(8)))
case("attn_h_bwd_reduce_scaled", "", lambda: A(B(6, 8), B(6, 8), F(6, 2)))
case("attn_h_bwd_post", "plain", lambda: A(B(6, 8), F(8, 8), F(8)))
case("attn_h_bwd_post", "addend", lambda: A(B(6, 8), F(8, 8), F(8), addend=B(6, 16)[:, 8:]))
# ---- weight gradients ----
case("gram", "bf16", lambda: A(B(6, 8), B(6, 4)))
case("gram", "out_slice_no_colsum", lambda: A(F(6, 8), F(6, 4), out=F(8, 12)[:, 4:8], want_colsum=False))
case("gram", "f32_high", lambda: A(F(6, 8), F(6, 4)), **HIGH)
case("gram2", "colsum", lambda: A(B(6, 8), B(6, 4), B(6, 4), F(8, 8)[:, :4], F(8, 8)[:, 4:]))
case("gram2", "no_colsum_f32_high", lambda: A(F(6, 8), F(6, 4), F(6, 4), F(8, 4), F(8, 4), want_colsum=False), **HIGH)
# ---- LayerNorm / BatchNorm ----
case("ln_fwd", "full", lambda: A(B(6, 8), B(6, 8), 0.5, 0.5, F(8), F(8), True, 1e-5))
case("ln_fwd", "no_res", lambda: A(F(6, 8), None, 1.0, 0.0, F(8), F(8), False, 1e-5))
case("ln_fwd", "no_affine", lambda: A(F(6, 8), F(6, 8), 0.75, 0.25, None, None, False, 1e-5))
case("ln_bwd", "a_eq_b", lambda: A(B(6, 8), B(6, 8), B(6, 8), B(6, 8), 0.5, 0.5, F(8), True, F(6), F(6)))
case("ln_bwd", "a_ne_b", lambda: A(F(6, 8), F(6, 8), F(6, 8), F(6, 8), 0.75, 0.25, F(8), False, F(6), F(6)))
case("ln_bwd", "no_res", lambda: A(F(6, 8), F(6, 8), F(6, 8), None, 1.0, 0.0, F(8), False, F(6), F(6)))
case("ln_bwd", "no_affine", lambda: A(F(6, 8), F(6, 8), F(6, 8), F(6, 8), 0.5, 0.5, None, False, None, None))
case("colstats", "shift", lambda: A(B(6, 8), F(8)))
case("colstats", "no_shift", lambda: A(F(6, 16)[:, :8], None))
case("bn_finalize", "running", lambda: A(F(16), F(8), 6.0, 1e-5, 0.1, F(8), F(8)))
case("bn_finalize", "none", lambda: A(F(16), None, 6.0, 1e-5, 0.1, None, None))
case("bn_apply", "full", lambda: A(B(6, 8), *_bn(), B(6, 8), True))
case("bn_apply", "none", lambda: A(F(6, 8), F(8), F(8), None, None, None, False))
case("bn_apply_packed", "full", lambda: A(B(6, 8), *_bn(), B(6, 8), True, 384))
case("bn_apply_packed", "none", lambda: A(B(6, 8), F(8), F(8), None, None, None, True, 384))
case("bn_bwd_stats", "full", lambda: A(B(6, 8), B(6, 8), *_bn(), True))
case("bn_bwd_stats", "none", lambda: A(F(6, 8), F(6, 8), F(8), F(8), None, None, False))
case("bn_bwd_stats2", "two", lambda: A(B(6, 8), B(6, 8), B(6, 8), *_bn(), True))
case("bn_bwd_stats2", "one", lambda: A(F(6, 8), None, F(6, 8), F(8), F(8), None, None, False))
case("gram_ln_bwd_supported", "bf16", lambda: A(8, 4, torch.bfloat16))
case("gram_ln_bwd_supported", "f32", lambda: A(8, 4, torch.float32))
case("gram_ln_bwd", "", lambda: A(B(6, 8), B(6, 8), F(6), F(6), F(8), F(8), True, B(6, 4)))
case("gram_bn_bwd_supported", "bf16", lambda: A(8, 4, torch.bfloat16))
case("gram_bn_bwd_supported", "f32", lambda: A(8, 4, torch.float32))
case("gram_bn_bwd", "two", lambda: A(B(6, 8), B(6, 8), B(6, 8), *_bn(), True, F(16), 0.125, True, B(6, 4)))
case("gram_bn_bwd", "one", lambda: A(B(6, 8), None, B(6, 8), *_bn(), False, F(16), 0.125, False, B(6, 4)))
case("gram2_bn_bwd_supported", "bf16", lambda: A(B(6, 8), B(6, 8), B(6, 8), B(6, 8)))
case("gram2_bn_bwd_supported", "f32", lambda: A(F(6, 8), F(6, 8), F(6, 8), F(6, 8)))
case("gram2_bn_bwd", "", lambda: A(B(6, 8), B(6, 8), *_bn(), True, F(16), 0.125, True, B(6, 8), B(6, 8),
                                   F(8, 16)[:, :8], F(8, 16)[:, 8:]))
case("bn_bwd_apply", "full", lambda: A(B(6, 8), B(6, 8), *_bn(), True, F(16), 0.125, True))
case("bn_bwd_apply", "none", lambda: A(F(6, 8), F(6, 8), F(8), F(8), None, None, False, F(16), 0.125, False))
case("colsum", "", lambda: A(B(6, 8)))
# ---- dropout, losses, metrics ----
case("dropout", "res", lambda: A(B(6, 8), B(6, 8), 0.5, 1234567))
case("dropout", "no_res", lambda: A(F(6, 8), None, 0.25, 7))
case("dropout_dev", "", lambda: A(B(6, 8), B(6, 8), 0.5, L(4), 2))
case("nll_fwd", "", lambda: A(F(6, 5), L(6), L(3)))
case("nll_bwd", "", lambda: A(B(6, 5), L(6), L(3), F(1), 0.25))
for _kind, _target in (("f32", lambda: F(6, 5)), ("i64", lambda: L(6, 5)), ("class", lambda: L(6))):
    case("bce_fwd", _kind, lambda t=_target: A(F(6, 5), t(), None))
    case("bce_fwd", _kind + "_idx", lambda t=_target: A(B(6, 8)[:, :5], t(), L(3), 0.25))
    case("bce_bwd", _kind, lambda t=_target: A(F(6, 5), t(), None, F(()), 1.0))
    case("bce_bwd", _kind + "_idx", lambda t=_target: A(B(6, 8)[:, :5], t(), L(3), F(1), 0.25))
case("rocauc_counts", "f32", lambda: A(F(6, 5), F(6, 5), None))
case("rocauc_counts", "i64_idx", lambda: A(B(6, 8)[:, :5], L(6, 5), L(3)))
case("rocauc_counts", "no_rows", lambda: A(F(6, 5), F(6, 5), L(0)))
case("argmax_count", "f32", lambda: A(F(6, 5), F(6), None))
case("argmax_count", "i64_idx_column", lambda: A(B(6, 8)[:, :5], L(6, 1), L(3)))
case("sum_n", "", lambda: A([F(6, 8), F(6, 16)[:, 8:], F(6, 16)[:, ::2]]))
# ---- head ----
case("combine_fc_supported", "f32", lambda: A(64, 7, torch.float32))
case("combine_fc_supported", "bf16", lambda: A(64, 7, torch.bfloat16))
case("combine_fc_supported", "bf16_wide", lambda: A(64, 172, torch.bfloat16))
case("combine_fc_supported", "f16", lambda: A(64, 7, torch.float16))
case("combine_fc_mapped_supported", "bf16", lambda: A(64, 7, torch.bfloat16))
case("combine_fc_mapped_supported", "f32", lambda: A(64, 7, torch.float32))
case("combine_fc_fwd", "plain", lambda: A(B(6, 8), 0.5, B(6, 8), 0.5, B(5, 8), F(5)))
case("combine_fc_fwd", "f32_high", lambda: A(F(6, 8), 0.75, F(6, 8), 0.25, F(8, 8), F(8)), **HIGH)
case("combine_fc_fwd", "mapped", lambda: A(B(6, 8), 0.5, B(6, 8), 0.5, B(5, 8), F(5), row_map=I(6)))
case("combine_fc_bwd", "plain", lambda: A(F(6, 5), B(5, 8), 0.5, 0.5, torch.bfloat16))
case("combine_fc_bwd", "f32_high", lambda: A(F(6, 8), F(8, 8), 0.75, 0.25, torch.float32), **HIGH)
case("combine_fc_bwd", "mapped", lambda: A(F(6, 5), B(5, 8), 0.5, 0.5, torch.bfloat16, row_map=I(6)))
case("combine_fc_bwd_g", "plain", lambda: A(F(6, 5), B(5, 8), 0.5, 0.5))
case("combine_fc_bwd_g", "mapped", lambda: A(F(6, 5), B(5, 8), 0.5, 0.5, row_map=I(6)))
# ---- GraphConv layer and stem ----
case("gcn_epilogue_supported", "bf16", lambda: A(64, 64, torch.bfloat16))
case("gcn_epilogue_supported", "f32", lambda: A(64, 32, torch.float32))
case("gcn_epilogue_supported", "f16", lambda: A(64, 64, torch.float16))
case("gcn_epilogue_stats", "plain", lambda: A(B(6, 8), B(8, 8), F(8)))
case("gcn_epilogue_stats", "stats", lambda: A(B(6, 8), B(8, 16)[:, :8], F(8), shift=F(8), want_stats=True))
case("gcn_epilogue_stats", "f32_high", lambda: A(F(6, 8), F(4, 8), F(4), shift=F(4), want_stats=True), **HIGH)
case("gcn_epilogue_cat", "one_pass", lambda: A(B(6, 8), B(6, 8), B(8, 16), F(8)))
case("gcn_epilogue_cat", "one_pass_stats", lambda: A(B(6, 8), B(6, 8), B(8, 16), F(8), shift=F(8), want_stats=True))
case("gcn_epilogue_cat", "switched_off", lambda: A(B(6, 8), B(6, 8), B(8, 16), F(8), shift=F(8), want_stats=True),
     env={"SGF_GCN_CAT": "0"})
case("gcn_epilogue_cat", "unsupported", lambda: A(B(6, 8), B(6, 8), B(8, 16), F(8)),
     results={"sgf_gcn_epilogue_cat_supported": 0})
case("gcn_epilogue_cat", "f32", lambda: A(F(6, 8), F(6, 4), F(8, 12), F(8), shift=F(8), want_stats=True))
case("gcn_epilogue_cat", "f32_high", lambda: A(F(6, 8), F(6, 4), F(8, 12), F(8)), **HIGH)
case("stem_pair_supported", "bf16", lambda: A(32, 64, torch.bfloat16))
case("stem_pair_supported", "f32", lambda: A(32, 64, torch.float32))
case("stem_pair", "pair_stats", lambda: A(B(6, 4), B(8, 4), F(8), B(8, 4), F(8), shift0=F(8), want_stats0=True))
case("stem_pair", "single", lambda: A(B(6, 4), B(8, 4), F(8), None, None))
case("gcn_epilogue_dx", "bf16_slice", lambda: A(B(6, 8), B(8, 16)[:, 8:]))
case("gcn_epilogue_dx", "f32_high", lambda: A(F(6, 8), F(8, 4)), **HIGH)
case("gcn_epilogue_dx2_acc_supported", "bf16", lambda: A(8, torch.bfloat16))
case("gcn_epilogue_dx2_acc_supported", "f32", lambda: A(8, torch.float32))
case("gcn_epilogue_dx2_acc", "full", lambda: A(B(6, 8), B(8, 16), B(6, 8), B(6, 8)))
case("gcn_epilogue_dx2_acc", "none", lambda: A(B(6, 8), B(8, 16), None, None))
case("gcn_bn_bwd_dx_supported", "bf16", lambda: A(8, torch.bfloat16))
case("gcn_bn_bwd_dx_supported", "f32", lambda: A(8, torch.float32))
case("gcn_bn_bwd_dx", "first", lambda: A(B(6, 8), B(6, 8), *_bn(), True, F(16), 0.125, True, B(8, 16), None, False, True))
case("gcn_bn_bwd_dx", "last", lambda: A(B(6, 8), B(6, 8), *_bn(), True, F(16), 0.125, True, B(8, 16), U(4096), True, False))
case("gcn_epilogue_dx2", "pair", lambda: A(B(6, 8), B(8, 16)[:, :8], B(8, 16)[:, 8:]))
case("gcn_epilogue_dx2", "f32_high_unpaired", lambda: A(F(6, 8), F(8, 16)[:, :8], F(8, 16)[:, 8:], pair=False), **HIGH)
case("axpby", "bf16", lambda: A(B(6, 8), 0.5, B(6, 8), 0.5))
case("axpby", "f32_views", lambda: A(F(6, 16)[:, :8], 0.75, F(6, 16)[:, 8:], 0.25))


# ---- the neighbour sampler's call sites (sgformer_amd/sampling.py), driven on a hand-made sampler ----
def _sampler(fanouts):
    from sgformer_amd import sampling
    s = object.__new__(sampling.NeighborSampler)
    s.rowptr, s.colind, s.local_of, s.max_deg = L(9), I(12), I(8), 2
    s.n, s.device, s.fanouts, s.seed, s.batches, s.host_reads = 8, CPU, list(fanouts), 99, 0, 0
    s._fan_dev = I(len(fanouts)) if all(k >= 0 for k in fanouts) else None
    s._fan_host = (ctypes.c_int32 * len(fanouts))(*fanouts)
    return s


def _sample(fanouts):
    s = _sampler(fanouts)
    return (I(3),), {}, s.sample, [s.rowptr, s.colind, s.local_of]


case("NeighborSampler.sample", "one_call", lambda: _sample([3, 2]))
case("NeighborSampler.sample", "hop_by_hop", lambda: _sample([2, -1]))
case("NeighborSampler.sample", "one_call_edge_list_only", lambda: _sample([3, 2]), env={"SGF_SAMPLED_CSR": "0"})


# ------------------------------------------------------------------------------------------------
# recording
# ------------------------------------------------------------------------------------------------
def _forget_memoised_queries(kernels):
    """Each case records the queries it depends on, whether or not the table memoises their answers."""
    for name in ("_x3_cache", "_constant_bytes"):
        getattr(kernels, name, {}).clear()
    for name, v in list(vars(kernels.HipKernels).items()):
        if name.endswith("_ws_bytes") and isinstance(v, int):
            setattr(kernels.HipKernels, name, None)


def record_all():
    """{case id: {"calls": [[entry, [normalised arguments]], ...], "returns": ... | "raises": exception name}}"""
    from sgformer_amd import _lib, kernels
    rec = Recorder()
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_lib, "_lib", rec.library(_lib.SIGNATURES))
        mp.setattr(torch.cuda, "current_stream", lambda device=None: NS(cuda_stream=STREAM))
        mp.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
        mp.setattr(torch.cuda, "current_device", lambda: 0)
        for var in ("SGF_GCN_CAT", "SGF_GRAM_PAIR", "SGF_SAMPLED_CSR"):
            mp.delenv(var, raising=False)
        precision = torch.get_float32_matmul_precision()
        try:
            for cid, method, build, options in CASES:
                _forget_memoised_queries(kernels)
                kernels._workspaces.clear()
                rec.calls, rec.keep, rec.results = [], [], options.get("results", {})
                torch.set_float32_matmul_precision(options.get("precision", "highest"))
                built = build()
                args, kwargs = built[:2]
                fn = built[2] if len(built) > 2 else getattr(kernels.HipKernels, method)
                ins = _flatten([list(built[3]) if len(built) > 3 else [], args, kwargs], [])
                with pytest.MonkeyPatch.context() as env:
                    for k, v in options.get("env", {}).items():
                        env.setenv(k, v)
                    try:
                        ret, entry = fn(*args, **kwargs), {}
                    except (TypeError, ValueError) as e:
                        ret, entry = None, {"raises": type(e).__name__}
                rets, others = _flatten(ret, []), {}
                entry["calls"] = [[name, [_normalise(r, ins, rets, kernels._workspaces, others) for r in raw]]
                                  for name, raw in rec.calls]
                entry.setdefault("returns", _describe(ret))
                out[cid] = entry
        finally:
            torch.set_float32_matmul_precision(precision)
            kernels._workspaces.clear()
            _forget_memoised_queries(kernels)
    return json.loads(json.dumps(out))


def _dump(recorded):
    return "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in recorded.items()) + "\n}\n"


@pytest.fixture(scope="module")
def recorded():
    return record_all()


# ------------------------------------------------------------------------------------------------
# the tests
# ------------------------------------------------------------------------------------------------
def test_calls_match_the_golden_file(recorded):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert list(recorded) == list(golden), set(recorded) ^ set(golden)
    wrong = [cid for cid in golden if recorded[cid] != golden[cid]]
    first = wrong[0] if wrong else None
    assert not wrong, (f"{len(wrong)} cases differ: {wrong}\nfirst, recorded: {json.dumps(recorded.get(first))}\n"
                       f"first, golden:   {json.dumps(golden.get(first))}")


def test_every_launch_ends_in_the_stream_and_names_no_unknown_pointer_kind(recorded):
    """Every entry that takes a stream gets the current one, last; every pointer is accounted for."""
    from sgformer_amd import _lib
    for cid, entry in recorded.items():
        for name, args in entry["calls"]:
            res, argtypes = _lib.SIGNATURES[name]
            if res is ctypes.c_int32 and argtypes and argtypes[-1] is ctypes.c_void_p and not name.endswith("_supported"):
                assert args[-1] == "stream", (cid, name)
            assert "stream" not in args[:-1], (cid, name)


def test_every_public_method_is_driven():
    from sgformer_amd.kernels import HipKernels
    public = {n for n in vars(HipKernels) if not n.startswith("_") and callable(getattr(HipKernels, n))} - {"check"}
    driven = {method for _cid, method, _b, _o in CASES}
    assert len(NOT_DRIVEN) <= 4 and set(NOT_DRIVEN) <= public
    assert public - driven == set(NOT_DRIVEN), sorted(public - driven - set(NOT_DRIVEN))
    assert len(public) >= 80


def test_every_entry_the_table_names_is_called(recorded):
    """Every sgf_* entry that sgformer_amd/kernels.py names in code (attribute of the library or entry name as a string) is
    called by at least one case."""
    from sgformer_amd import _lib, kernels
    named = set()
    for node in ast.walk(ast.parse(inspect.getsource(kernels))):
        if isinstance(node, ast.Attribute) and node.attr in _lib.SIGNATURES:
            named.add(node.attr)
        elif isinstance(node, ast.Constant) and isinstance(node.value, str) and node.value in _lib.SIGNATURES:
            named.add(node.value)
    called = {name for entry in recorded.values() for name, _args in entry["calls"]}
    assert named - called == set(), sorted(named - called)
    assert len(named) >= 120


def test_case_ids_are_unique():
    ids = [cid for cid, _m, _b, _o in CASES]
    assert len(ids) == len(set(ids))


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_kernel_table_host.py --write")
    with open(GOLDEN, "w") as f:
        f.write(_dump(record_all()))
    print(f"wrote {os.path.relpath(GOLDEN, ROOT)}")
