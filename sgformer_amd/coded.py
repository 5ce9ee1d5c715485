"""The kernel-table methods of the SpMM that gathers lossless 12-bit coded operand rows (include/sgf.h: sgf_spmm_code_rows,
sgf_spmm_code_values, sgf_spmm_coded; csrc/spmm_coded.hip, csrc/spmm.hip: k_spmm_row_coded).  They hang on the HIP table as
K.spmm_coded_supported / K.spmm_code_rows / K.spmm_code_values / K.spmm_coded (install(), called where the table is made):
the CPU table of the tests has none of them, and graph.spmm_on asks with hasattr as it does for every optional method."""
from __future__ import annotations

import torch

from . import _lib
from . import kernels as _k

_BF16 = torch.bfloat16

# set to a list to record (launch class, device int32 [1] count of escaped rows, rows) per prepared operand: the escape
# shares of profiles/spmm_coded_escapes.md.  Nothing in a step reads the counts on the host.
escape_log = None


def spmm_coded_supported(x_shape, dtype) -> bool:
    """Would sgf_spmm_coded gather the slots for a contiguous operand of this shape (else it runs sgf_spmm_split's kernels on
    the dense rows)?  The launcher's own rule, SGF_SPMM_CODED included."""
    n, d = int(x_shape[0]), int(x_shape[1])
    if dtype != _BF16 or n == 0:
        return False
    return bool(_lib.load().sgf_spmm_coded_supported(d, _k._dtype_code(dtype), d, d, n, 1))


def spmm_code_rows(x: torch.Tensor):
    """(slots uint8 [n * 384], scale uint8 [n], n_escaped int32 [1]) of a bf16 [n, 256] operand with contiguous rows."""
    n, d = x.shape
    if x.dtype != _BF16 or d != 256 or x.stride(1) != 1:
        raise ValueError("spmm_code_rows: bf16 rows of 256 contiguous columns")
    dev = x.device
    slots = torch.empty(max(int(_lib.load().sgf_spmm_coded_bytes(n)), 1), dtype=torch.uint8, device=dev)
    scale = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    n_escaped = torch.empty(1, dtype=torch.int32, device=dev)
    _k._launch(dev, "sgf_spmm_code_rows", x, x.stride(0), n, slots, scale, n_escaped)
    return slots, scale, n_escaped


def spmm_code_values(colind: torch.Tensor, val: torch.Tensor, scale: torch.Tensor):
    """(val' fp32 [nnz], n_unsupported int32 [1]): the stored values with the source rows' scales folded in, escape-tagged."""
    dev, nnz = val.device, int(val.numel())
    val_coded = torch.empty(max(nnz, 1), dtype=torch.float32, device=dev)
    n_unsupported = torch.empty(1, dtype=torch.int32, device=dev)
    _k._launch(dev, "sgf_spmm_code_values", colind, val, nnz, scale, val_coded, n_unsupported)
    return val_coded, n_unsupported


def spmm_coded(rowptr, colind, val, val_coded, x: torch.Tensor, slots, n_unsupported, n_rows: int,
               long_segments: int = 0) -> torch.Tensor:
    """K.spmm(rowptr, colind, val, x, n_rows, long_segments=...) bit for bit, gathering the coded `slots` of x (and the dense
    rows of x for escape-tagged entries) wherever the launch allows and no stored value is negative (decided on the device)."""
    x = _k._rows(x)
    d = x.shape[1]
    y = torch.empty((n_rows, d), dtype=x.dtype, device=x.device)
    if n_rows == 0 or d == 0:
        return y
    _k._launch(x.device, "sgf_spmm_coded", rowptr, colind, val, val_coded, x, x.stride(0), x.shape[0], slots, n_unsupported, y,
               y.stride(0), n_rows, d, _k._code(x), _k.LONG_ROW, long_segments,
               *_k._long_row_scratch(x.device, long_segments, d))
    _k.counters["spmm_coded"] += 1
    return y


def install(table):
    """The four methods as attributes of one HIP kernel table."""
    table.spmm_coded_supported = spmm_coded_supported
    table.spmm_code_rows = spmm_code_rows
    table.spmm_code_values = spmm_code_values
    table.spmm_coded = spmm_coded
    return table
