"""The packed row format of sgf_bn_apply_packed / sgf_spmm_packed (include/sgf.h) in numpy — TEST ONLY.

One slot of S bytes per bf16 row of 256 columns: bytes [0, 32) a mask, bit c (byte c // 8, bit c % 8) set iff the bf16 bits
of column c are not 0x0000; then the values of the set columns in column order, at most (S - 32) / 2; zero behind them.  A row
with more non-zeros than that overflows: its slot holds the values that fit and is not decodable."""
import numpy as np

D = 256
MASK_BYTES = 32


def capacity(slot_bytes: int) -> int:
    return (slot_bytes - MASK_BYTES) // 2


def encode(rows: np.ndarray, slot_bytes: int):
    """rows uint16 [n, 256] (bf16 bits) -> (slots uint8 [n, slot_bytes], number of overflowing rows)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint16)
    n = rows.shape[0]
    assert rows.shape == (n, D)
    cap = capacity(slot_bytes)
    slots = np.zeros((n, slot_bytes), dtype=np.uint8)
    present = rows != 0
    slots[:, :MASK_BYTES] = np.packbits(present, axis=1, bitorder="little")
    overflow = 0
    for i in range(n):
        vals = rows[i][present[i]]
        overflow += int(vals.size > cap)
        vals = vals[:cap]
        slots[i, MASK_BYTES:MASK_BYTES + 2 * vals.size] = vals.view(np.uint8)
    return slots, overflow


def counts(slots: np.ndarray) -> np.ndarray:
    """Non-zero count per row, from the masks."""
    return np.unpackbits(np.ascontiguousarray(slots[:, :MASK_BYTES]), axis=1, bitorder="little").sum(axis=1)


def decode(slots: np.ndarray) -> np.ndarray:
    """slots uint8 [n, S] -> rows uint16 [n, 256]; rows that overflow their slot come back as all 0xffff (not decodable)."""
    slots = np.ascontiguousarray(slots, dtype=np.uint8)
    n, slot_bytes = slots.shape
    cap = capacity(slot_bytes)
    present = np.unpackbits(slots[:, :MASK_BYTES], axis=1, bitorder="little").astype(bool)
    rows = np.zeros((n, D), dtype=np.uint16)
    for i in range(n):
        k = int(present[i].sum())
        if k > cap:
            rows[i] = 0xFFFF
            continue
        rows[i][present[i]] = slots[i, MASK_BYTES:MASK_BYTES + 2 * k].copy().view(np.uint16)
    return rows


def crafted_rows(slot_bytes: int, n: int, seed: int, overflow_row: bool = False) -> np.ndarray:
    """uint16 [n, 256]: random rows with about half of the columns zero (non-zero counts of both parities in front of every
    lane), and in rows 0-5: no non-zero; one, in the last column; exactly the capacity; -0.0 values (kept: their bits are not
    zero); the capacity with the last column set; and, with `overflow_row`, all 256 (else capacity - 1)."""
    rng = np.random.default_rng(seed)
    cap = capacity(slot_bytes)
    vals = (rng.standard_normal((n, D)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    vals[vals == 0] = 0x3F80
    rows = np.where(rng.random((n, D)) < 0.5, vals, 0).astype(np.uint16)
    rows[0] = 0
    rows[1] = 0
    rows[1, D - 1] = 0x4000
    rows[2] = 0
    rows[2, rng.permutation(D)[:cap]] = 0x3F80
    rows[3, ::7] = 0x8000                       # -0.0
    rows[4] = 0
    rows[4, D - cap:] = vals[4, D - cap:]
    rows[5] = vals[5]
    if not overflow_row:
        rows[5, rng.permutation(D)[:D - (cap - 1)]] = 0
    return rows
