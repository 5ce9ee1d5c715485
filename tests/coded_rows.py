"""The 12-bit row code of sgf_spmm_code_rows / sgf_spmm_code_values / sgf_spmm_coded (include/sgf.h) in numpy — TEST ONLY.

A bf16 value is s | Ek (8 bits) | m (7 bits).  Per row of 256, E = the largest Ek among the finite non-zero (normal) elements,
15 if there is none; an element is coded s | e | m with e = Ek - (E - 15) in 1..15, a zero of either sign s | 0 | 0.  A row
escapes when an element is subnormal, Inf or NaN or has Ek < E - 14: scale byte 255, slot all zero.  Slot of 384 bytes:
dword l (byte 4 l):      bits 15..0  s0 | e2 | e0 | m0,   bits 31..16  s1 | e3 | e1 | m1      (columns 4l .. 4l+3)
half  l (byte 256 + 2l): bits  7..0  s2 | m2,             bits 15..8   s3 | m3
Decoding puts e into the low four bits of an fp32 exponent field: element = decoded * 2^(E - 15)."""
import numpy as np
import torch

D = 256
SLOT = 384
ESCAPED = 255
LENGTHS = (0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 23, 24, 25, 100)


def row_scale(rows: np.ndarray) -> np.ndarray:
    """uint16 [n, 256] -> uint8 [n]: E of every row, ESCAPED for the rows that are not coded."""
    rows = np.ascontiguousarray(rows, dtype=np.uint16)
    ek = ((rows >> 7) & 0xFF).astype(np.int64)
    m = (rows & 0x7F).astype(np.int64)
    bad = ((ek == 255) | ((ek == 0) & (m != 0))).any(axis=1)
    normal = ek != 0
    hi = np.where(normal, ek, 0).max(axis=1)
    lo = np.where(normal, ek, 255).min(axis=1)
    any_normal = normal.any(axis=1)
    E = np.where(any_normal, hi, 15)
    esc = bad | (any_normal & (lo + 14 < E))
    return np.where(esc, ESCAPED, E).astype(np.uint8)


def encode(rows: np.ndarray):
    """rows uint16 [n, 256] (bf16 bits) -> (slots uint8 [n, 384], scale uint8 [n], number of escaped rows)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint16)
    n = rows.shape[0]
    assert rows.shape == (n, D)
    scale = row_scale(rows)
    esc = scale == ESCAPED
    r = rows.astype(np.uint32)
    ek = (r >> 7) & 0xFF
    E = np.where(esc, 15, scale).astype(np.uint32)[:, None]
    e = np.where(ek != 0, ek + 15 - E, 0).astype(np.uint32) & 0xF
    c = (r & 0x807F) | (e << 7)                                   # s | 0000 | e | m, 16 bits
    c, e, r = c.reshape(n, 64, 4), e.reshape(n, 64, 4), r.reshape(n, 64, 4)
    w = c[:, :, 0] | (e[:, :, 2] << 11) | ((c[:, :, 1] | (e[:, :, 3] << 11)) << 16)
    sm = ((r >> 8) & 0x80) | (r & 0x7F)                           # s | m, 8 bits
    h = (sm[:, :, 2] | (sm[:, :, 3] << 8)).astype(np.uint16)
    slots = np.zeros((n, SLOT), dtype=np.uint8)
    slots[:, :256] = w.astype("<u4").view(np.uint8).reshape(n, 256)
    slots[:, 256:] = h.astype("<u2").view(np.uint8).reshape(n, 128)
    slots[esc] = 0
    return slots, scale, int(esc.sum())


def decode_floats(slots: np.ndarray) -> np.ndarray:
    """slots uint8 [n, 384] -> fp32 bits uint32 [n, 256]: what a lane of the gather multiplies (s << 31 | e << 23 | m << 16)."""
    slots = np.ascontiguousarray(slots, dtype=np.uint8)
    n = slots.shape[0]
    w = slots[:, :256].copy().view("<u4").astype(np.uint32)       # [n, 64]
    h = slots[:, 256:].copy().view("<u2").astype(np.uint32)       # [n, 64]
    out = np.zeros((n, 64, 4), dtype=np.uint32)
    out[:, :, 0] = (w << 16) & 0x87FF0000
    out[:, :, 1] = w & 0x87FF0000
    e2, e3 = (w >> 11) & 0xF, (w >> 27) & 0xF
    b2, b3 = h & 0xFF, (h >> 8) & 0xFF
    out[:, :, 2] = ((b2 & 0x80) << 24) | (e2 << 23) | ((b2 & 0x7F) << 16)
    out[:, :, 3] = ((b3 & 0x80) << 24) | (e3 << 23) | ((b3 & 0x7F) << 16)
    return out.reshape(n, D)


def decode(slots: np.ndarray, scale: np.ndarray) -> np.ndarray:
    """(slots, scale) -> rows uint16 [n, 256]; escaped rows come back as all 0xffff (not decodable)."""
    f = decode_floats(slots)
    e = (f >> 23) & 0xF
    E = scale.astype(np.uint32)[:, None]
    ek = np.where(e != 0, e + E - 15, 0)
    rows = (((f >> 16) & 0x807F) | (ek << 7)).astype(np.uint16)
    rows[scale == ESCAPED] = 0xFFFF
    return rows


def code_values(colind: np.ndarray, val: np.ndarray, scale: np.ndarray):
    """(val' float32 [nnz], number of val with the sign bit set, -0.0 included): val * 2^(E - 15) as an exponent-field addition
    where val is a normal float > 0, the source row is coded and the result is a normal float; else -val (sign bit flipped)."""
    u = np.ascontiguousarray(val, dtype=np.float32).view(np.uint32)
    E = scale[np.asarray(colind, dtype=np.int64)].astype(np.int64)
    ev = ((u >> 23) & 0xFF).astype(np.int64)
    en = ev + E - 15
    ok = ((u >> 31) == 0) & (ev >= 1) & (ev <= 254) & (E != ESCAPED) & (en >= 1) & (en <= 254)
    scaled = (u & 0x807FFFFF) | (np.clip(en, 0, 255).astype(np.uint32) << 23)
    out = np.where(ok, scaled, u ^ 0x80000000).astype(np.uint32)
    return out.view(np.float32), int((u >> 31).sum())


def bf16_bits(a: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bits uint16, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def gaussian(n, seed):
    return bf16_bits(np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32))


def gaussian_scaled(n, seed, span=30):
    """Gaussian rows times a per-row power of two out of 2^-span .. 2^span."""
    rng = np.random.default_rng(seed)
    s = np.ldexp(1.0, rng.integers(-span, span + 1, size=(n, 1))).astype(np.float32)
    return bf16_bits(rng.standard_normal((n, D)).astype(np.float32) * s)


def relu_relu(n, seed):
    """relu(n1) + relu(n2): a quarter exact zeros."""
    rng = np.random.default_rng(seed)
    a = np.maximum(rng.standard_normal((n, D)), 0) + np.maximum(rng.standard_normal((n, D)), 0)
    return bf16_bits(a.astype(np.float32))


def plant_escapes(rows: np.ndarray, which) -> np.ndarray:
    """A copy with the rows `which` made to escape, in turn by: an element 20 binades under the maximum, a subnormal, an Inf,
    a NaN."""
    rows = rows.copy()
    for k, i in enumerate(which):
        col = (37 * k) % D
        kind = k % 4
        if kind == 0:
            rows[i, col] = 0x3F80                                # 1.0 ...
            rows[i, (col + 1) % D] = 0x3F80 - (20 << 7)          # ... and 2^-20
        elif kind == 1:
            rows[i, col] = 0x0001
        elif kind == 2:
            rows[i, col] = 0x7F80
        else:
            rows[i, col] = 0x7FC1
    return rows


def ladder_csr(n, seed, long_row=None):
    """(lens, rowptr int64, colind int32, val float32 in [0.01, 1)): rows of every length of LENGTHS in turn, sources ascending
    inside a row, a self loop in every non-empty row, a duplicate source in every row of two or more, rows 0 and n - 1 among
    the sources of every row of 16 or more; `long_row` = (row, length) replaces one row by a long one."""
    rng = np.random.default_rng(seed)
    lens = [LENGTHS[i % len(LENGTHS)] for i in range(n)]
    if long_row is not None:
        lens[long_row[0]] = long_row[1]
    cols = []
    for i, k in enumerate(lens):
        c = rng.integers(0, n, size=k)
        if k >= 1:
            c[0] = i
        if k >= 2:
            c[1] = c[-1]
        if k >= 16:
            c[2], c[3] = 0, n - 1
        cols.append(np.sort(c))
    colind = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, dtype=np.int32)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    val = rng.uniform(0.01, 1.0, size=colind.size).astype(np.float32)
    return lens, torch.from_numpy(rowptr), torch.from_numpy(colind), torch.from_numpy(val)
