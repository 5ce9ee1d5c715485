"""Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC11) in int64 torch tensors — TEST ONLY, the
host side of the keep decisions of csrc/gat.hip (tests/cpu_kernels_gat.py, tests/test_gat_host.py, tests/test_gpu_gat.py).  Every
intermediate stays below 2^49, so int64 never wraps; works on any device.  tests/test_gat_host.py holds it to the paper's
known-answer vectors."""
M32 = 0xFFFFFFFF
_MUL0, _MUL1 = 0xD2511F53, 0xCD9E8D57
_WEYL0, _WEYL1 = 0x9E3779B9, 0xBB67AE85


def mul_hi_lo(a, c):
    """(high, low) 32 bits of a * c for a Python int a < 2^32 and an int64 tensor c in [0, 2^32): 16-bit limbs"""
    a0, a1 = a & 0xFFFF, a >> 16
    c0, c1 = c & 0xFFFF, c >> 16
    mid = c0 * a1 + c1 * a0                              # < 2^33
    low = c0 * a0 + ((mid & 0xFFFF) << 16)               # < 2^33
    return c1 * a1 + (mid >> 16) + (low >> 32), low & M32


def philox4x32_10(counter, key):
    """counter: four int64 tensors in [0, 2^32); key: two Python ints.  Returns the four output words as int64 tensors."""
    x0, x1, x2, x3 = counter
    k0, k1 = key[0] & M32, key[1] & M32
    for _ in range(10):
        h0, l0 = mul_hi_lo(_MUL0, x0)
        h1, l1 = mul_hi_lo(_MUL1, x2)
        x0, x1, x2, x3 = h1 ^ x1 ^ k0, l1, h0 ^ x3 ^ k1, l0
        k0, k1 = (k0 + _WEYL0) & M32, (k1 + _WEYL1) & M32
    return x0, x1, x2, x3
