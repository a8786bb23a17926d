"""Operand recipes shared by tests/test_mx_config.py (which checks them against the exactness condition on the CPU) and
tests/test_mx_gemm_gpu.py (which runs them)."""
import numpy as np

import mx_oracle as MX


def exact_operands(M, N, K, a_bit, seed):
    """(a codes [M, K], a_s, b codes [N, K], b_s), one code per byte, for which the block-scaled product is exact in fp32 in any
    summation order: weights over all 16 e2m1 codes; activations over all 16 e2m1 codes (K <= 4096) or the e4m3 integers
    -15 .. 15 (K <= 1024); a_s in {127, 128}, b_s in {126, 127, 128}: a_s + b_s spans the four values 253 .. 256."""
    assert K <= (4096 if a_bit == 'e2m1' else 1024)
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 16, (N, K)).astype(np.uint8)
    if a_bit == 'e2m1':
        a = rng.integers(0, 16, (M, K)).astype(np.uint8)
    else:
        a = MX.e4m3_encode(rng.integers(-15, 16, (M, K)).astype(np.float32))
    a_s = rng.integers(127, 129, (M, K // 32)).astype(np.uint8)
    b_s = rng.integers(126, 129, (N, K // 32)).astype(np.uint8)
    return a, a_s, b, b_s


def random_operands(M, N, K, a_bit, seed):
    """the full code sets (e4m3 without its two NaN codes) and a wide scale range"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 16, (N, K)).astype(np.uint8)
    if a_bit == 'e2m1':
        a = rng.integers(0, 16, (M, K)).astype(np.uint8)
    else:
        a = rng.integers(0, 256, (M, K)).astype(np.uint8)
        a[(a & 0x7f) == 0x7f] = 0x38
    a_s = rng.integers(97, 140, (M, K // 32)).astype(np.uint8)
    b_s = rng.integers(107, 134, (N, K // 32)).astype(np.uint8)
    return a, a_s, b, b_s


def pack(codes, bit):
    import fp4_oracle as O
    return O.pack_fp4(codes) if bit == 'e2m1' else np.ascontiguousarray(codes, dtype=np.uint8)
