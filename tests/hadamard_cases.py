"""The shapes of tests/test_hadamard_widths_gpu.py and tests/test_quarot_widths_gpu.py, importable without a GPU: the CPU test
(tests/test_hadamard_utils.py) checks the exactness precondition of every case and the factor order of every size a model can
produce; the GPU tests run the same lists. A kernel case is (outer, n, inner, K0): llmc_hadamard on [outer, n, inner] with the
order-K0 factor matrix passed explicitly. What each case reaches in launch_had / k_had_rows / k_had_cols is stated next to it
(rpb: rows per workgroup, C: columns per workgroup, L = log2(n / K0))."""

# ---- k_had_rows, K0 == 1 ------------------------------------------------------------------------------------------------------------
ROWS_POW2 = [
    (3, 4, 1, 1),            # L = 2: a partial register butterfly
    (5, 8, 1, 1),            # L = 3: the register butterfly alone
    (5, 16, 1, 1),           # L = 4: the DPP xor-1 stage is the last stage
    (5, 32, 1, 1),           # L = 5: DPP xor-2 last
    (70, 256, 1, 1),         # L = 8: the ds_swizzle xor-16 stage last; 32 fp32 (16 fp64) rows per workgroup, the last one holds 6
    (9, 2048, 1, 1),         # L - 9 = 2: rows_high_bits<2>; 4 fp32 (2 fp64) rows per workgroup and a tail workgroup
    (3, 8192, 1, 1),         # L - 9 = 4: rows_high_bits<4>
    (2, 16384, 1, 1),        # L - 9 = 5: rows_high_bits<5>; 128 KiB of LDS in fp64
]

# ---- k_had_rows with a factor matrix ----------------------------------------------------------------------------------------------
ROWS_FACTOR = [
    (2, 20, 1, 20),          # L = 0, per-element mix; runs of 8 cross segments and rows
    (3, 40, 1, 20),          # L = 1, per-element mix
    (3, 80, 1, 20),          # L = 2, per-element mix
    (3, 160, 1, 20),         # L = 3: the shortest row on the vector mix
    (5, 3072, 1, 12),        # 2 fp32 rows per workgroup, the last workgroup holds 1
    (5, 5120, 1, 20),        # 10 waves
    (5, 4608, 1, 36),        # 9 waves
    (5, 7680, 1, 60),        # 15 waves
    (3, 15360, 1, 60),       # 137 280 B of LDS in fp64
    (2, 36864, 1, 36),       # 152 640 B in fp32, L - 9 = 1: the longest row with a factor that fits; F64 is refused
]

# ---- k_had_cols -----------------------------------------------------------------------------------------------------------------------
COLS = [
    (2, 4096, 40, 1),        # C = 2 (fp32) / 1 (fp64); four passes (s0 = 0, 3, 6, 9)
    (2, 8192, 9, 1),         # C = 1, odd inner; five passes, the last a radix-2 pass; 64 KiB in fp64
    (1, 16384, 3, 1),        # C = 1; five passes, the last a radix-4 pass; 128 KiB in fp64
    (3, 512, 24, 1),         # the s0 = 6 pass has three bits; C = 16 with a chunk of 8 left over
    (3, 1024, 130, 1),       # C = 8 (fp32) / 4 (fp64), 2 columns left over
    (2, 2048, 200, 1),       # C = 4 (fp32) / 2 (fp64)
    (2, 3584, 5, 28),        # C = 2 with one column left over (fp32), C = 1 (fp64)
    (2, 4608, 5, 36),        # C = 1 with the mix
    (2, 7680, 3, 60),        # C = 1 with the mix; 75 840 B in fp64
    (1, 14336, 3, 28),       # C = 1 with the mix; 117 824 B in fp64
    (3, 60, 7, 60),          # L = 0; C = 8 with 7 valid columns
]
# heads in the middle, [tokens, heads, 128]: the per-head online rotation of o_proj's input
HEADS = [(37, 32, 128, 1), (37, 64, 128, 1), (37, 28, 128, 28), (37, 24, 128, 12), (37, 20, 128, 20), (37, 36, 128, 36),
         (37, 12, 128, 12)]

KERNEL_CASES = ROWS_POW2 + ROWS_FACTOR + COLS + HEADS

# ---- unaligned views: (dtype name, rows, n, K0), a buffer of one element more sliced from 1 ---------------------------------------
UNALIGNED = [
    ('float32', 3, 1024, 1),         # scalar loads / stores around the LDS exchange
    ('float64', 3, 1024, 1),
    ('bfloat16', 5, 384, 12),        # around the K0 mix
    ('float16', 3, 8192, 1),         # around rows_high_bits<4>
]

# ---- random data against hadamard_oracle.bound ------------------------------------------------------------------------------------
RANDOM_CASES = [(3, 8192, 1, 1), (2, 7680, 1, 60), (2, 4096, 40, 1), (2, 3584, 5, 28), (37, 28, 128, 28)]

# ---- the Python layer: sizes a model produces, with the order get_hadK picks for them ("model-reachable") -------------------------
HIDDEN = [(4096, 1), (8192, 1), (3584, 28), (3072, 12)]                       # RandomHadamard.right / left_t (fp64)
LINEAR = [                                                                    # apply_exact_had_to_linear: (out, in, had_dim, output)
    (5, 14336, -1, False),           # down_proj: rows of 14336 = 28 * 512
    (256, 4096, 128, True),          # v_proj: two heads of 128 along the output axis, inner 4096
    (4096, 24, -1, True),            # the whole output axis
]
ROTATER_FULL = [(8192, 1), (12288, 12), (14336, 28)]                          # Rotater.rotate, full: [2, 37, n]
ROTATER_HEADS = [(12, 12), (20, 20), (24, 12), (28, 28), (32, 1), (36, 36), (64, 1)]      # partial: [2, 37, heads * 128]
HAD_DIM = 128
MODEL_REACHABLE = sorted(set(HIDDEN + ROTATER_FULL + ROTATER_HEADS + [(14336, 28), (4096, 1)]))
REFUSED_SIZES = [(11008, 172), (5120, 40), (13824, 108), (40, 40)]            # (size, the order that is refused); 40: heads


def seed(outer, n, inner):
    return n * 131 + outer * 7 + inner


def ints(shape, seed, lo=-8, hi=8):
    """the integer inputs of a case (int64): the CPU test checks the precondition on the very arrays the GPU test transforms"""
    import numpy as np
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape, dtype=np.int64)
