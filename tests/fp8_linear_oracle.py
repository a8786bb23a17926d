"""numpy oracle of llmc_fp8_scaled_gemm (csrc/fp8_linear.hip): OCP e4m3fn codes decoded to float64, the scaled product and the
scaled sum of absolute products in float64, and the bound the device result is held to.

    E[m, n] = a_s[m] b_s[n] sum_k a[m, k] b[n, k]          P[m, n] = a_s[m] b_s[n] sum_k |a[m, k] b[n, k]|
    |C - E| <= c_acc(K) P + 2 * 2^-24 |E| + u_out |E|  (+ u_out |E + bias| with a bias)

Where the terms come from — nothing here is fitted to what the kernel returns:

  c_acc(K) P   The kernels issue the NON-scaled matrix instructions (v_mfma_f32_32x32x16_fp8_fp8 on the tile rungs,
               v_mfma_f32_16x16x32_fp8_fp8 on the decode rung). A product of two e4m3 numbers has at most 8 significant bits
               and is exact in fp32 — but the instruction does not add the products at fp32 width. Measured with one-product
               probes (256 + 2^-j; the same window K22 found in the block-scaled form): the 8 products of the 8
               consecutive operand bytes one lane hands an instruction are aligned to the largest of them, and what lies more
               than 13 binary places below its leading bit is cut off (256 + 2^-5 came back exact, 256 + 2^-6 as 256); the
               sums of different lanes' groups, of different instructions and the accumulator meet at fp32 width
               (256 + 2^-15 exact). The bound follows from that window, not from the kernel's observed error:
                 window   each of the other 7 products of a group loses less than 2^-13 of the largest product's leading bit,
                          so a group loses less than 7 * 2^-13 max |a b| <= 7 * 2^-13 sum_group |a b|; over all groups
                          7 * 2^-13 sum |a b|. Which k a group holds does not matter to this bound.
                 adds     the group sums, the accumulator and (decode rung) the 8 K slices are added in an order that is not
                          documented, every addition returning an fp32 number with a relative error of at most one ulp,
                          u = 2^-23 (a truncating adder; round to nearest would be 2^-24): the classical bound for n - 1
                          additions is gamma(n - 1) sum |terms|, gamma(n) = n u / (1 - n u), taken with n = K + 8 (as if every
                          product were its own term: an upper bound on K / 8 group sums + 8 slices).
                   c_acc(K) = 7 * 2^-13 + gamma(K + 7),   u = 2^-23.
               The scales are applied afterwards, so the bound on the accumulator carries over to P = a_s b_s sum |a b|.
  2 * 2^-24    fl(fl(acc * a_s) * b_s): two fp32 products, each rounded to nearest.
  u_out        one rounding to the output format, half a unit in its last place: 2^-8 (bf16: 8 significant bits), 2^-11 (fp16), 2^-24 (fp32, where it stands for nothing more than
               the slack of stating the two products' roundings against E instead of against the accumulator).
  bias         added in the output format after that rounding: one more rounding of |E + bias|.

Exact data (exact_case): codes from {0, +-0.5, +-1, +-1.5, +-2} and power-of-two scales. Every product is a multiple of 0.25, so
every partial sum in every order is a multiple of 0.25 of magnitude <= sum |a b|; it is an fp32 number as soon as
sum |a b| / 0.25 < 2^24 (exact_in_any_order checks exactly that). The non-zero products lie between 0.25 and 4, five binary
places apart at the most: nothing reaches the 13-place window. The device result must then be E rounded once.
"""
import numpy as np

U_OUT = {'f32': 2.0 ** -24, 'bf16': 2.0 ** -8, 'f16': 2.0 ** -11}
U_ACC = 2.0 ** -23
DECODE_SLICES = 8
WINDOW_BITS = 13          # binary places below the leading bit of a group's largest product that survive
GROUP = 8                 # products per lane and instruction


def decode_e4m3fn(codes):
    """uint8 OCP e4m3fn codes -> float64 (0x7f / 0xff: NaN; no infinities)."""
    c = np.asarray(codes, dtype=np.uint8).astype(np.int64)
    e, m = (c >> 3) & 15, c & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * 2.0 ** (e - 7.0))
    mag = np.where((e == 15) & (m == 7), np.nan, mag)
    return np.where(c >> 7 == 1, -mag, mag)


def encode_exact(values):
    """values that ARE e4m3fn numbers -> codes (asserted: nothing is rounded here)."""
    v = np.asarray(values, dtype=np.float64)
    table = decode_e4m3fn(np.arange(256, dtype=np.uint8))
    codes = np.zeros(v.shape, dtype=np.uint8)
    hit = np.zeros(v.shape, dtype=bool)
    for c in list(range(0, 0x7f)) + list(range(0x80, 0xff)):
        if c == 0x80:
            continue                       # -0: +0 stands for zero
        sel = v == table[c]
        codes[sel] = c
        hit |= sel
    assert hit.all(), 'encode_exact: a value is not an e4m3fn number'
    return codes


def _col(s, n):
    s = np.asarray(s, dtype=np.float64).reshape(-1)
    assert s.size in (1, n)
    return np.broadcast_to(s, (n,)) if s.size == 1 else s


def gemm(a_codes, a_s, b_codes, b_s):
    """(E, P) in float64. a_codes [M, K], b_codes [N, K]; a_s [M] or [1], b_s [N] or [1]."""
    A, B = decode_e4m3fn(a_codes), decode_e4m3fn(b_codes)
    sc = _col(a_s, A.shape[0])[:, None] * _col(b_s, B.shape[0])[None, :]
    return (A @ B.T) * sc, (np.abs(A) @ np.abs(B).T) * np.abs(sc)


def c_acc(K):
    n = K + DECODE_SLICES - 1
    return (GROUP - 1) * 2.0 ** -WINDOW_BITS + n * U_ACC / (1.0 - n * U_ACC)


def bound(E, P, K, dt, bias=None):
    b = c_acc(K) * P + 2.0 * 2.0 ** -24 * np.abs(E) + U_OUT[dt] * np.abs(E)
    if bias is not None:
        b = b + U_OUT[dt] * np.abs(E + np.asarray(bias, dtype=np.float64)[None, :])
    return b


def expected(E, bias=None):
    """what the result is compared with: E, plus the bias where there is one"""
    return E if bias is None else E + np.asarray(bias, dtype=np.float64)[None, :]


# ---- exact data ------------------------------------------------------------------------------------------------------
EXACT_VALUES = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0])
EXACT_QUANTUM = 0.25


def exact_case(M, N, K, seed, a_per_token=True, b_per_channel=True):
    """codes and power-of-two scales (fp32) of the exact-data recipe"""
    g = np.random.default_rng(seed)
    a = encode_exact(g.choice(EXACT_VALUES, size=(M, K)))
    b = encode_exact(g.choice(EXACT_VALUES, size=(N, K)))
    a_s = (2.0 ** g.integers(-3, 4, size=M if a_per_token else 1)).astype(np.float32)
    b_s = (2.0 ** g.integers(-3, 4, size=N if b_per_channel else 1)).astype(np.float32)
    return a, a_s, b, b_s


def exact_in_any_order(a_codes, b_codes):
    """(ok, ratio): every partial sum of every output, in any order, is an fp32 number: sum |a b| / quantum < 2^24, the products
    being multiples of the quantum (asserted)."""
    A, B = decode_e4m3fn(a_codes), decode_e4m3fn(b_codes)
    assert np.array_equal(np.round(A / 0.5), A / 0.5) and np.array_equal(np.round(B / 0.5), B / 0.5), 'operands are multiples of 0.5'
    ratio = float((np.abs(A) @ np.abs(B).T).max() / EXACT_QUANTUM)
    return ratio < 2.0 ** 24, ratio


# ---- random data -----------------------------------------------------------------------------------------------------
def random_case(M, N, K, seed):
    """Random normal operands, a few rows of each scaled by 2^+-6, quantized per row to e4m3fn the way a per-token / per-channel
    quantizer does (scale = absmax / 448 in fp32, code = nearest e4m3fn number of x / scale by torch's cast)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    out = []
    for rows in (M, N):
        x = torch.randn(rows, K, generator=g)
        pick = torch.randperm(rows, generator=g)[:max(1, rows // 8)]
        x[pick] *= 2.0 ** torch.where(torch.rand(pick.numel(), generator=g) < 0.5, -6.0, 6.0)[:, None]
        cols = torch.randperm(K, generator=g)[:4]
        x[:, cols] *= 2.0 ** 6
        s = (x.abs().amax(dim=1) / 448.0).clamp(min=1e-12)
        codes = (x / s[:, None]).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
        out += [codes, s.numpy().astype(np.float32)]
    return tuple(out)
