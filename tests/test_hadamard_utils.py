"""hadamard_utils without a GPU: the factor matrices (built, not tabulated) are Hadamard matrices and equal an independent second
construction; the factor chosen for a size follows the reference's order of divisibility tests; the signs of
random_hadamard_matrix are the reference's draw; the oracle's factorised transform equals the literal Kronecker product; bad
arguments to llmc_hadamard are refused before anything touches a GPU."""
import numpy as np
import pytest
import torch

import hadamard_oracle as O


@pytest.mark.parametrize('K', [12, 20, 28, 36, 60])
def test_factor_matrices_are_hadamard_and_match_the_second_construction(K):
    from llmc_amd.compression.quantization.hadamard_utils import get_hadK
    n = K if K == 20 else K * 8          # 20 * 2^k is divisible by 40, which the reference tests first
    H, k = get_hadK(n)
    assert k == K and H.dtype == torch.float32 and tuple(H.shape) == (K, K)
    assert O.is_hadamard(H.numpy())
    assert np.array_equal(H.numpy().astype(np.int64), O.paley(K))
    Ht, _ = get_hadK(n, transpose=True)
    assert torch.equal(Ht, H.T)


def test_factor_choice_follows_the_reference_order():
    from llmc_amd.compression.quantization.hadamard_utils import get_hadK, is_pow2
    # 384 = 12 * 32; 448 = 28 * 16; 14336 = 28 * 512 (Llama-3-8B); 28672 = 28 * 1024 (Llama-3-70B); 4096 = 2^12
    for n, K in ((384, 12), (448, 28), (14336, 28), (28672, 28), (4096, 1), (20, 20), (36 * 4, 36), (60 * 2, 60)):
        H, k = get_hadK(n)
        assert k == K and (H is None) == (K == 1), n
    assert is_pow2(1) and is_pow2(4096) and not is_pow2(0) and not is_pow2(384)
    # 13824 = 108 * 128 (Llama-1-13B): divisible by 36 and 12 too, but 108 is tested first — and refused, not replaced
    for n, K in ((13824, 108), (11008, 172), (52 * 64, 52), (40 * 16, 40), (156 * 8, 156), (140 * 4, 140)):
        with pytest.raises(NotImplementedError, match=str(K)):
            get_hadK(n)
    with pytest.raises(NotImplementedError):
        get_hadK(28 * 3)
    with pytest.raises(NotImplementedError):
        get_hadK(100)


@pytest.mark.parametrize('seed', [0, 1, 1234])
def test_signs_are_the_reference_draw(seed):
    from llmc_amd.compression.quantization.hadamard_utils import random_hadamard_matrix
    torch.manual_seed(seed)
    want = torch.randint(low=0, high=2, size=(256,)).to(torch.float64) * 2 - 1        # hadamard_utils.py:103-104 of the reference
    after = torch.rand(1)
    torch.manual_seed(seed)
    Q = random_hadamard_matrix(256, 'cpu')
    assert Q.n == 256 and Q.sigma.dtype == torch.float64 and torch.equal(Q.sigma, want)
    assert torch.equal(torch.rand(1), after)          # the generator advanced exactly as far


def test_oracle_factorised_transform_is_the_kronecker_product():
    rng = np.random.default_rng(0)
    for n, K in ((1, 1), (2, 1), (64, 1), (512, 1), (24, 12), (448, 28), (12, 12)):
        hk = None if K == 1 else O.paley(K)
        x = rng.integers(-8, 9, size=(3, n), dtype=np.int64)
        M = O.dense_M(n, hk)
        assert np.array_equal(O.apply_M(x, hk), x @ M.T)
        assert np.array_equal(O.apply_M(x.T.copy(), hk, axis=0), M @ x.T)
    # fact 2: W Q = T(W o sigma), Q^T W = T along the output axis of sigma[:, None] o W
    sigma = rng.integers(0, 2, size=448) * 2.0 - 1.0
    hk = O.paley(28)
    Q = O.dense_Q(sigma, hk)
    W = rng.standard_normal((5, 448))
    assert np.allclose(W @ Q, O.transform(W * sigma, hk), rtol=0, atol=1e-12)
    assert np.allclose(Q.T @ W.T, O.transform(sigma[:, None] * W.T, hk, axis=0), rtol=0, atol=1e-12)
    assert np.allclose(Q @ Q.T, np.eye(448) * (448 / O.fl32_sqrt(448) ** 2), rtol=0, atol=1e-12)


def test_bad_arguments_are_refused_without_touching_the_gpu():
    from llmc_amd import _ffi
    L = _ffi.lib()
    assert L.llmc_hadamard(None, None, 7, 1, 64, 1, None, 1, 1.0, None) == -22
    assert 'dtype' in _ffi.last_error()
    assert L.llmc_hadamard(None, None, _ffi.F32, 1, 0, 1, None, 1, 1.0, None) == -22
    assert L.llmc_hadamard(None, None, _ffi.F32, 1, 64, 0, None, 1, 1.0, None) == -22
    assert L.llmc_hadamard(None, None, _ffi.F32, 1, 64, 1, None, 1, 1.0, None) == -22 and 'null' in _ffi.last_error()
    assert L.llmc_hadamard(None, None, _ffi.F32, 1, 24, 1, None, 12, 1.0, None) == -22 and 'hadK' in _ffi.last_error()
    assert L.llmc_hadamard(None, None, _ffi.F32, 1, 512, 1, None, 128, 1.0, None) == -95 and 'K0 > 64' in _ffi.last_error()
    assert L.llmc_hadamard(None, None, _ffi.BF16, 1, 36, 1, None, 12, 1.0, None) == -95 and 'power of two' in _ffi.last_error()
    assert L.llmc_hadamard(None, None, _ffi.F32, 1, 100, 1, None, 1, 1.0, None) == -95
    assert L.llmc_hadamard(None, None, _ffi.F32, 1, 65536, 1, None, 1, 1.0, None) == -95 and 'resident' in _ffi.last_error()
    assert L.llmc_hadamard(None, None, _ffi.F32, 0, 64, 1, None, 1, 1.0, None) == 0            # nothing to do


def test_cpu_tensors_are_refused():
    from llmc_amd import _ffi
    from llmc_amd.compression.quantization.hadamard_utils import matmul_hadU
    with pytest.raises(_ffi.LlmcHipError):
        matmul_hadU(torch.zeros(4, 64))


# ---- the exact oracle of the scaled transforms and the case tables of the width tests (tests/hadamard_cases.py) ------------------
_DTYPES = (torch.float32, torch.float64, torch.float16, torch.bfloat16)


def test_exact_scaled_is_the_dense_product_rounded_the_same_way():
    """fl32(e) * fl32(scale) has 48 significant bits at the most, so the float64 product is exact and its conversion to float32
    is the single rounding of the fp32 multiplication; the F64 value is the correctly rounded rational product."""
    from fractions import Fraction
    rng = np.random.default_rng(1)
    for n, K in ((2, 1), (8, 1), (64, 1), (20, 20), (24, 12), (112, 28), (72, 36), (60, 60)):
        hk = None if K == 1 else O.paley(K)
        x = rng.integers(-8, 9, size=(3, n), dtype=np.int64)
        e = x @ O.dense_M(n, hk).T
        scale = 1.0 / O.fl32_sqrt(n)
        assert np.array_equal(O.apply_M(x, hk), e)
        s32 = float(np.float32(scale))
        p32 = (e.astype(np.float64) * s32).astype(np.float32)
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            got = O.exact_scaled(e, scale, dt)
            assert got.dtype == dt and torch.equal(got, torch.from_numpy(p32).to(dt)), (n, dt)
        got = O.exact_scaled(e, scale, torch.float64)
        want = np.array([[float(Fraction(int(v)) * Fraction(scale)) for v in row] for row in e])
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), want), n
        # scale 1 gives the integers back
        assert torch.equal(O.exact_scaled(e, 1.0, torch.float64), torch.from_numpy(e).double())
    with pytest.raises(AssertionError):
        O.exact_scaled(np.array([2 ** 24]), 1.0, torch.float32)


def test_every_width_case_keeps_its_sums_exact():
    """integer inputs in [-8, 8]: every entry of M_n x (and every partial sum: at most 8 n < 2^19) is an integer below 2^24"""
    import hadamard_cases as HC
    worst = 0
    for outer, n, inner, K0 in HC.KERNEL_CASES + [(r, n, 1, K0) for _, r, n, K0 in HC.UNALIGNED]:
        assert 8 * n < 2 ** 19 and n <= 36864
        hk = None if K0 == 1 else O.paley(K0)
        xi = HC.ints((outer, n, inner), HC.seed(outer, n, inner))
        assert np.abs(xi).max() <= 8
        e = O.apply_M(xi, hk, axis=1)
        assert e.dtype == np.int64 and np.abs(e).max() < 2 ** 24, (outer, n, inner, K0)
        worst = max(worst, int(np.abs(e).max()))
    print('largest |M_n x| over the cases:', worst)
    assert len(set(HC.KERNEL_CASES)) == len(HC.KERNEL_CASES)


def test_model_reachable_sizes_pick_the_tabulated_order():
    import hadamard_cases as HC
    from llmc_amd.compression.quantization.hadamard_utils import get_hadK
    for n, K in HC.MODEL_REACHABLE:
        H, k = get_hadK(n)
        assert k == K and (H is None) == (K == 1), n
        if K > 1:
            assert np.array_equal(H.numpy().astype(np.int64), O.paley(K))
    for out_f, in_f, had_dim, output in HC.LINEAR:
        if had_dim == -1:
            assert (out_f if output else in_f, get_hadK(out_f if output else in_f)[1]) in HC.MODEL_REACHABLE
    # sizes that need a factor matrix the kernel does not take are refused when the rotation is set up, before any launch:
    # 11008 = 172 * 64 (Llama-2-7B), 5120 = 40 * 128 and 13824 = 108 * 128 (Llama-2-13B), 40 heads (Llama-2-13B)
    for n, K in HC.REFUSED_SIZES:
        with pytest.raises(NotImplementedError, match=f'order-{K} '):
            get_hadK(n)


def test_a_partial_rotater_with_40_heads_is_refused_before_any_launch():
    from llmc_amd.compression.quantization.base_blockwise_quantization import BaseBlockwiseQuantization

    class Stub:
        intermediate_size, num_heads, hidden_size, fp32_had = 13824, 40, 5120, True
    for name in ('self_attn.o_proj', 'mlp.down_proj'):
        with pytest.raises(NotImplementedError):
            BaseBlockwiseQuantization.get_replacement_params(Stub(), mode='online_rotate', w_only=False, name=name)
