"""tests/fp8_linear_oracle.py against torch on the CPU: the decoder, the scaled product, the bound's ingredients, and that the
exact-data recipe is what it says (every partial sum in every order an fp32 number)."""
import numpy as np
import pytest
import torch

import fp8_linear_oracle as O


def test_decode_is_torchs_e4m3fn():
    codes = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(codes).view(torch.float8_e4m3fn).double().numpy()
    got = O.decode_e4m3fn(codes)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and int(np.isnan(got).sum()) == 2
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok]) and np.array_equal(np.signbit(got[ok]), np.signbit(want[ok]))


def test_encode_exact_round_trips_and_refuses_other_values():
    v = np.array([[0.0, 0.5, -1.5, 2.0, 448.0, -2.0 ** -9]])
    assert np.array_equal(O.decode_e4m3fn(O.encode_exact(v)), v)
    with pytest.raises(AssertionError):
        O.encode_exact(np.array([0.3]))


@pytest.mark.parametrize('M,N,K,per_token,per_channel', [(5, 7, 128, True, True), (3, 130, 384, False, True), (17, 16, 256, True, False)])
def test_gemm_matches_torch_on_random_data(M, N, K, per_token, per_channel):
    a, a_s, b, b_s = O.random_case(M, N, K, seed=M + N)
    if not per_token:
        a_s = a_s[:1]
    if not per_channel:
        b_s = b_s[:1]
    E, P = O.gemm(a, a_s, b, b_s)
    A = torch.from_numpy(a).view(torch.float8_e4m3fn).double()
    B = torch.from_numpy(b).view(torch.float8_e4m3fn).double()
    sa, sb = torch.from_numpy(a_s).double(), torch.from_numpy(b_s).double()
    want = (A @ B.T) * sa[:, None] * sb[None, :]
    wantP = (A.abs() @ B.abs().T) * sa[:, None] * sb[None, :]
    # float64 sums of at most 384 products of 8-bit numbers: the two evaluations differ by a few ulp of float64 at most
    assert np.abs(E - want.numpy()).max() <= 1e-12 * P.max() and np.abs(P - wantP.numpy()).max() <= 1e-12 * P.max()
    assert (np.abs(E) <= P * (1 + 1e-12)).all()


def test_bound_terms():
    assert O.c_acc(128) == pytest.approx(7 * 2.0 ** -13 + 135 * 2.0 ** -23, rel=1e-4) and O.c_acc(4096) < 7 * 2.0 ** -13 + 4104 * 2.0 ** -23 * 1.001
    E, P = np.array([[1.0, -2.0]]), np.array([[3.0, 2.0]])
    b = O.bound(E, P, 128, 'bf16')
    assert np.allclose(b, O.c_acc(128) * P + (2.0 ** -23 + 2.0 ** -8) * np.abs(E), rtol=0, atol=0)
    bb = O.bound(E, P, 128, 'f16', bias=np.array([1.0, 2.0]))
    assert np.allclose(bb - O.bound(E, P, 128, 'f16'), 2.0 ** -11 * np.array([[2.0, 0.0]]), rtol=0, atol=1e-18)
    assert np.array_equal(O.expected(E, np.array([1.0, 2.0])), np.array([[2.0, 0.0]]))


@pytest.mark.parametrize('M,N,K', [(1, 16, 128), (17, 130, 384), (33, 65, 1152)])
def test_exact_recipe_is_exact_in_any_order(M, N, K):
    a, a_s, b, b_s = O.exact_case(M, N, K, seed=K)
    ok, ratio = O.exact_in_any_order(a, b)
    assert ok and ratio <= 4 * K / O.EXACT_QUANTUM          # |a b| <= 4
    assert set(np.unique(O.decode_e4m3fn(a))) <= set(O.EXACT_VALUES)
    assert (np.log2(a_s) == np.round(np.log2(a_s))).all() and (np.log2(b_s) == np.round(np.log2(b_s))).all()
    E, P = O.gemm(a, a_s, b, b_s)
    # E is an fp32 number (a multiple of 0.25 below 2^24 quanta times a power of two), and so is every partial sum: fp32
    # summation in three different orders returns it bit for bit
    assert np.array_equal(E.astype(np.float32).astype(np.float64), E)
    A, B = O.decode_e4m3fn(a).astype(np.float32), O.decode_e4m3fn(b).astype(np.float32)
    sc = (O._col(a_s, M)[:, None] * O._col(b_s, N)[None, :]).astype(np.float32)
    prod = A[:, None, :] * B[None, :, :]                                     # [M, N, K] exact fp32 products
    fwd = np.zeros((M, N), np.float32)
    for k in range(K):
        fwd = fwd + prod[:, :, k]
    bwd = np.zeros((M, N), np.float32)
    for k in reversed(range(K)):
        bwd = bwd + prod[:, :, k]
    g = np.random.default_rng(0).permutation(K)
    rnd = np.zeros((M, N), np.float32)
    for k in g:
        rnd = rnd + prod[:, :, k]
    for s in (fwd, bwd, rnd):
        assert np.array_equal((s * sc).astype(np.float64), E)
