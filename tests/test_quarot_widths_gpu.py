"""The Python layer of the rotations (RandomHadamard, apply_exact_had_to_linear, Rotater) at model widths, bit for bit.

tests/test_quarot_gpu.py runs it at the toy model's 256 / 448 / 4 heads of 64 and compares the scaled fp32 transforms with a
rounding bound, inside which a scale one ulp off or applied at the wrong point would stay. Here the inputs are small integers
(times a power of two for the fp64 rotations), so every sum is exact in any order and the result is determined: one
multiplication by the scale and one rounding (hadamard_oracle.exact_scaled), then the cast back to the module's dtype where the
code casts. Sizes and the factor order get_hadK picks for each are in tests/hadamard_cases.py (checked on the CPU by
tests/test_hadamard_utils.py; the sizes that are refused, and a partial Rotater with 40 heads, are asserted there too):

  RandomHadamard.right [5, n], left_t [n, 9] and [n] in fp64, n = 4096, 8192 (order 1), 3584 (28), 3072 (12): the hidden axis;
      left_t is k_had_cols with one column per workgroup, or k_had_rows on a single row for a vector
  apply_exact_had_to_linear on bf16 Linears: down_proj with 14336 = 28 * 512 inputs; v_proj in heads of 128 along the output axis
      ([2, 128, 4096]); the whole output axis of 4096
  Rotater.rotate on bf16 / fp16 [2, 37, n]: full with n = 8192, 12288 = 12 * 1024, 14336; partial with 12, 20, 24, 28, 32, 36, 64
      heads of 128; both fp32_had settings, which round the same fp32 value once and so must give the same bits."""
import math

import numpy as np
import pytest
import torch

import hadamard_cases as HC
import hadamard_oracle as O

pytestmark = pytest.mark.gpu


def _hk(K):
    return None if K == 1 else O.paley(K)


@pytest.mark.parametrize('n,K', HC.HIDDEN)
def test_random_hadamard_rotations_in_fp64_bit_for_bit(n, K):
    from llmc_amd.compression.quantization.hadamard_utils import random_hadamard_matrix, rotate_left_t, rotate_right
    torch.manual_seed(n)
    want_sigma = torch.randint(low=0, high=2, size=(n,)).to(torch.float64) * 2 - 1
    torch.manual_seed(n)
    Q = random_hadamard_matrix(n, 'cuda')
    assert torch.equal(Q.sigma.cpu(), want_sigma)
    sigma = want_sigma.numpy().astype(np.int64)
    scale = 1.0 / O.fl32_sqrt(n)

    def want(e):          # fl64((M_n (ints o sigma)) 2^-7 scale): the sums and the power of two are exact, one rounding
        assert np.abs(e).max() < 2 ** 24
        return torch.from_numpy(np.ascontiguousarray((e.astype(np.float64) * 2.0 ** -7) * scale))

    wi = HC.ints((5, n), n + 1, -127, 127)
    W = (torch.from_numpy(wi).double() * 2.0 ** -7).cuda()
    got = rotate_right(W, Q)
    assert got.dtype == torch.float64 and torch.equal(got.cpu(), want(O.apply_M(wi * sigma, _hk(K))))
    assert torch.equal(W.cpu(), torch.from_numpy(wi).double() * 2.0 ** -7)
    wi = HC.ints((n, 9), n + 2, -127, 127)
    W = (torch.from_numpy(wi).double() * 2.0 ** -7).cuda()
    got = rotate_left_t(W, Q)
    assert got.shape == W.shape and torch.equal(got.cpu(), want(O.apply_M(wi * sigma[:, None], _hk(K), axis=0)))
    assert torch.equal(W.cpu(), torch.from_numpy(wi).double() * 2.0 ** -7)
    wi = HC.ints((n,), n + 3, -127, 127)
    b = (torch.from_numpy(wi).double() * 2.0 ** -7).cuda()
    got = rotate_left_t(b, Q)
    assert got.shape == b.shape and torch.equal(got.cpu(), want(O.apply_M(wi * sigma, _hk(K))))


@pytest.mark.parametrize('out_f,in_f,had_dim,output', HC.LINEAR)
@pytest.mark.parametrize('device', ['cuda', 'cpu'])
def test_apply_exact_had_to_linear_bit_for_bit(out_f, in_f, had_dim, output, device):
    from llmc_amd.compression.quantization.hadamard_utils import apply_exact_had_to_linear, get_hadK
    dtype = torch.bfloat16
    wi = HC.ints((out_f, in_f), out_f * 31 + in_f)
    l = torch.nn.Linear(in_f, out_f, bias=False).to(dtype)
    l.weight.data = torch.from_numpy(wi).to(dtype)
    l = l.to(device)
    if had_dim == -1:
        n = out_f if output else in_f
        K = get_hadK(n)[1]
        e = O.apply_M(wi, _hk(K), axis=0 if output else 1)
        scale = 1.0 / O.fl32_sqrt(n)
    else:
        e = O.apply_M(wi.reshape(out_f // had_dim, had_dim, in_f), None, axis=1).reshape(out_f, in_f)
        scale = 1 / math.sqrt(had_dim)
    apply_exact_had_to_linear(l, had_dim=had_dim, output=output)
    assert l.weight.dtype == dtype and l.weight.device.type == device and tuple(l.weight.shape) == (out_f, in_f)
    assert torch.equal(l.weight.data.cpu(), O.exact_scaled(e, scale, torch.float32).to(dtype))


def _rotater_case(n, K, heads):
    """integer input [2, 37, n] and M x of it along the row (heads None) or across the heads"""
    xi = HC.ints((2, 37, n), n + 5)
    if heads is None:
        return xi, O.apply_M(xi, _hk(K)), 1.0 / O.fl32_sqrt(n)
    e = O.apply_M(xi.reshape(-1, heads, HC.HAD_DIM), _hk(K), axis=1).reshape(xi.shape)
    return xi, e, 1 / math.sqrt(heads)


@pytest.mark.parametrize('n,K,heads', [(n, K, None) for n, K in HC.ROTATER_FULL] + [(h * HC.HAD_DIM, K, h) for h, K in HC.ROTATER_HEADS])
def test_rotater_bit_for_bit_and_independent_of_fp32_had(n, K, heads):
    from llmc_amd.compression.quantization.hadamard_utils import get_hadK
    from llmc_amd.compression.quantization.module_utils import Rotater
    xi, e, scale = _rotater_case(n, K, heads)
    had_K, k = get_hadK(n if heads is None else heads)
    assert k == K
    for dtype in (torch.bfloat16, torch.float16):
        x0 = torch.from_numpy(xi).to(dtype)
        want = O.exact_scaled(e, scale, torch.float32).to(dtype)
        assert torch.equal(want, O.exact_scaled(e, scale, dtype))          # rounding fp32 -> dtype once, either way
        got = {}
        for fp32_had in (True, False):
            x = x0.cuda()
            r = Rotater(heads is None, heads is not None, fp32_had, K, had_K, None if heads is None else HC.HAD_DIM)
            got[fp32_had] = r.rotate(x)
            assert got[fp32_had].dtype == dtype and got[fp32_had].shape == x.shape
            assert torch.equal(got[fp32_had].cpu(), want), (dtype, fp32_had)
            assert torch.equal(x.cpu(), x0), 'the input was modified'
        assert torch.equal(got[True], got[False])
