"""llmc_hadamard on the GPU against tests/hadamard_oracle.py.

Exactness: integer inputs in [-8, 8] and scale 1 make every partial sum an integer below 2^24, so whatever order the kernel adds
in, the result must equal numpy's int64 M_n x bit for bit (F32 / F64), or its single rounding (F16 / BF16). The shapes cover every
regime of the kernel: inside a wave (2, 64, 128), tiles stored from registers (512), the LDS exchange (1024, 4096, 32768 = the
longest resident fp32 row), factor matrices (384 = 12 * 32, 448 = 28 * 16, 14336 = 28 * 512, 28672 = 28 * 1024), rows sharing a
workgroup (outer 3, 67), the strided kernel (inner 64).

Scaled transforms on random data: |yhat_i - y_i| <= gamma_r ||x||_1 scale + u_dt |y_i| with r = log2(n / K0) + K0 + 1
(hadamard_oracle.bound) — derived from the number of roundings, not tuned."""
import numpy as np
import pytest
import torch

import hadamard_oracle as O

pytestmark = pytest.mark.gpu

NP_DT = {torch.float32: np.float32, torch.float64: np.float64}
U_DT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}


def _hadK(K):
    from llmc_amd.compression.quantization.hadamard_utils import get_hadK
    if K == 1:
        return None
    h, k = get_hadK(K)
    assert k == K
    return h


def _ints(shape, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=shape, dtype=np.int64)


# (outer, n, inner, K0)
ROW_CASES = [(1, 2, 1, 1), (67, 2, 1, 1), (3, 64, 1, 1), (67, 128, 1, 1), (3, 512, 1, 1), (3, 1024, 1, 1), (67, 4096, 1, 1),
             (3, 32768, 1, 1), (67, 384, 1, 12), (3, 448, 1, 28), (67, 448, 1, 28), (3, 14336, 1, 28), (3, 28672, 1, 28),
             (1, 12, 1, 12), (3, 24, 1, 12)]
COL_CASES = [(1, 4, 64, 1), (3, 32, 64, 1), (67, 256, 64, 1), (3, 4, 1000, 1), (3, 12, 64, 12), (3, 448, 24, 28)]


@pytest.mark.parametrize('outer,n,inner,K0', ROW_CASES + COL_CASES)
def test_integer_inputs_are_transformed_bit_for_bit(outer, n, inner, K0):
    from llmc_amd.compression.quantization.hadamard_utils import hadamard_transform
    hadK = _hadK(K0)
    xi = _ints((outer, n, inner), seed=n * 131 + outer)
    exact = O.apply_M(xi, None if hadK is None else hadK.numpy(), axis=1)
    assert np.abs(exact).max() < 2 ** 24
    for dt in (torch.float32, torch.float64, torch.float16, torch.bfloat16):
        if dt == torch.float64 and n * 8 + K0 * K0 * 4 > 160 * 1024:          # an fp64 row of this length is not resident
            continue
        x = torch.from_numpy(xi).to(dt).cuda()
        want = torch.from_numpy(exact).to(torch.float64).to(dt)          # integers below 2^24: one rounding
        y = hadamard_transform(x, n, inner, hadK, K0, 1.0)
        assert torch.equal(y.cpu(), want), (dt, 'out of place')
        assert torch.equal(x.cpu(), torch.from_numpy(xi).to(dt)), 'the input was modified'
        z = hadamard_transform(x, n, inner, hadK, K0, 1.0, out=x)            # in place
        assert z.data_ptr() == x.data_ptr() and torch.equal(x.cpu(), want), (dt, 'in place')


def test_unaligned_rows_take_the_scalar_path():
    """a view that starts 2 bytes off a 16-byte boundary: same values"""
    from llmc_amd.compression.quantization.hadamard_utils import hadamard_transform
    xi = _ints((5, 256), seed=7)
    buf = torch.zeros(5 * 256 + 1, dtype=torch.bfloat16, device='cuda')
    x = buf[1:].view(5, 256)
    x.copy_(torch.from_numpy(xi).to(torch.bfloat16))
    y = hadamard_transform(x, 256, 1, None, 1, 1.0)
    assert torch.equal(y.cpu(), torch.from_numpy(O.apply_M(xi)).to(torch.float64).to(torch.bfloat16))


def test_unsupported_calls_are_refused():
    from llmc_amd import _ffi
    L = _ffi.lib()
    x = torch.zeros(128 * 4, device='cuda')
    hk = torch.ones(128, 128, device='cuda')
    st = _ffi.stream()
    assert L.llmc_hadamard(x.data_ptr(), x.data_ptr(), _ffi.F32, 1, 512, 1, hk.data_ptr(), 128, 1.0, st) == -95
    assert 'K0 > 64' in _ffi.last_error()
    assert L.llmc_hadamard(x.data_ptr(), x.data_ptr(), _ffi.F32, 1, 36, 1, hk.data_ptr(), 12, 1.0, st) == -95
    assert 'power of two' in _ffi.last_error()
    assert L.llmc_hadamard(x.data_ptr(), x.data_ptr(), _ffi.F32, 1, 65536, 1, None, 1, 1.0, st) == -95
    assert 'resident' in _ffi.last_error()
    assert L.llmc_hadamard(x.data_ptr(), x.data_ptr(), _ffi.F64, 1, 32768, 1, None, 1, 1.0, st) == -95
    assert 'resident' in _ffi.last_error()
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0


@pytest.mark.parametrize('outer,n,inner,K0', [(3, 128, 1, 1), (5, 4096, 1, 1), (2, 32768, 1, 1), (5, 448, 1, 28), (2, 28672, 1, 28),
                                                (3, 32, 64, 1), (3, 12, 64, 12)])
def test_scaled_transform_within_the_derived_bound(outer, n, inner, K0):
    from llmc_amd.compression.quantization.hadamard_utils import hadamard_transform
    hadK = _hadK(K0)
    hk = None if hadK is None else hadK.numpy()
    g = torch.Generator().manual_seed(n + K0)
    x64 = torch.randn(outer, n, inner, generator=g, dtype=torch.float64) * torch.exp(torch.randn(outer, n, inner, generator=g,
                                                                                              dtype=torch.float64))
    for dt in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        if dt == torch.float64 and n * 8 > 160 * 1024:
            continue
        x = x64.to(dt)
        s64 = 1.0 / O.fl32_sqrt(n)
        scale = s64 if dt == torch.float64 else float(np.float32(s64))      # the fp32 path rounds the scale to fp32
        y = O.transform(x.double().numpy(), hk, axis=1, scale=scale)
        l1 = np.abs(x.double().numpy()).sum(axis=1, keepdims=True)
        u_acc = 2.0 ** -53 if dt == torch.float64 else 2.0 ** -24
        bnd = O.bound(l1, y, n, K0, scale, u_acc, U_DT[dt])
        got = hadamard_transform(x.cuda(), n, inner, hadK, K0, s64).cpu().double().numpy()
        err = np.abs(got - y)
        print(f'{dt} n={n} K0={K0} inner={inner}: max err / bound = {(err / bnd).max():.3f}')
        assert (err <= bnd).all(), (dt, float((err / bnd).max()))
