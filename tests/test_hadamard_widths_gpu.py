"""llmc_hadamard at the widths a real model produces, bit for bit against tests/hadamard_oracle.py.

tests/test_hadamard_kernel_gpu.py runs the sizes of the toy model; launch_had picks its path from n, K0, inner and the accumulator
size, and these cases (tests/hadamard_cases.py, shared with the CPU test of their precondition) run the paths it leaves out. Every
input is an integer in [-8, 8], so every partial sum is an integer below 2^19 and exact in fp32 and fp64 in any order: with
scale 1 the result is numpy's int64 M_n x, with scale 1 / fl32(sqrt(n)) it is hadamard_oracle.exact_scaled (one multiplication by
the scale cast to the accumulator type, one rounding to the tensor dtype). No tolerance anywhere. The factor matrix is passed
explicitly, so a size that get_hadK maps to another order (5120 = 40 * 128) is still a valid order-20 input here.

(outer, n, inner, K0) and what it reaches; L = log2(n / K0), rpb = rows per workgroup, C = columns per workgroup (fp32 / fp64):

k_had_rows, K0 = 1
  (3, 4, 1, 1)        L = 2: a partial register butterfly, runs shorter than 8
  (5, 8, 1, 1)        L = 3: the register butterfly alone
  (5, 16, 1, 1)       L = 4: the DPP xor-1 stage is the last stage of a row
  (5, 32, 1, 1)       L = 5: DPP xor-2 last
  (70, 256, 1, 1)     L = 8: ds_swizzle xor-16 last; rpb 32 / 16, the last workgroup holds 6 rows
  (9, 2048, 1, 1)     L - 9 = 2 (rows_high_bits<2>); rpb 4 / 2 with a tail workgroup of one row
  (3, 8192, 1, 1)     L - 9 = 4 (rows_high_bits<4>)
  (2, 16384, 1, 1)    L - 9 = 5 (rows_high_bits<5>); 128 KiB of LDS in fp64
k_had_rows with a factor
  (2, 20, 1, 20) (3, 40, 1, 20) (3, 80, 1, 20)      L = 0, 1, 2 with order 20: the per-element mix; runs of 8 cross segment
                      boundaries and, for n = 20, rows
  (3, 160, 1, 20)     L = 3: the shortest row on the vector mix
  (5, 3072, 1, 12)    rpb 2 (fp32), the last workgroup holds 1 row
  (5, 5120, 1, 20)    10 waves       (5, 4608, 1, 36)    9 waves       (5, 7680, 1, 60)    15 waves
  (3, 15360, 1, 60)   137 280 B of LDS in fp64
  (2, 36864, 1, 36)   152 640 B in fp32, L - 9 = 1: the longest row with a factor that fits; F64 is refused (-95, "resident")
k_had_cols
  (2, 4096, 40, 1)    C = 2 / 1; four passes, the first with s0 >= 9
  (2, 8192, 9, 1)     C = 1, odd inner (2-byte accesses at odd element offsets); five passes ending in a radix-2 pass; 64 KiB in fp64
  (1, 16384, 3, 1)    C = 1; five passes ending in a radix-4 pass; 128 KiB in fp64
  (3, 512, 24, 1)     the s0 = 6 pass has three bits; C = 16 / 8 with a chunk of 8 left over
  (3, 1024, 130, 1)   C = 8 / 4 with 2 columns left over
  (2, 2048, 200, 1)   C = 4 / 2
  (2, 3584, 5, 28)    C = 2 with one column left over / C = 1
  (2, 4608, 5, 36) (2, 7680, 3, 60) (1, 14336, 3, 28)      C = 1 with the mix; 75 840 B and 117 824 B in fp64
  (3, 60, 7, 60)      L = 0: no pass at all; C = 8 with 7 valid columns
  (37, heads, 128, K0)    heads in the middle, [tokens, heads, 128]: 32 and 64 heads (K0 = 1), 28, 24 = 12 * 2, 20, 36, 12 heads
unaligned views (the view starts one element off a 16-byte boundary inside a buffer of guard elements, which stay as they were)
  F32 and F64 (3, 1024): scalar loads and stores around the LDS exchange; BF16 (5, 384) order 12: around the mix;
  F16 (3, 8192): around rows_high_bits<4>; each with an unaligned out=, in place, aligned -> unaligned and unaligned -> aligned
random data: five of the shapes above within hadamard_oracle.bound (derived from the number of roundings, not tuned)."""
import numpy as np
import pytest
import torch

import hadamard_cases as HC
import hadamard_oracle as O

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.float64, torch.float16, torch.bfloat16)
U_DT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
LDS_MAX = 160 * 1024


def _hadK(K):
    from llmc_amd.compression.quantization.hadamard_utils import get_hadK
    if K == 1:
        return None
    h, k = get_hadK(K)
    assert k == K
    return h


def _wants(e, n, dt):
    """(scale, expected tensor) for scale 1 and scale 1 / fl32(sqrt(n))"""
    s = 1.0 / O.fl32_sqrt(n)
    return ((1.0, torch.from_numpy(e).to(torch.float64).to(dt)), (s, O.exact_scaled(e, s, dt)))


@pytest.mark.parametrize('outer,n,inner,K0', HC.KERNEL_CASES)
def test_model_widths_are_transformed_bit_for_bit(outer, n, inner, K0):
    from llmc_amd import _ffi
    from llmc_amd.compression.quantization.hadamard_utils import hadamard_transform
    hadK = _hadK(K0)
    xi = HC.ints((outer, n, inner), HC.seed(outer, n, inner))
    e = O.apply_M(xi, None if hadK is None else hadK.numpy(), axis=1)
    for dt in DTYPES:
        x0 = torch.from_numpy(xi).to(dt)
        if dt == torch.float64 and n * 8 + K0 * K0 * 4 > LDS_MAX:          # an fp64 row of this length is not resident: refused
            x, y, hk = x0.cuda(), torch.zeros(outer, n, inner, dtype=dt, device='cuda'), hadK.cuda().contiguous()
            rc = _ffi.lib().llmc_hadamard(x.data_ptr(), y.data_ptr(), _ffi.F64, outer, n, inner, hk.data_ptr(), K0, 1.0,
                                          _ffi.stream())
            assert rc == -95 and 'resident' in _ffi.last_error()
            torch.cuda.synchronize()
            assert torch.equal(x.cpu(), x0) and float(y.abs().sum()) == 0.0
            continue
        for scale, want in _wants(e, n, dt):
            x = x0.cuda()
            y = hadamard_transform(x, n, inner, hadK, K0, scale)
            assert y.dtype == dt and torch.equal(y.cpu(), want), (dt, scale, 'out of place')
            assert torch.equal(x.cpu(), x0), (dt, scale, 'the input was modified')
            z = hadamard_transform(x, n, inner, hadK, K0, scale, out=x)
            assert z.data_ptr() == x.data_ptr() and torch.equal(x.cpu(), want), (dt, scale, 'in place')


GUARD = 77.0


def _view(rows, n, dt, aligned, fill=None):
    """a [rows, n] view in the middle of a buffer of guard elements: `pad` of them in front, one behind. 8 elements are a multiple
    of 16 bytes in every dtype, 9 are not: the unaligned view starts one element off a 16-byte boundary"""
    pad = 8 if aligned else 9
    buf = torch.full((pad + rows * n + 1,), GUARD, dtype=dt, device='cuda')
    v = buf[pad:pad + rows * n].view(rows, n)
    assert v.is_contiguous() and buf.data_ptr() % 16 == 0 and (v.data_ptr() % 16 == 0) == aligned
    if fill is not None:
        v.copy_(fill)
    return buf, v, pad


def _guards_intact(buf, pad):
    return bool((buf[:pad] == GUARD).all()) and float(buf[-1]) == GUARD


@pytest.mark.parametrize('dtname,rows,n,K0', HC.UNALIGNED)
@pytest.mark.parametrize('in_aligned,out_aligned,in_place', [(False, False, False), (False, False, True), (True, False, False),
                                                              (False, True, False)])
def test_unaligned_views_on_every_store_path(dtname, rows, n, K0, in_aligned, out_aligned, in_place):
    from llmc_amd.compression.quantization.hadamard_utils import hadamard_transform
    dt = getattr(torch, dtname)
    hadK = _hadK(K0)
    xi = HC.ints((rows, n, 1), HC.seed(rows, n, 1))
    e = O.apply_M(xi, None if hadK is None else hadK.numpy(), axis=1).reshape(rows, n)
    x0 = torch.from_numpy(xi.reshape(rows, n)).to(dt)
    for scale, want in _wants(e, n, dt):
        xbuf, x, xoff = _view(rows, n, dt, in_aligned, x0)
        if in_place:
            ybuf, y, yoff = xbuf, x, xoff
        else:
            ybuf, y, yoff = _view(rows, n, dt, out_aligned)
        got = hadamard_transform(x, n, 1, hadK, K0, scale, out=y)
        assert got.data_ptr() == y.data_ptr()
        assert torch.equal(y.cpu(), want), (scale, 'values')
        assert _guards_intact(ybuf, yoff), (scale, 'an element next to the output view was written')
        if not in_place:
            assert torch.equal(x.cpu(), x0), (scale, 'the input was modified')
            assert _guards_intact(xbuf, xoff), (scale, 'an element next to the input view was written')


@pytest.mark.parametrize('outer,n,inner,K0', HC.RANDOM_CASES)
def test_scaled_transform_of_random_data_within_the_derived_bound(outer, n, inner, K0):
    """test_hadamard_kernel_gpu.py::test_scaled_transform_within_the_derived_bound at model widths: same data, same bound"""
    from llmc_amd.compression.quantization.hadamard_utils import hadamard_transform
    hadK = _hadK(K0)
    hk = None if hadK is None else hadK.numpy()
    g = torch.Generator().manual_seed(n + K0)
    x64 = torch.randn(outer, n, inner, generator=g, dtype=torch.float64) * torch.exp(torch.randn(outer, n, inner, generator=g,
                                                                                              dtype=torch.float64))
    for dt in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
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
