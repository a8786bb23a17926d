"""Every route of the internal GEMMs on the smallest shape that reaches it: the route hook is asked first (the test knows which
kernel it is about to run), then the kernel's bits are compared — the fp32 family against the oracle's fma chain (phase by phase
for the phased forms), the split-bf16 family against k_gemm3 (option gemm3_nospec)."""
import functools

import numpy as np
import pytest
import torch

from gemm_routes import SG_SET, SG_SUB, route_of, up
from llmc_amd import _ffi
from oracle import gptq_ref as G

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def problem(M, N, Kd, phase=0):
    """a [M x Kd], b [Kd x N], c0 [M x N] and the chain's product: phase by phase, what `C -= a b` leaves and, one phase, a b itself"""
    gen = torch.Generator().manual_seed(M * 3 + N * 5 + Kd)
    a, b, c0 = torch.randn(M, Kd, generator=gen) * 0.01, torch.randn(Kd, N, generator=gen), torch.randn(M, N, generator=gen)
    sub = c0.numpy().copy()
    for p in range(0, Kd, phase or Kd):
        sub = sub - G.mm_chain(np.ascontiguousarray(a[:, p:p + (phase or Kd)].numpy()), np.ascontiguousarray(b[p:p + (phase or Kd)].numpy()))
    prod = G.mm_chain(a.numpy(), b.numpy()) if not phase else None
    return a, b, c0, sub, prod


def padded(t):      # on the device with a leading dimension that is a multiple of 4
    out = torch.zeros(t.shape[0], up(t.shape[1], 4))
    out[:, :t.shape[1]] = t
    return out.cuda()[:, :t.shape[1]]


def run(kernel, a, b, c, TA=False, TB=False, epilogue=SG_SUB, phase=0, **opts):
    """op(A) = a, op(B) = b; asserts the route, launches, returns C"""
    M, Kd = a.shape
    N = b.shape[1]
    A, B = padded(a.t() if TA else a), padded(b.t() if TB else b)
    C = B if c is None else padded(c)      # None: in place
    L = _ffi.lib()
    with _ffi.option(**opts):
        r = route_of('sgemm', A, B, C, M, N, Kd, TA=TA, TB=TB, epilogue=epilogue, phase_len=phase, alias='B' if c is None else None)
        assert r.name == kernel, (r, opts)
        if phase:
            _ffi.check(L.llmc_test_sgemm_phased(A.data_ptr(), B.data_ptr(), C.data_ptr(), A.stride(0), B.stride(0), C.stride(0), M, N, Kd, int(TA),
                                                phase, _ffi.stream()), 'sgemm_phased')
        else:
            _ffi.check(L.llmc_test_sgemm(A.data_ptr(), B.data_ptr(), C.data_ptr(), A.stride(0), B.stride(0), C.stride(0), M, N, Kd, int(TA), int(TB),
                                         epilogue, 0, 0, 0, 0, _ffi.stream()), 'sgemm')
    return C, r


@pytest.mark.parametrize('shape', [(64, 64, 128), (130, 70, 127)])
@pytest.mark.parametrize('TA', [False, True])
def test_shortk(shape, TA):
    a, b, c0, sub, prod = problem(*shape)
    C, r = run('GK_SHORTK', a, b, c0, TA=TA)
    np.testing.assert_array_equal(bits(C), bits(sub))
    C, r = run('GK_SHORTK', a, b, c0, TA=TA, epilogue=SG_SET)
    np.testing.assert_array_equal(bits(C), bits(prod))


def test_shortk_in_place():
    """C = A^T B written over B (K3's panel solve): one workgroup per column tile walks the row tiles"""
    a, b, c0, sub, prod = problem(128, 192, 128)
    out, _ = run('GK_SHORTK', a, b, c0, TA=True, epilogue=SG_SET)
    C, r = run('GK_SHORTK', a, b, None, TA=True, epilogue=SG_SET)
    assert (r.gx, r.gy) == (3, 1)
    np.testing.assert_array_equal(bits(C), bits(out))
    np.testing.assert_array_equal(bits(C), bits(prod))


@pytest.mark.parametrize('TA', [False, True])
def test_shortk_phased(TA):
    a, b, c0, sub, _ = problem(128, 192, 256, 128)
    C, r = run('GK_SHORTK_PHASED', a, b, c0, TA=TA, phase=128)
    np.testing.assert_array_equal(bits(C), bits(sub))


@pytest.mark.parametrize('form', [2, 4])
def test_wide(form):
    a, b, c0, sub, _ = problem(256, 128, 128, 128)
    C, r = run('GK_WIDE%d' % form, a, b, c0, TA=True, phase=128, no_shortk=1, sgemm_no_wide=form)
    np.testing.assert_array_equal(bits(C), bits(sub))


def test_k_sgemm_instantiations():
    a, b, c0, sub, prod = problem(128, 128, 144)
    for TA in (False, True):
        C, r = run('GK_SGEMM', a, b, c0, TA=TA)                       # plain C -= AB: phased by rewrite, interior-only
        assert r.phased and r.phase_len == 1 << 30 and not r.edge
        np.testing.assert_array_equal(bits(C), bits(sub))
        C, r = run('GK_SGEMM', a, b, c0, TA=TA, TB=True, epilogue=SG_SET)      # op(B) = T
        assert not r.phased and r.tb
        np.testing.assert_array_equal(bits(C), bits(prod))
    a, b, c0, sub, _ = problem(130, 70, 200)
    C, r = run('GK_SGEMM', a, b, c0)
    assert r.edge and r.phased
    np.testing.assert_array_equal(bits(C), bits(sub))
    a, b, c0, sub, _ = problem(128, 128, 256, 128)
    C, r = run('GK_SGEMM', a, b, c0, TA=True, phase=128, no_shortk=1, sgemm_no_wide=1)      # explicit phases
    assert r.phased and r.phase_len == 128
    np.testing.assert_array_equal(bits(C), bits(sub))


def gemm3(kernel, A, B, C0, M, N, Kd, TA, planes=False, **opts):
    L = _ffi.lib()
    C = C0.clone()
    with _ffi.option(**opts):
        assert route_of('gemm3', A, B, C, M, N, Kd, TA=TA, planes=planes).name == kernel
        if planes:
            ws = torch.full((6 * Kd * up(max(M, N), 8),), -1, dtype=torch.int16).cuda()
            _ffi.check(L.llmc_test_gemm3_planes(A.data_ptr(), B.data_ptr(), C.data_ptr(), A.stride(0), B.stride(0), C.stride(0), M, N, Kd, 0, 0,
                                                ws.data_ptr(), _ffi.stream()), 'gemm3 planes')
        else:
            _ffi.check(L.llmc_test_gemm3(A.data_ptr(), B.data_ptr(), C.data_ptr(), A.stride(0), B.stride(0), C.stride(0), M, N, Kd, int(TA), 0, 0, 0, 0,
                                         _ffi.stream()), 'gemm3')
    return C


def operands(M, N, Kd):
    gen = torch.Generator().manual_seed(M + 7 * N + Kd)
    At = torch.randn(Kd, M, generator=gen) * torch.exp(torch.randn(Kd, 1, generator=gen))
    return At, torch.randn(Kd, N, generator=gen).cuda(), torch.randn(M, N, generator=gen).cuda()


@pytest.mark.parametrize('TA', [True, False])
def test_gemm3(TA):
    """k_gemm3 is the family's reference: here it is held to fp32-level accuracy — its error against fp64, relative to max |A|^T |B|,
    within twice the exact fp32 chain's (the bound of test_gemm3_split_bf16_matches_fp32_accuracy)"""
    M, N, Kd = 128, 128, 32
    At, B, C0 = operands(M, N, Kd)
    A = At.cuda() if TA else At.t().contiguous().cuda()
    C3 = gemm3('GK_GEMM3', A, B, C0, M, N, Kd, TA)
    assert torch.equal(C3, gemm3('GK_GEMM3', A, B, C0, M, N, Kd, TA, gemm3_nospec=1))      # the option moves no route here: the same kernel, asserted inside
    C1 = C0.clone()
    _ffi.check(_ffi.lib().llmc_test_sgemm(A.data_ptr(), B.data_ptr(), C1.data_ptr(), A.stride(0), B.stride(0), C1.stride(0), M, N, Kd, int(TA), 0, 0,
                                          0, 0, 0, 0, _ffi.stream()), 'sgemm')
    ref = C0.double() - At.double().t().cuda() @ B.double()
    scale = (At.double().abs().t().cuda() @ B.double().abs()).max()
    e3, e1 = ((C3.double() - ref).abs().max() / scale).item(), ((C1.double() - ref).abs().max() / scale).item()
    assert e3 <= max(2 * e1, 2e-7), (e3, e1)


def test_gemm3s_and_its_planes_form():
    M, N, Kd = 256, 128, 128
    At, B, C0 = operands(M, N, Kd)
    A = At.cuda()
    ref = gemm3('GK_GEMM3', A, B, C0, M, N, Kd, True, gemm3_nospec=1)
    assert not torch.equal(ref, C0)
    assert torch.equal(gemm3('GK_GEMM3S', A, B, C0, M, N, Kd, True, gemm3s_min_tiles=1), ref)
    assert torch.equal(gemm3('GK_GEMM3S_PRE', A, B, C0, M, N, Kd, True, planes=True, gemm3s_min_tiles=1, gemm3_no_wide=1), ref)


def test_gemm3w():
    M, N, Kd = 128, 128, 128
    At, B, C0 = operands(M, N, Kd)
    A = At.cuda()
    ref = gemm3('GK_GEMM3', A, B, C0, M, N, Kd, True, gemm3_nospec=1)
    assert not torch.equal(ref, C0)
    assert torch.equal(gemm3('GK_GEMM3W', A, B, C0, M, N, Kd, True, planes=True, gemm3s_min_tiles=1), ref)
