"""llmc_test_gemm_route for the tests: which kernel a product of the internal GEMMs would launch, and how (a pure host call)."""
from types import SimpleNamespace

import numpy as np

from llmc_amd import _ffi

KERNELS = ('GK_SGEMM', 'GK_SHORTK', 'GK_SHORTK_PHASED', 'GK_WIDE2', 'GK_WIDE4', 'GK_GEMM3', 'GK_GEMM3S', 'GK_GEMM3S_PRE', 'GK_GEMM3W')
(GK_SGEMM, GK_SHORTK, GK_SHORTK_PHASED, GK_WIDE2, GK_WIDE4, GK_GEMM3, GK_GEMM3S, GK_GEMM3S_PRE, GK_GEMM3W) = range(9)
FIELDS = ('status', 'kernel', 'gx', 'gy', 'gz', 'threads', 'lds', 'ta', 'tb', 'phased', 'edge', 'phase_len', 'planes_dma', 'sm_log', 'sn_log',
          'sbm', 'nsb', 'wide_form')
SG_SUB, SG_SET, SG_NEG = 0, 1, 2
EINVAL, ENOTSUP = -22, -95


def up(x, m):
    return (x + m - 1) // m * m


def route(family, M, N, Kd, TA=False, TB=False, epilogue=SG_SUB, hints=(0, 0, 0, 0), phase_len=0, lda=None, ldb=None, ldc=None, batch=1,
          last=None, strides=None, planes=False, ldp=None, plane_stride=None, alias=None, mis=(0, 0, 0, 0)):
    """family 'sgemm' / 'gemm3'; hints = (a_upper, a_lower, b_upper, c_upper_only); leading dimensions default to the operand's width
    rounded up to 4, the planes' to llmc_test_gemm3_planes' layout; alias None / 'B' / 'A' (C is that operand); mis: bytes added to the
    256-B aligned addresses of A, B, C and the planes. Returns the hook's fields, `empty`, and the kernel's name."""
    lda = up(M if TA else Kd, 4) if lda is None else lda
    ldb = up(Kd if TB else N, 4) if ldb is None else ldb
    ldc = up(N, 4) if ldc is None else ldc
    Ml, Nl, Kl = last or (M, N, Kd)
    sA, sB, sC = strides or (lda * max(M, Kd), ldb * max(N, Kd), ldc * M)
    ldp = up(max(M, N), 8) if ldp is None else ldp
    ps = Kd * ldp if plane_stride is None else plane_stride
    inp = np.array([{'sgemm': 0, 'gemm3': 1}[family], M, N, Kd, lda, ldb, ldc, int(TA), int(TB), epilogue, *hints, phase_len, batch, Ml, Nl, Kl,
                    sA, sB, sC, int(planes), ldp, ps, {None: 0, 'B': 1, 'A': 2}[alias], *mis], dtype=np.int64)
    out = np.zeros(len(FIELDS), dtype=np.int32)
    rc = _ffi.lib().llmc_test_gemm_route(inp.ctypes.data, out.ctypes.data)
    assert rc in (0, 1), rc
    r = SimpleNamespace(**{k: int(v) for k, v in zip(FIELDS, out)}, empty=rc == 1)
    r.name = KERNELS[r.kernel] if r.status == 0 and not r.empty else None
    return r


def route_of(family, A, B, C, M, N, Kd, **kw):
    """The route of a product of device tensors as the launching hooks pass them: row strides as leading dimensions, the addresses'
    offsets from 256 B as misalignments."""
    return route(family, M, N, Kd, lda=A.stride(0), ldb=B.stride(0), ldc=C.stride(0),
                 mis=(A.data_ptr() % 256, B.data_ptr() % 256, C.data_ptr() % 256, 0), **kw)
