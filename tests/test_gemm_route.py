"""Which kernel runs an internal GEMM is data (sgemm_route / gemm3_route through llmc_test_gemm_route, a pure host call): the routes
of the products K3 and K4 launch, what every option moves, the refusals, and the launch geometry, checked without a device."""
import itertools

import pytest

from gemm_routes import (EINVAL, ENOTSUP, GK_GEMM3, GK_GEMM3S, GK_GEMM3S_PRE, GK_GEMM3W, GK_SGEMM, GK_SHORTK, GK_SHORTK_PHASED, GK_WIDE2,
                         GK_WIDE4, SG_NEG, SG_SET, SG_SUB, route)
from llmc_amd import _ffi

# K4's updates of a [4096 x 14336] weight: err columns k-major (lda = R), inverse factor and weight with ld = K
K4 = dict(TA=True, lda=4096, ldb=14336, ldc=14336)


def grid(r):
    return (r.gx, r.gy, r.gz)


def test_k4_products():
    far = route('sgemm', 4096, 13824, 512, phase_len=128, **K4)
    assert far.name == 'GK_WIDE2' and far.phased and far.phase_len == 128 and far.threads == 256 and far.lds == 73728
    few = route('sgemm', 4096, 512, 512, phase_len=128, **K4)            # 512 tiles of 64 x 64 <= 1024
    assert few.name == 'GK_SHORTK_PHASED' and grid(few) == (8, 64, 1) and few.wide_form == 2
    assert route('sgemm', 4096, 1152, 512, phase_len=128, **K4).name == 'GK_WIDE2'      # 18 x 64 = 1152 tiles
    near = route('sgemm', 4096, 384, 128, **K4)
    assert near.name == 'GK_SHORTK' and grid(near) == (6, 64, 1) and near.threads == 256 and near.lds == 0 and not near.phased
    assert grid(route('sgemm', 4096, 384, 128, alias='B', **K4)) == (6, 1, 1)      # in place: one workgroup walks the row tiles
    assert route('sgemm', 4096, 384, 128, phase_len=128, **K4).name == 'GK_SHORTK'      # a phase that covers all of K is no phase


def test_k_sgemm_instantiations():
    r = route('sgemm', 128, 128, 144)
    assert r.name == 'GK_SGEMM' and r.phased and r.phase_len == 1 << 30 and not r.edge and grid(r) == (1, 1, 1)      # plain C -= AB: one phase over all of K
    assert route('sgemm', 130, 128, 144).edge and route('sgemm', 128, 124, 144).edge and route('sgemm', 128, 128, 152).edge
    assert route('sgemm', 128, 128, 144, batch=2, last=(128, 64, 144)).edge
    for ep in (SG_SET, SG_NEG):
        r = route('sgemm', 128, 128, 144, epilogue=ep)
        assert r.name == 'GK_SGEMM' and not r.phased and r.phase_len == 0
    for TA in (False, True):
        r = route('sgemm', 128, 128, 144, TA=TA, TB=True)
        assert r.name == 'GK_SGEMM' and not r.phased and r.tb and r.ta == TA
        assert route('sgemm', 128, 128, 128, TA=TA, TB=True).name == 'GK_SGEMM'          # no short-K kernel for op(B) = T
    for ep in (SG_SUB, SG_SET):
        r = route('sgemm', 128, 128, 128, epilogue=ep, hints=(1, 0, 0, 0))      # a_upper: neither short-K nor phased
        assert r.name == 'GK_SGEMM' and not r.phased
    assert route('sgemm', 128, 128, 128, hints=(0, 0, 1, 0)).name == 'GK_SGEMM' and route('sgemm', 128, 128, 128, hints=(0, 1, 0, 0)).name == 'GK_SHORTK'
    assert route('sgemm', 128, 128, 128, batch=2).name == 'GK_SGEMM'
    r = route('sgemm', 128, 128, 256, phase_len=128, hints=(0, 1, 0, 0))      # a_lower keeps a phased product off the short-K kernel and the wide one
    assert r.name == 'GK_SGEMM' and r.phased and r.phase_len == 128


def test_gemm3_products():
    r = route('gemm3', 4096, 4096, 512, TA=True)
    assert r.name == 'GK_GEMM3S' and grid(r) == (32, 16, 1) and r.threads == 512 and r.lds == 147456
    r = route('gemm3', 2048, 2048, 512, TA=True)                          # 128 tiles of 256 x 128, below 256
    assert r.name == 'GK_GEMM3' and grid(r) == (16, 16, 1) and r.threads == 256 and r.lds == 0
    assert route('gemm3', 2048, 2048, 512, TA=True, planes=True).name == 'GK_GEMM3S_PRE'      # >= 48 tiles, below 1024 tiles of 128 x 128
    r = route('gemm3', 4096, 4096, 512, TA=True, planes=True)
    assert r.name == 'GK_GEMM3W' and r.threads == 256 and r.lds == 73728
    assert route('gemm3', 4096, 4096, 512, TA=True, planes=True, hints=(0, 0, 0, 1)).name == 'GK_GEMM3S_PRE'      # 528 working tiles
    assert route('gemm3', 8192, 8192, 512, TA=True, planes=True, hints=(0, 0, 0, 1), ldp=8192).name == 'GK_GEMM3W'      # 2080
    for ep in (SG_SET, SG_NEG):
        assert route('gemm3', 4096, 4096, 512, TA=True, planes=True, epilogue=ep).name == 'GK_GEMM3S_PRE'
    for M, planes in itertools.product((128, 2048, 4096, 14336), (False, True)):
        assert route('gemm3', M, M, 512, TA=False, planes=planes).name == 'GK_GEMM3'
    for h in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0)):
        assert route('gemm3', 4096, 4096, 512, TA=True, hints=h).name == 'GK_GEMM3'
    assert route('gemm3', 4096, 4096, 96, TA=True).name == 'GK_GEMM3' and route('gemm3', 4096, 4096, 192, TA=True).name == 'GK_GEMM3S'
    assert route('gemm3', 4096, 4096, 512, TA=True, batch=3, planes=True).name == 'GK_GEMM3'      # the planes of ONE panel


def test_options_move_routes():
    with _ffi.option(no_shortk=1):
        assert route('sgemm', 4096, 384, 128, **K4).name == 'GK_SGEMM'
        assert route('sgemm', 4096, 512, 512, phase_len=128, **K4).name == 'GK_WIDE2'
    with _ffi.option(sgemm_no_wide=1):
        r = route('sgemm', 4096, 13824, 512, phase_len=128, **K4)
        assert r.name == 'GK_SGEMM' and r.phased and r.phase_len == 128 and r.wide_form == 0 and grid(r) == (108, 32, 1)
    with _ffi.option(sgemm_no_wide=4):
        assert route('sgemm', 4096, 13824, 512, phase_len=128, **K4).name == 'GK_WIDE4'
        r = route('sgemm', 384, 13824, 512, TA=True, phase_len=128)      # M % 256 != 0
        assert r.name == 'GK_WIDE2' and r.wide_form == 2
    with _ffi.option(sgemm_no_wide=2):
        assert route('sgemm', 4096, 13824, 512, phase_len=128, **K4).name == 'GK_WIDE2'
    with _ffi.option(gemm3_nospec=1):
        for planes in (False, True):
            assert route('gemm3', 4096, 4096, 512, TA=True, planes=planes).name == 'GK_GEMM3'
    with _ffi.option(gemm3_no_wide=1):
        assert route('gemm3', 4096, 4096, 512, TA=True, planes=True).name == 'GK_GEMM3S_PRE'
    with _ffi.option(gemm3s_min_tiles=1):
        assert route('gemm3', 256, 128, 128, TA=True).name == 'GK_GEMM3S'
        assert route('gemm3', 128, 128, 128, TA=True, planes=True).name == 'GK_GEMM3W'
        assert route('gemm3', 136, 128, 128, TA=True, planes=True).name == 'GK_GEMM3S_PRE'
    assert route('gemm3', 4096, 4096, 512, TA=True).planes_dma == 1
    with _ffi.option(gemm3s_no_dma=1):
        assert route('gemm3', 4096, 4096, 512, TA=True).planes_dma == 0
        assert route('gemm3', 2048, 2048, 512, TA=True, planes=True).planes_dma == 0


def test_refusals_and_empty_products():
    ok = dict(M=128, N=128, Kd=144)
    assert route('sgemm', **ok, mis=(4, 0, 0, 0)).status == EINVAL and route('sgemm', **ok, mis=(0, 8, 0, 0)).status == EINVAL
    assert route('sgemm', **ok, lda=146).status == EINVAL and route('sgemm', **ok, ldb=130).status == EINVAL
    assert route('sgemm', **ok, batch=2, strides=(4098, 4096, 4096)).status == EINVAL
    assert route('sgemm', **ok, mis=(0, 0, 4, 0), ldc=130).status == 0                      # k_sgemm takes any C
    assert route('sgemm', 128, 128, 256, TB=True, phase_len=128).status == ENOTSUP
    assert route('sgemm', 128, 128, 256, phase_len=128, epilogue=SG_SET).status == EINVAL and route('sgemm', 128, 128, 256, phase_len=24).status == EINVAL
    assert route('sgemm', 256, 256, 144, alias='B').status == EINVAL                      # in place off the short-K path: one row tile
    assert route('sgemm', 128, 256, 144, alias='B').name == 'GK_SGEMM' and route('sgemm', 256, 256, 128, alias='B').name == 'GK_SHORTK'
    g3 = dict(M=256, N=256, Kd=128, TA=True)
    assert route('gemm3', **g3).status == 0
    assert route('gemm3', **g3, phase_len=128).status == EINVAL
    assert route('gemm3', **g3, alias='B').status == EINVAL and route('gemm3', **g3, alias='A').status == EINVAL
    assert route('gemm3', 256, 254, 128, TA=True, ldb=256, ldc=256).status == EINVAL and route('gemm3', 254, 256, 128, TA=True, lda=256).status == EINVAL
    assert route('gemm3', 254, 256, 128, TA=False).status == 0                            # M % 4 matters for k-major A only
    assert route('gemm3', **g3, mis=(8, 0, 0, 0)).status == EINVAL
    for fam in ('sgemm', 'gemm3'):
        for dims in ((0, 128, 128), (128, 0, 128)):
            r = route(fam, *dims, lda=128, ldb=128, ldc=128)
            assert r.status == 0 and r.empty and r.name is None
        r = route(fam, 128, 128, 128, batch=0)
        assert r.status == 0 and r.empty
        assert route(fam, 0, 128, 128, lda=130, ldb=128, ldc=128).status == 0      # emptiness is looked at first


TILE = {GK_SGEMM: (128, 128), GK_SHORTK: (64, 64), GK_SHORTK_PHASED: (64, 64), GK_GEMM3: (128, 128), GK_GEMM3S: (256, 128), GK_GEMM3S_PRE: (256, 128)}
WIDE = {GK_WIDE2: (128, 6), GK_WIDE4: (256, 5), GK_GEMM3W: (128, 6)}      # tile rows, log2 of the tiles an XCD runs at a time


@pytest.mark.parametrize('opts', [{}, dict(no_shortk=1, sgemm_no_wide=4), dict(gemm3s_min_tiles=1), dict(gemm3s_min_tiles=1, gemm3_no_wide=1)])
def test_launch_geometry(opts):
    """Grids cover the tiles; the wide kernels' tile blocks are consistent and their 1-D grid is whole rounds of 8 blocks."""
    seen = set()
    sizes = (4, 60, 64, 128, 130, 256, 1024, 4096)
    with _ffi.option(**opts):
        for fam, M, N, Kd, TA, ep, ph in itertools.product(('sgemm', 'gemm3'), sizes, sizes, (16, 127, 128, 144, 256, 512), (False, True),
                                                          (SG_SUB, SG_SET), (0, 128)):
            for planes, upper, batch in ((False, 0, 1), (True, 1, 1), (False, 0, 3)) if fam == 'gemm3' and ph == 0 else ((False, 0, 1), (False, 0, 3)):
                r = route(fam, M, N, Kd, TA=TA, epilogue=ep, phase_len=ph, planes=planes, hints=(0, 0, 0, upper), batch=batch)
                if r.status:
                    continue
                seen.add(r.kernel)
                assert r.threads == (512 if r.kernel in (GK_GEMM3S, GK_GEMM3S_PRE) else 256)
                if r.kernel in TILE:
                    bm, bn = TILE[r.kernel]
                    assert grid(r) == (-(-N // bn), -(-M // bm), batch), (fam, M, N, Kd, r)
                else:
                    bm, logt = WIDE[r.kernel]
                    tm, tn = M // bm, N // 128
                    assert M % bm == 0 and N % 128 == 0 and batch == 1
                    assert r.sm_log >= 1 and r.sn_log >= 1 and r.sm_log + r.sn_log == logt
                    assert r.sbm == -(-tm >> r.sm_log) and r.nsb == r.sbm * -(-tn >> r.sn_log)
                    assert grid(r) == (-(-r.nsb // 8) * 8 << logt, 1, 1)
                    assert r.lds == (110592 if r.kernel == GK_WIDE4 else 73728)
    assert seen >= ({GK_SGEMM, GK_GEMM3} | ({GK_WIDE4, GK_WIDE2} if 'no_shortk' in opts else {GK_SHORTK, GK_SHORTK_PHASED}))
    if 'gemm3s_min_tiles' in opts:
        assert seen >= {GK_GEMM3S, GK_GEMM3S_PRE} | (set() if 'gemm3_no_wide' in opts else {GK_GEMM3W})
