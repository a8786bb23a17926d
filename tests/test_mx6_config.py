"""The OCP MXFP6 path at configuration time (no GPU): the 'mxfp6_quant' deploy key and its module, what
MxFp6RealQuantLinear.check_config takes and refuses, the argument checks of the entry points (pure host calls), and the exact-data
recipe of tests/test_mx6_gemm_gpu.py against its own exactness condition."""
import numpy as np
import pytest
import torch

import test_mx6_gemm_gpu as G

WEIGHT = G.WEIGHT


def _never(module):
    raise AssertionError('the quantizer must not run for a refused configuration')


def test_module_is_registered_and_takes_the_mxfp6_forms():
    from llmc_amd.compression.quantization.module_utils import (_LLMC_LINEAR_TYPES_, _REALQUANT_LINEAR_MAP_,
                                                                MxFp6RealQuantLinear)
    assert _REALQUANT_LINEAR_MAP_['mxfp6_quant'] is MxFp6RealQuantLinear
    assert MxFp6RealQuantLinear in _LLMC_LINEAR_TYPES_
    assert MxFp6RealQuantLinear.check_config({'weight': dict(WEIGHT)}) is None                      # weight-only
    assert MxFp6RealQuantLinear.check_config({'weight': dict(WEIGHT), 'act': dict(bit='e3m2', granularity='per_group')}) == 'e3m2'


@pytest.mark.parametrize('key,value', [('bit', 'e2m1'), ('bit', 6), ('granularity', 'per_channel'), ('group_size', 128),
                                       ('float_semantics', 'qtorch'), ('scale_format', 'dtype')])
def test_new_refuses_another_weight_form(key, value):
    from llmc_amd.compression.quantization.module_utils import MxFp6RealQuantLinear
    w = dict(WEIGHT)
    w[key] = value
    with pytest.raises(ValueError, match=key):
        MxFp6RealQuantLinear.new(torch.nn.Linear(128, 16), _never, {'weight': w})
    w.pop(key)
    with pytest.raises(ValueError, match=key):
        MxFp6RealQuantLinear.new(torch.nn.Linear(128, 16), _never, {'weight': w})


@pytest.mark.parametrize('act,reason', [(dict(bit='e2m1', granularity='per_group'), 'e2m1'),
                                        (dict(bit='e4m3', granularity='per_token'), 'e4m3'),
                                        (dict(bit='e5m2', granularity='per_token'), 'e5m2'),
                                        (dict(bit='e3m2', granularity='per_tensor', static=True), 'static')])
def test_new_refuses_another_activation_quantizer(act, reason):
    from llmc_amd.compression.quantization.module_utils import MxFp6RealQuantLinear
    with pytest.raises(ValueError, match=reason):
        MxFp6RealQuantLinear.new(torch.nn.Linear(128, 16), _never, {'weight': dict(WEIGHT), 'act': act})


def test_entry_points_refuse_what_they_do_not_take():
    from llmc_amd import _ffi
    L = _ffi.lib()
    p = 1 << 12        # an aligned non-null stand-in pointer; the calls return before touching it
    ok_gemm = dict(A=p, a_s=p, B6=p, b_s=p, M=4, N=4, K=128, out_dt=1, bias=None, C=p, rung=-1, stream=None)

    def gemm(**kw):
        return L.llmc_mx6_gemm_on_rung(*{**ok_gemm, **kw}.values())

    assert all(gemm(**{name: None}) == -22 for name in ('A', 'a_s', 'B6', 'b_s', 'C'))
    assert L.llmc_mx6_gemm(None, p, p, p, 4, 4, 128, 1, None, p, None) == -22
    assert gemm(A=p + 8) == -22 and 'align' in _ffi.last_error()
    assert gemm(a_s=p + 1) == -22 and gemm(out_dt=7) == -22 and gemm(M=0) == -22
    assert gemm(rung=2) == -22 and gemm(rung=0, M=17) == -22 and 'decode' in _ffi.last_error()
    assert all(gemm(K=K) == -95 and '128' in _ffi.last_error() for K in (64, 96, 130)) and gemm(K=1 << 24) == -95
    assert [L.llmc_mx6_gemm_rung(M, 4096, 4096) for M in (1, 16, 17, 4096)] == [0, 0, 1, 1]

    ok_q = dict(X=p, dt=1, M=4, K=128, codes=p, scales=p, stream=None)

    def quant(**kw):
        return L.llmc_mx6_act_quant(*{**ok_q, **kw}.values())

    assert all(quant(**{name: None}) == -22 for name in ('X', 'codes', 'scales'))
    assert quant(X=p + 2) == -22 and quant(dt=2) == -22                  # fp32 activations are not taken
    assert quant(K=48) == -95 and '32' in _ffi.last_error()
    assert L.llmc_mx6_pack(None, 4, 128, p, None) == -22 and L.llmc_mx6_pack(p + 4, 4, 128, p, None) == -22
    assert L.llmc_mx6_pack(p, 4, 48, p, None) == -95 and '32' in _ffi.last_error()


def test_exact_recipe_satisfies_its_exactness_condition():
    for (M, N, K), _ in G.EXACT:
        a, a_s, b, b_s = G.exact_operands(M, N, K, seed=M + N)
        ok, ratio = G.exact_in_any_order(a, a_s, b, b_s)
        assert ok, ((M, N, K), ratio)
        C, _ = G.gemm64(a, a_s, b, b_s)
        assert np.array_equal(C.astype(np.float32).astype(np.float64), C)                            # the result is an fp32 number
        assert ((a >> 4) & 1).any() and not ((a >> 4) & 1).all()                                      # both exponent classes of the kernel
    # and the condition does refuse what is not exact: full-range codes under a wide scale spread
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 64, (8, 1024)).astype(np.uint8), rng.integers(0, 64, (24, 1024)).astype(np.uint8)
    a_s, b_s = rng.integers(119, 136, (8, 32)).astype(np.uint8), rng.integers(119, 136, (24, 32)).astype(np.uint8)
    assert not G.exact_in_any_order(a, a_s, b, b_s)[0]
