"""The plain FP8 Linear at configuration time (no GPU): the library exports llmc_fp8_scaled_gemm and _ffi carries its signature,
the entry point's return codes (pure host checks: nothing is launched), the wrappers' shape and dtype checks, what
VllmRealQuantLinear.new records for forward, and the stored forms forward still refuses."""
import ctypes

import pytest
import torch

FP8 = torch.float8_e4m3fn
W_CH = dict(bit='e4m3', symmetric=True, granularity='per_channel', quant_type='float-quant', use_qtorch=True)
W_T = dict(W_CH, granularity='per_tensor')
A_TOK = dict(bit='e4m3', symmetric=True, granularity='per_token', quant_type='float-quant', use_qtorch=True)
A_STATIC = dict(bit='e4m3', symmetric=True, granularity='per_tensor', quant_type='float-quant', use_qtorch=True, static=True)


def test_library_exports_the_entry_and_ffi_carries_its_signature():
    from llmc_amd import _ffi
    L = _ffi.lib()
    assert hasattr(L, 'llmc_fp8_scaled_gemm') and hasattr(L, 'llmc_fp8_scaled_gemm_rung') and hasattr(L, 'llmc_fp8_scaled_gemm_on_rung')
    fn = L.llmc_fp8_scaled_gemm
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 13
    assert [fn.argtypes[i] for i in (2, 5, 6, 7, 8)] == [ctypes.c_int64] * 5 and fn.argtypes[9] is ctypes.c_int
    # the ladder: decode up to 64 tokens, a tile rung above
    assert L.llmc_fp8_scaled_gemm_rung(1, 4096) == 0 and L.llmc_fp8_scaled_gemm_rung(64, 4096) == 0
    assert L.llmc_fp8_scaled_gemm_rung(65, 4096) == 1 and L.llmc_fp8_scaled_gemm_rung(4096, 4096) == 1


def test_entry_point_return_codes():
    from llmc_amd import _ffi
    L = _ffi.lib()
    p = 1 << 12        # an aligned non-null stand-in pointer; the calls return before touching it
    bf16 = _ffi.dt(torch.bfloat16)
    ok = dict(A=p, a_s=p, a_s_n=4, B=p, b_s=p, b_s_n=8, M=4, N=8, K=192, out_dt=bf16, bias=None, C=p, stream=None)

    def gemm(**kw):
        return L.llmc_fp8_scaled_gemm(*{**ok, **kw}.values())

    assert gemm() == -95 and '128' in _ffi.last_error()                  # everything valid but the depth: LLMC_ENOTSUP
    for K in (64, 130, 1 << 24):
        assert gemm(K=K) == -95, K
    for name in ('A', 'a_s', 'B', 'b_s', 'C'):
        assert gemm(**{name: None}) == -22, name
    assert gemm(A=p + 8) == -22 and 'align' in _ffi.last_error()
    assert gemm(B=p + 4) == -22
    assert gemm(a_s=p + 2) == -22 and gemm(b_s=p + 1) == -22
    assert gemm(out_dt=7) == -22
    for n in (0, 2, 3, 5):
        assert gemm(a_s_n=n) == -22 and 'a_s' in _ffi.last_error(), n
    for n in (0, 2, 7, 9):
        assert gemm(b_s_n=n) == -22, n
    assert gemm(a_s_n=1) == -95 and gemm(b_s_n=1) == -95                 # per-tensor scales are in the allowed set
    assert gemm(M=0) == -22 and gemm(N=0) == -22
    assert gemm(out_dt=bf16 | (1 << 8)) == -22                           # stray high bits are another out_dt
    # a named rung (the entry of the measuring tool and the tests): the decode rung does not take more than 64 tokens, and there
    # are two rungs
    def on_rung(rung, **kw):
        v = list({**ok, **kw}.values())
        return L.llmc_fp8_scaled_gemm_on_rung(*v[:12], rung, None)

    assert on_rung(0, M=65, a_s_n=65) == -22 and on_rung(2) == -22 and on_rung(-2) == -22
    assert on_rung(-1) == -95 and on_rung(0) == -95 and on_rung(1) == -95


def test_wrappers_check_shapes_before_any_gpu_use():
    from llmc_amd.compression.quantization import fp8_linear_ops as F8
    a8, w8 = torch.zeros(3, 128, dtype=FP8), torch.zeros(16, 128, dtype=FP8)
    a_s, w_s = torch.ones(3, 1), torch.ones(16, 1)
    with pytest.raises(TypeError, match='a8'):
        F8.fp8_scaled_gemm(a8.float(), a_s, w8, w_s)
    with pytest.raises(TypeError, match='w8'):
        F8.fp8_scaled_gemm(a8, a_s, w8.view(torch.uint8).to(torch.int8), w_s)
    with pytest.raises(ValueError, match='disagree on K'):
        F8.fp8_scaled_gemm(a8, a_s, torch.zeros(16, 256, dtype=FP8), w_s)
    with pytest.raises(ValueError, match='a_s'):
        F8.fp8_scaled_gemm(a8, torch.ones(2), w8, w_s)
    with pytest.raises(ValueError, match='w_s'):
        F8.fp8_scaled_gemm(a8, a_s, w8, torch.ones(15))
    with pytest.raises(TypeError, match='a_s'):
        F8.fp8_scaled_gemm(a8, a_s.double(), w8, w_s)
    with pytest.raises(TypeError, match='output'):
        F8.fp8_scaled_gemm(a8, a_s, w8, w_s, dtype=torch.float64)
    with pytest.raises(ValueError, match='bias'):
        F8.fp8_scaled_gemm(a8, a_s, w8, w_s, bias=torch.zeros(3))
    with pytest.raises(ValueError, match=r'\[N, K\]'):
        F8.fp8_scaled_gemm(a8, a_s, w8[0], w_s)
    # everything in order: the first thing that needs the GPU refuses the CPU tensors
    with pytest.raises(Exception, match='MI355X only'):
        F8.fp8_scaled_gemm(a8, a_s, w8, w_s)


def test_act_mode_names_the_two_pairings_and_refuses_the_rest():
    from llmc_amd.compression.quantization.fp8_linear_ops import act_mode
    assert act_mode(None) is None
    assert act_mode(A_TOK) == 'dynamic_per_token' and act_mode(A_STATIC) == 'static_per_tensor'
    for bad, reason in ((dict(A_TOK, bit='e5m2'), 'e5m2'), (dict(A_TOK, bit=8, quant_type='int-quant'), 'int8'),
                        (dict(A_TOK, granularity='per_tensor'), 'dynamic per_tensor'), (dict(A_STATIC, granularity='per_token'), 'static per_token')):
        with pytest.raises(NotImplementedError, match=reason):
            act_mode(bad)


def _stub_w_q(granularity):
    def w_q(module):
        R, K = module.weight.shape
        scales = torch.ones(R, 1, dtype=module.weight.dtype) if granularity == 'per_channel' else torch.ones(1)
        return torch.zeros(R, K, dtype=FP8), scales, None
    return w_q


@pytest.mark.parametrize('cls_name', ['VllmRealQuantLinear', 'SglRealQuantLinear', 'LightllmRealQuantLinear', 'Lightx2vRealQuantLinear'])
def test_new_records_the_act_mode(cls_name):
    from llmc_amd.compression.quantization import module_utils as MU
    cls = getattr(MU, cls_name)
    lin = torch.nn.Linear(256, 48).to(torch.bfloat16)
    m = cls.new(lin, _stub_w_q('per_channel'), {'weight': W_CH, 'act': A_TOK, 'quant_type': 'float-quant'})
    assert m.act_mode == 'dynamic_per_token' and m.act_cfg == A_TOK and m.input_scale is None
    assert m.weight.dtype == FP8 and tuple(m.weight_scale.shape) == (48, 1)
    lin.register_buffer('buf_act_scales_0', torch.tensor(0.01))
    m = cls.new(lin, _stub_w_q('per_tensor'), {'weight': W_T, 'act': A_STATIC, 'quant_type': 'float-quant'})
    assert m.act_mode == 'static_per_tensor' and m.act_cfg == A_STATIC and m.input_scale.numel() == 1
    m = cls.new(lin, _stub_w_q('per_channel'), {'weight': W_CH})
    assert m.act_mode is None and m.act_cfg is None
    # a pairing forward does not run is recorded as the error it will raise, not raised by `new` (deploy + save still work)
    m = cls.new(lin, _stub_w_q('per_channel'), {'weight': W_CH, 'act': dict(A_TOK, bit='e5m2')})
    assert isinstance(m.act_mode, NotImplementedError)
    with pytest.raises(NotImplementedError, match='e5m2'):
        m(torch.zeros(2, 256, dtype=torch.bfloat16))


def test_forward_still_refuses_the_other_stored_forms():
    from llmc_amd.compression.quantization.module_utils import VllmRealQuantLinear
    x = torch.zeros(2, 256, dtype=torch.bfloat16)
    # packed integers (weight_packed)
    m = VllmRealQuantLinear(torch.zeros(48, 32, dtype=torch.int32), None, torch.ones(48, 2, dtype=torch.float16), None, True, 'weight_scale')
    with pytest.raises(NotImplementedError, match='weight_packed'):
        m(x)
    # per_block scales (weight_scale_inv)
    m = VllmRealQuantLinear(torch.zeros(48, 256, dtype=FP8), None, torch.ones(1, 2), None, False, 'weight_scale_inv')
    with pytest.raises(NotImplementedError, match='per_block'):
        m(x)
    # int8 and e5m2 weights
    for dt in (torch.int8, torch.float8_e5m2):
        m = VllmRealQuantLinear(torch.zeros(48, 256, dtype=dt), None, torch.ones(48, 1), None, False, 'weight_scale')
        with pytest.raises(NotImplementedError, match='weight dtype'):
            m(x)
