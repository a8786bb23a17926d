"""The QUIK real-quant Linear at configuration time (no GPU): the map entry, what QuikRealQuantLinear.new stores, the pairings
forward refuses, the entry points' host checks and the wrappers' argument checks."""
import pytest
import torch

W = dict(bit=8, symmetric=True, granularity='per_channel', group_size=-1)
A = dict(bit=8, symmetric=True, granularity='per_token')


def _linear(K, N, F, dtype=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed)
    m = torch.nn.Linear(K, N, bias=True, dtype=dtype)
    m.weight.data = torch.randn(N, K, generator=g).to(dtype)
    order = torch.randperm(K, generator=g)
    m.register_buffer('buf_int_ids', order[:K - F])
    m.register_buffer('buf_fp_ids', order[K - F:])
    return m


def _stub_w_q(module):
    """symmetric int8 per row over the int columns, in plain torch: stands in for QUIK.w_q"""
    w = module.weight.data.float().index_select(1, module.buf_int_ids)
    s = w.abs().amax(1, keepdim=True).clamp_min(1e-5) / 127
    return torch.round(w / s).clamp(-128, 127).to(torch.int8), s.reshape(-1), None


def test_map_entry_and_linear_types():
    from llmc_amd.compression.quantization import module_utils as MU
    assert MU._REALQUANT_LINEAR_MAP_['quik_quant'] is MU.QuikRealQuantLinear
    assert MU.QuikRealQuantLinear in MU._LLMC_LINEAR_TYPES_


@pytest.mark.parametrize('K,F,Ki,Fp', [(320, 24, 320, 32), (256, 32, 256, 32), (320, 0, 320, 0), (64, 24, 64, 32)])
def test_new_stores_the_padded_form(K, F, Ki, Fp):
    from llmc_amd.compression.quantization.module_utils import QuikRealQuantLinear
    lin = _linear(K, 48, F)
    m = QuikRealQuantLinear.new(lin, _stub_w_q, {'weight': W, 'act': A})
    n_int = K - F
    codes, scales, _ = _stub_w_q(lin)
    assert m.weight.dtype == torch.int8 and tuple(m.weight.shape) == (48, Ki)
    assert torch.equal(m.weight[:, :n_int], codes) and not m.weight[:, n_int:].any()
    assert m.weight_scale.dtype == torch.float32 and tuple(m.weight_scale.shape) == (48, 1)
    assert torch.equal(m.weight_scale.reshape(-1), scales)
    assert m.weight_fp.dtype == torch.bfloat16 and tuple(m.weight_fp.shape) == (48, Fp)
    assert torch.equal(m.weight_fp[:, :F], lin.weight.data.index_select(1, lin.buf_fp_ids))
    assert not m.weight_fp[:, F:].view(torch.int16).any()                      # +0, not -0
    assert m.int_ids.dtype == m.fp_ids.dtype == m.col_map.dtype == torch.int32
    assert torch.equal(m.int_ids.long(), lin.buf_int_ids) and torch.equal(m.fp_ids.long(), lin.buf_fp_ids)
    want = torch.cat([torch.arange(n_int), Ki + torch.arange(F)])              # a permutation onto the int and fp slots
    assert torch.equal(m.col_map[torch.cat([lin.buf_int_ids, lin.buf_fp_ids])].long(), want)
    assert torch.equal(m.bias, lin.bias.data) and m.act_mode == 'dynamic_per_token' and m.act_cfg == A


@pytest.mark.parametrize('cfg,why', [
    ({'weight': W, 'act': dict(A, symmetric=False)}, 'symmetric'),
    ({'weight': W, 'act': dict(A, bit=4)}, '8-bit'),
    ({'weight': W, 'act': dict(A, granularity='per_tensor', static=True)}, 'static'),
    ({'weight': dict(W, granularity='per_group', group_size=32)}, 'per_channel'),
    ({'weight': dict(W, symmetric=False), 'act': A}, 'per_channel'),
    ({'weight': W}, 'act'),
])
def test_refused_pairings_are_recorded_and_raised_by_forward(cfg, why):
    from llmc_amd.compression.quantization.module_utils import QuikRealQuantLinear
    m = QuikRealQuantLinear.new(_linear(64, 16, 8), _stub_w_q, cfg)             # deploy and save still work
    assert isinstance(m.act_mode, NotImplementedError)
    with pytest.raises(NotImplementedError, match=why):
        m(torch.zeros(2, 64, dtype=torch.bfloat16))


def test_entry_points_host_checks():
    from llmc_amd import _ffi
    L = _ffi.lib()
    p, bf16 = 1 << 12, _ffi.dt(torch.bfloat16)
    ok = dict(A8=p, a_s=p, A_fp=p, W8=p, w_s=p, W_fp=p, M=4, N=8, Ki=64, Fp=32, fp_dt=bf16, out_dt=bf16, bias=None, C=p)

    def gemm(rung=-1, **kw):
        return L.llmc_quik_gemm_on_rung(*{**ok, **kw}.values(), rung, None)

    assert gemm(Ki=96) == -95 and gemm(Fp=16) == -95 and gemm(Ki=65536 + 64) == -95       # LLMC_ENOTSUP: nothing is launched
    assert gemm(A8=None) == -22 and gemm(A_fp=None) == -22 and gemm(W8=p + 8) == -22 and gemm(fp_dt=_ffi.dt(torch.float32)) == -22
    assert gemm(rung=2) == -22 and gemm(rung=0, M=65) == -22
    assert L.llmc_quik_gemm_rung(1, 4096) == 0 and L.llmc_quik_gemm_rung(64, 4096) == 0 and L.llmc_quik_gemm_rung(65, 4096) == 1
    assert L.llmc_quik_act_split_fits(bf16, 4096, 3840, 256) == 1 and L.llmc_quik_act_split_fits(bf16, 4100, 4160, 0) == 0
    assert L.llmc_quik_act_split_fits(_ffi.dt(torch.float32), 4096, 3840, 256) == 0
    assert L.llmc_quik_act_split_fits(bf16, 1 << 17, 1 << 17, 0) == 0                     # a row wider than the LDS of a CU
    assert L.llmc_quik_act_split(p, bf16, 2, 1 << 17, p, 1 << 17, 0, p, p, None, None) == -95


def test_wrappers_check_arguments_and_refuse_cpu_tensors():
    from llmc_amd import _ffi
    from llmc_amd.compression.quantization import quik_ops as QK
    a8, w8 = torch.zeros(3, 64, dtype=torch.int8), torch.zeros(16, 64, dtype=torch.int8)
    a_fp, w_fp = torch.zeros(3, 32, dtype=torch.bfloat16), torch.zeros(16, 32, dtype=torch.bfloat16)
    a_s, w_s = torch.ones(3, 1), torch.ones(16, 1)
    with pytest.raises(TypeError, match='a8'):
        QK.quik_gemm(a8.float(), a_s, a_fp, w8, w_s, w_fp)
    with pytest.raises(TypeError, match='outlier'):
        QK.quik_gemm(a8, a_s, a_fp.half(), w8, w_s, w_fp)
    with pytest.raises(ValueError, match='activation parts'):
        QK.quik_gemm(a8, a_s, a_fp[:, :16], w8, w_s, w_fp)
    with pytest.raises(ValueError, match='a_s'):
        QK.quik_gemm(a8, a_s[:1], a_fp, w8, w_s, w_fp)
    with pytest.raises(ValueError, match='bias'):
        QK.quik_gemm(a8, a_s, a_fp, w8, w_s, w_fp, bias=torch.zeros(3))
    with pytest.raises(ValueError, match='rung'):
        QK.quik_gemm(a8, a_s, a_fp, w8, w_s, w_fp, rung='decode_split')
    with pytest.raises(ValueError, match='64 tokens'):
        QK.quik_gemm(torch.zeros(65, 64, dtype=torch.int8), torch.ones(65), torch.zeros(65, 32, dtype=torch.bfloat16), w8, w_s, w_fp,
                     rung='decode')
    x, col_map = torch.zeros(3, 88, dtype=torch.bfloat16), torch.arange(88, dtype=torch.int32)
    with pytest.raises(TypeError, match='bf16'):
        QK.quik_act_split(x.float(), col_map, 64, 32)
    with pytest.raises(ValueError, match='col_map'):
        QK.quik_act_split(x, col_map.long(), 64, 32)
    with pytest.raises(ValueError, match='Ki'):
        QK.quik_act_split(x, col_map, 128, 64)
    with pytest.raises(_ffi.LlmcHipError, match='no CPU fallback'):
        QK.quik_act_split(x, col_map, 64, 32)
    with pytest.raises(_ffi.LlmcHipError, match='no CPU fallback'):
        QK.quik_gemm(a8, a_s, a_fp, w8, w_s, w_fp)
