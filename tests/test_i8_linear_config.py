"""The W8A8 integer Linear at configuration time (no GPU): which `act` sections i8_linear_ops.act_mode takes, the entry point's
host-side return codes and ladder, the wrapper's shape and dtype checks, what VllmRealQuantLinear.new records for an int8 weight,
and the weight-only int8 module that still does not run."""
import pytest
import torch

W_CH = dict(bit=8, symmetric=True, granularity='per_channel', group_size=-1)
A_TOK = dict(bit=8, symmetric=True, granularity='per_token')
A_STATIC = dict(bit=8, symmetric=True, granularity='per_tensor', static=True)


def test_act_mode_names_the_two_pairings_and_refuses_the_rest():
    from llmc_amd.compression.quantization.i8_linear_ops import act_mode
    assert act_mode(None) is None
    assert act_mode(A_TOK) == 'dynamic_per_token' and act_mode(dict(A_TOK, quant_type='int-quant')) == 'dynamic_per_token'
    assert act_mode(A_STATIC) == 'static_per_tensor'
    for bad, reason in ((dict(A_TOK, symmetric=False), 'asymmetric'), (dict(A_TOK, bit=4), 'bit 4'),
                        (dict(A_TOK, bit='e4m3', quant_type='float-quant'), 'float-quant'),
                        (dict(A_TOK, granularity='per_tensor'), 'dynamic per_tensor'), (dict(A_STATIC, granularity='per_token'), 'static per_token'),
                        (dict(A_TOK, granularity='per_group', group_size=128), 'dynamic per_group')):
        with pytest.raises(NotImplementedError, match=reason):
            act_mode(bad)


def test_entry_point_return_codes_and_ladder():
    from llmc_amd import _ffi
    L = _ffi.lib()
    p = 1 << 12        # an aligned non-null stand-in pointer; the calls return before touching it
    ok = dict(A=p, a_s=p, a_s_n=4, B=p, b_s=p, b_s_n=8, M=4, N=8, K=24, out_dt=_ffi.dt(torch.bfloat16), bias=None, C=p, ws=None, ws_bytes=0,
              rung=-1, stream=None)

    def gemm(**kw):
        return L.llmc_i8_scaled_gemm_on_rung(*{**ok, **kw}.values())

    assert gemm() == -95 and '16' in _ffi.last_error()                   # everything valid but the depth: LLMC_ENOTSUP
    assert gemm(K=65536 + 16) == -95 and '65536' in _ffi.last_error()
    for name in ('A', 'a_s', 'B', 'b_s', 'C'):
        assert gemm(**{name: None}) == -22, name
    assert gemm(A=p + 8) == -22 and 'align' in _ffi.last_error()
    assert gemm(a_s_n=3) == -22 and gemm(b_s_n=7) == -22 and gemm(out_dt=7) == -22 and gemm(M=0) == -22
    assert gemm(rung=3) == -22 and gemm(rung=-2) == -22 and gemm(rung=0, M=65, a_s_n=65) == -22 and gemm(rung=2, M=65, a_s_n=65) == -22
    assert gemm(K=32, rung=2) == -22 and 'workspace' in _ffi.last_error()          # decode_split without its workspace
    assert gemm(K=32, rung=2, ws=p, ws_bytes=L.llmc_i8_scaled_gemm_ws_bytes(4, 8, 32) - 1) == -22
    # the ladder: the decode rungs up to 64 tokens, the tile rung above; a workspace only where a decode rung can run
    assert L.llmc_i8_scaled_gemm_rung(64, 4096, 4096) in (0, 2) and L.llmc_i8_scaled_gemm_rung(65, 4096, 4096) == 1
    assert L.llmc_i8_scaled_gemm_ws_bytes(64, 4096, 4096) >= 64 * 4096 * 4 and L.llmc_i8_scaled_gemm_ws_bytes(65, 4096, 4096) == 0
    with _ffi.option(i8_split_slices=4):
        assert L.llmc_i8_scaled_gemm_ws_bytes(2, 16, 4096) == 4 * 2 * 16 * 4 and L.llmc_i8_scaled_gemm_ws_bytes(2, 16, 256) == 2 * 2 * 16 * 4


def test_wrapper_checks_shapes_before_any_gpu_use():
    from llmc_amd.compression.quantization import i8_linear_ops as I8
    a8, w8 = torch.zeros(3, 128, dtype=torch.int8), torch.zeros(16, 128, dtype=torch.int8)
    a_s, w_s = torch.ones(3, 1), torch.ones(16, 1)
    for exc, match, args, kw in ((TypeError, 'a8', (a8.float(), a_s, w8, w_s), {}), (TypeError, 'w8', (a8, a_s, w8.view(torch.uint8), w_s), {}),
                                 (ValueError, 'disagree on K', (a8, a_s, torch.zeros(16, 256, dtype=torch.int8), w_s), {}),
                                 (ValueError, 'a_s', (a8, torch.ones(2), w8, w_s), {}), (ValueError, 'w_s', (a8, a_s, w8, torch.ones(15)), {}),
                                 (TypeError, 'a_s', (a8, a_s.double(), w8, w_s), {}), (TypeError, 'output', (a8, a_s, w8, w_s), {'dtype': torch.float64}),
                                 (ValueError, 'bias', (a8, a_s, w8, w_s), {'bias': torch.zeros(3)}), (ValueError, r'\[N, K\]', (a8, a_s, w8[0], w_s), {}),
                                 (ValueError, 'rung', (a8, a_s, w8, w_s), {'rung': 'tile256'}),
                                 (ValueError, '64 tokens', (torch.zeros(65, 128, dtype=torch.int8), torch.ones(65), w8, w_s), {'rung': 'decode_split'}),
                                 (Exception, 'MI355X only', (a8, a_s, w8, w_s), {})):       # in order: the first GPU use refuses CPU tensors
        with pytest.raises(exc, match=match):
            I8.i8_scaled_gemm(*args, **kw)


@pytest.mark.parametrize('cls_name', ['VllmRealQuantLinear', 'SglRealQuantLinear', 'LightllmRealQuantLinear', 'Lightx2vRealQuantLinear'])
def test_new_records_the_act_mode_of_an_int8_weight(cls_name):
    from llmc_amd.compression.quantization import module_utils as MU
    cls = getattr(MU, cls_name)
    lin = torch.nn.Linear(256, 48).to(torch.bfloat16)

    def w_q(module):
        return torch.zeros(48, 256, dtype=torch.int8), torch.ones(48, 1, dtype=module.weight.dtype), None

    m = cls.new(lin, w_q, {'weight': W_CH, 'act': A_TOK})
    assert m.act_mode == 'dynamic_per_token' and m.act_cfg == A_TOK and m.input_scale is None and m.weight.dtype == torch.int8
    lin.register_buffer('buf_act_scales_0', torch.tensor(0.01))
    m = cls.new(lin, w_q, {'weight': W_CH, 'act': A_STATIC})
    assert m.act_mode == 'static_per_tensor' and tuple(m.input_scale.shape) == (1,)
    # a pairing forward does not run is recorded as the error it will raise, not raised by `new` (deploy + save still work)
    m = cls.new(lin, w_q, {'weight': W_CH, 'act': dict(A_TOK, symmetric=False)})
    assert isinstance(m.act_mode, NotImplementedError)
    with pytest.raises(NotImplementedError, match='asymmetric'):
        m(torch.zeros(2, 256, dtype=torch.bfloat16))
    # weight-only int8: no act section recorded, by `new` or by hand; forward names the dtype and what is out of scope
    for m in (cls.new(lin, w_q, {'weight': W_CH}), cls(torch.zeros(48, 256, dtype=torch.int8), None, torch.ones(48, 1), None, False, 'weight_scale')):
        assert m.act_mode is None
        with pytest.raises(NotImplementedError, match='weight dtype.*weight-only'):
            m(torch.zeros(2, 256, dtype=torch.bfloat16))
