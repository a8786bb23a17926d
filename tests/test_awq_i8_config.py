"""The W4A8 Linear on AutoAWQ's GEMM layout at configuration time (no GPU): what AutoawqRealQuantLinear.new records from the `act`
section, the wrapper's argument checks, and the entry point's host-side return codes."""
import pytest
import torch

A_TOK = dict(bit=8, symmetric=True, granularity='per_token')
A_STATIC = dict(bit=8, symmetric=True, granularity='per_tensor', static=True)
W_G = {'bit': 4, 'group_size': 128, 'pack_version': 'gemm_pack'}


@pytest.mark.parametrize('cls_name', ['AutoawqRealQuantLinear', 'MlcllmRealQuantLinear'])
def test_new_records_the_act_section(cls_name, monkeypatch):
    from llmc_amd.compression.quantization import module_utils as MU
    # the packing kernel needs a GPU; what `new` records does not depend on the packed words
    monkeypatch.setattr(MU, 'pack_awq_gemm', lambda w, s, z, g: (torch.zeros(256, 6, dtype=torch.int32), torch.ones(2, 48, dtype=torch.float16),
                                                                 torch.zeros(2, 6, dtype=torch.int32)))
    cls = getattr(MU, cls_name)
    lin = torch.nn.Linear(256, 48).to(torch.bfloat16)
    lin.register_buffer('buf_act_scales_0', torch.tensor(0.01))

    def w_q(module):
        return None, torch.ones(48, 2), torch.zeros(48, 2)

    m = cls.new(lin, w_q, {'weight': W_G, 'act': A_TOK})
    assert m.act_mode == 'dynamic_per_token' and m.act_cfg == A_TOK and 'input_scale' not in m.state_dict()
    m = cls.new(lin, w_q, {'weight': W_G, 'act': A_STATIC})
    assert m.act_mode == 'static_per_tensor' and tuple(m.state_dict()['input_scale'].shape) == (1,)
    # a pairing forward does not run is recorded as the error it will raise, not raised by `new` (deploy + save still work)
    for bad, reason in ((dict(A_TOK, symmetric=False), 'asymmetric'), (dict(A_TOK, bit=4), 'bit 4')):
        m = cls.new(lin, w_q, {'weight': W_G, 'act': bad})
        assert isinstance(m.act_mode, NotImplementedError)
        with pytest.raises(NotImplementedError, match=reason):
            m(torch.zeros(2, 256, dtype=torch.bfloat16))
    for m in (cls.new(lin, w_q, {'weight': W_G}), cls(torch.zeros(256, 6, dtype=torch.int32), None, torch.ones(2, 48), torch.zeros(2, 6))):
        assert m.act_mode is None and m.act_cfg is None and 'input_scale' not in m.state_dict()


def test_wrapper_checks_arguments_before_any_gpu_use():
    from llmc_amd.compression.quantization.awq_gemm_ops import awq_i8_gemm
    a8, a_s = torch.zeros(3, 128, dtype=torch.int8), torch.ones(3, 1)
    qw, qz, sc = torch.zeros(128, 2, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32), torch.ones(1, 16, dtype=torch.float16)
    for exc, match, args, kw in ((TypeError, 'int32', (a8, a_s, qw.long(), qz, sc, 128), {}), (ValueError, 'qzeros', (a8, a_s, qw, qz[:, :1], sc, 128), {}),
                                 (TypeError, 'a8', (a8.float(), a_s, qw, qz, sc, 128), {}), (ValueError, 'disagree on K', (a8[:, :64], a_s, qw, qz, sc, 128), {}),
                                 (ValueError, 'a_s', (a8, torch.ones(2), qw, qz, sc, 128), {}), (TypeError, 'a_s', (a8, a_s.double(), qw, qz, sc, 128), {}),
                                 (TypeError, 'output', (a8, a_s, qw, qz, sc, 128), {'dtype': torch.float32}),
                                 (ValueError, 'bias', (a8, a_s, qw, qz, sc, 128), {'bias': torch.zeros(3)}),
                                 (ValueError, 'rung', (a8, a_s, qw, qz, sc, 128), {'rung': 'decode'}),
                                 (Exception, 'MI355X only', (a8, a_s, qw, qz, sc, 128), {})):       # in order: the first GPU use refuses CPU tensors
        with pytest.raises(exc, match=match):
            awq_i8_gemm(*args, **kw)


def test_entry_point_return_codes_are_host_side():
    from llmc_amd import _ffi
    L = _ffi.lib()
    p = 1 << 12        # an aligned non-null stand-in pointer; the calls return before touching it
    ok = dict(a8=p, a_s=p, a_s_n=4, M=4, K=256, R=16, qw=p, qz=p, sc=p, g=128, dt=_ffi.dt(torch.bfloat16), bias=None, y=p, ws=None, ws_bytes=0,
              rung=0, stream=None)

    def gemm(**kw):
        return L.llmc_awq_i8_gemm_on_rung(*{**ok, **kw}.values())

    assert gemm() == -22 and 'workspace' in _ffi.last_error()             # everything valid but the stream rung's workspace
    assert gemm(ws=p, ws_bytes=L.llmc_awq_i8_gemm_ws_bytes(4, 256, 16, 128) - 1) == -22
    for name in ('a8', 'a_s', 'qw', 'qz', 'sc', 'y'):
        assert gemm(**{name: None}) == -22, name
    assert gemm(dt=_ffi.dt(torch.float32)) == -22 and gemm(R=12) == -22 and gemm(g=96) == -22 and gemm(a_s_n=3) == -22
    assert gemm(rung=2) == -22 and gemm(rung=-2) == -22
    assert gemm(g=16) == -95 and '32' in _ffi.last_error()
    assert gemm(K=16384, g=16384) == -95 and '8192' in _ffi.last_error()
    assert gemm(a8=p + 8) == -95 and 'align' in _ffi.last_error()
    assert gemm(K=1 << 22) == -95 and '2^22' in _ffi.last_error()
    # pure host calls: one fp32 [M, R] per slice of whole groups; the ladder's rung
    assert L.llmc_awq_i8_gemm_ws_bytes(4, 256, 16, 128) == 2 * 4 * 16 * 4 and L.llmc_awq_i8_gemm_ws_bytes(4, 256, 16, 16) == 0
    assert L.llmc_awq_i8_gemm_rung(64, 4096, 4096) == 0 and L.llmc_awq_i8_gemm_rung(65, 4096, 4096) == 1
