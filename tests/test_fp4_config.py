"""The narrow float formats at configuration time (no GPU): FloatQuantizer takes e2m1 / e3m2 with the reference's integer
ranges, Awq constructs from the shipped FP4 file, and the users that know only the two FP8 formats refuse a narrow-format
quantizer at construction with a NotImplementedError that names it."""
import json
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def shipped(name, rel):
    with open(os.path.join(HERE, 'golden', name)) as f:
        return json.load(f)[rel]


def construct(q, cfg=None, skip_collect=False):
    import llmc_amd.compression.quantization as Q
    from toy_model import ToyModel, calib_input
    model = ToyModel()
    cfg = cfg or {}
    cls = getattr(Q, q['method'])
    if skip_collect and hasattr(cls, 'collect_model_qparams'):       # compute, not configuration (tests/test_config_acceptance.py)
        class NoCollect(cls):
            def collect_model_qparams(self):
                pass
        cls = NoCollect
    config = {'calib': cfg.get('calib') or {}, 'model': cfg.get('model') or {}, 'quant': q}
    return cls(model, dict(q), calib_input(model), None, config)


def test_quantizer_takes_the_narrow_formats():
    from llmc_amd.compression.quantization import FloatQuantizer
    q = FloatQuantizer('e2m1', True, 'per_group', group_size=128, use_qtorch=True)
    assert int(q.qmax) == 6 and int(q.qmin) == -6 and q.qmax.dtype == torch.int64 and q.qmax.dim() == 0
    assert (q.e_bits, q.m_bits, q.num_bits) == (2, 1, 4) and q.sym and q.float_semantics == 'qtorch' and q.scale_format == 'dtype'
    q6 = FloatQuantizer('e3m2', True, 'per_channel', use_qtorch=True, float_semantics='ocp')
    assert int(q6.qmax) == 28 and (q6.e_bits, q6.m_bits, q6.num_bits) == (3, 2, 6)
    mx = FloatQuantizer('e2m1', True, 'per_group', group_size=32, use_qtorch=True, float_semantics='ocp', scale_format='e8m0')
    assert mx.scale_format == 'e8m0'
    for gran in ('per_tensor', 'per_token'):
        FloatQuantizer('e2m1', True, gran, use_qtorch=True)
    # the 8-bit formats are what they were
    q8 = FloatQuantizer('e4m3', True, 'per_channel', use_qtorch=True)
    assert float(q8.qmax) == 448.0 and q8.qmax.dtype == torch.float32 and not q8.narrow


def test_quantizer_refusals():
    from llmc_amd.compression.quantization import FloatQuantizer
    with pytest.raises(ValueError, match='e8m0'):
        FloatQuantizer('e2m1', True, 'per_group', group_size=32, use_qtorch=True, scale_format='e8m0')
    with pytest.raises(ValueError, match='e8m0'):
        FloatQuantizer('e2m1', True, 'per_channel', use_qtorch=True, float_semantics='ocp', scale_format='e8m0')
    with pytest.raises(ValueError, match='e8m0'):
        FloatQuantizer('e4m3', True, 'per_group', group_size=32, use_qtorch=True, scale_format='e8m0')
    with pytest.raises(ValueError, match='float_semantics'):
        FloatQuantizer('e2m1', True, 'per_channel', use_qtorch=True, float_semantics='rne')
    with pytest.raises(NotImplementedError, match='use_qtorch'):
        FloatQuantizer('e2m1', True, 'per_group', group_size=128)
    with pytest.raises(NotImplementedError, match='per_block'):
        FloatQuantizer('e2m1', True, 'per_block', block_size=128, use_qtorch=True)
    for algo in ('mse', 'hqq', 'learnable'):
        with pytest.raises(NotImplementedError, match=algo):
            FloatQuantizer('e2m1', True, 'per_group', group_size=128, use_qtorch=True, calib_algo=algo)
    with pytest.raises(NotImplementedError, match='e4m7'):
        FloatQuantizer('e4m7', True, 'per_channel', use_qtorch=True)


def test_awq_constructs_from_the_shipped_fp4_file():
    cfg = shipped('ref_quant_configs.json', 'methods/FP_Quant/awq_we2m1a16_g128.yml')
    from llmc_amd.compression.quantization import FloatQuantizer
    a = construct(cfg['quant'], cfg)
    assert isinstance(a.wquantizer, FloatQuantizer) and a.wquantizer.bit == 'e2m1' and a.wquantizer.narrow
    assert a.wquantizer.group_size == 128 and int(a.wquantizer.qmax) == 6 and a.w_only
    assert not a._fusable_wquantizer()              # the integer fusion is not taken: the narrow-format form is its own


def _e2m1(gran='per_group', **kw):
    w = dict(bit='e2m1', symmetric=True, granularity=gran, quant_type='float-quant', use_qtorch=True, **kw)
    if gran == 'per_group':
        w.setdefault('group_size', 128)
    return w


def test_gptq_refuses_a_narrow_format_quantizer():
    cfg = shipped('ref_quant_configs.json', 'methods/FP_Quant/gptq_we2m1a16_g128.yml')
    with pytest.raises(NotImplementedError, match='e2m1'):
        construct(cfg['quant'], cfg, skip_collect=True)
    from llmc_amd.compression.quantization.gptq_pipeline import GptqConfig
    with pytest.raises(NotImplementedError, match='e2m1'):
        GptqConfig(bit='e2m1')


def test_spqr_refuses_a_narrow_format_quantizer():
    cfg = shipped('ref_quant_configs.json', 'methods/SpQR/spqr_w_only.yml')
    q = dict(cfg['quant'], weight=_e2m1(group_size=cfg['quant']['weight'].get('group_size', 16)))
    with pytest.raises(NotImplementedError, match='e2m1'):
        construct(q, cfg, skip_collect=True)


@pytest.mark.parametrize('which', ['act', 'weight'])
def test_osplus_refuses_a_narrow_format_quantizer(which):
    cfg = shipped('ref_smooth_osplus_configs.json', 'methods/OsPlus/osplus_w_a.yml')
    q = dict(cfg['quant'])
    if which == 'act':
        q['act'] = dict(bit='e2m1', symmetric=True, granularity='per_token', quant_type='float-quant', use_qtorch=True)
    else:
        q['weight'] = _e2m1('per_channel')
    with pytest.raises(NotImplementedError, match='e2m1'):
        construct(q, cfg)


def test_entry_points_refuse_what_they_do_not_know():
    """Argument checks only: nothing reaches a GPU."""
    from llmc_amd import _ffi
    L = _ffi.lib()
    one = 1        # a non-null stand-in pointer; the calls return before touching it
    assert L.llmc_fpx_quant(one, 1, 4, 128, None, 0, 0x01 | (1 << 4), one, one, 1, 1, None, None) == -95       # format e5m2
    assert 'e2m1' in _ffi.last_error()
    assert L.llmc_fpx_quant(one, 1, 4, 128, None, 0, 0x01 | (2 << 4) | 0x200, one, one, 1, 1, None, None) == -95   # e8m0 without ocp
    assert 'ocp' in _ffi.last_error()
    assert L.llmc_fpx_quant(one, 1, 4, 128, None, 0, 0x01 | (2 << 4) | 0x1000, one, one, 1, 1, None, None) == -95  # unknown bit
    assert L.llmc_fpx_quant(None, 1, 4, 128, None, 0, 0x01 | (2 << 4), one, one, 1, 1, None, None) == -22
    assert L.llmc_fp8_quant(one, 1, 4, 128, 0x01 | (2 << 4), one, one, 1, 1, None, None) == -95                  # the FP8 entry refuses e2m1
    assert L.llmc_fpx_dequant(one, 3, 1, one, 1, 4, 128, one, 1, None) == -95                                    # no packed FP6
    assert L.llmc_fp4_pack(one, 4, 127, one, None) == -22                                                        # odd K
    assert L.llmc_fpx_quant_ws_bytes(1, 1 << 22) == L.llmc_fp8_quant_ws_bytes(1, 1 << 22) > 0
