"""GPTQ with a float weight quantizer: what the column loop has an FP8 grid for is routed to it at construction, what it has
none for is refused there with a NotImplementedError that says why. Construction only (no GPU): the class's
collect_model_qparams — compute — is skipped as tests/test_config_acceptance.py does."""
import json
import os

import pytest


class Cfg(dict):
    __getattr__ = dict.get


def shipped_quant():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_quant_configs.json')
    with open(path) as f:
        return json.load(f)['backend/vllm/fp8/gptq_fp8.yml']['quant']


def construct(weight=None, special=None):
    import llmc_amd.compression.quantization as Q
    from toy_model import ToyModel, calib_input
    q = shipped_quant()
    q['weight'] = dict(q['weight'], **(weight or {}))
    q['special'] = dict(q['special'], **(special or {}))

    class NoCollect(Q.GPTQ):
        def collect_model_qparams(self):
            pass
    model = ToyModel()
    return NoCollect(model, q, calib_input(model), None, Cfg(calib=Cfg(seq_len=64), model=Cfg(type='Toy')))


def test_shipped_file_routes_to_the_fp8_loop():
    a = construct()
    assert a.fp8 == 'e4m3' and a.gcfg.fp8 == 'e4m3' and a.gcfg.symmetric and a.gcfg.group_size == 0
    assert a.gcfg.qrange == (-448.0, 448.0) and not a.need_perm
    b = construct(weight=dict(bit='e5m2', granularity='per_group', group_size=128))
    assert b.fp8 == 'e5m2' and b.gcfg.qrange == (-57344.0, 57344.0) and b.gcfg.group_size == 128 and b.need_perm
    c = construct(weight=dict(granularity='per_group', group_size=64), special=dict(static_groups=True))
    assert c.fp8 == 'e4m3' and c.gcfg.static_groups and not c.need_perm


def test_integer_quantizers_are_not_routed():
    import llmc_amd.compression.quantization as Q
    from toy_model import ToyModel, calib_input
    q = dict(shipped_quant(), weight=dict(bit=8, symmetric=True, granularity='per_channel'))
    q.pop('act')

    class NoCollect(Q.GPTQ):
        def collect_model_qparams(self):
            pass
    model = ToyModel()
    a = NoCollect(model, q, calib_input(model), None, Cfg(calib=Cfg(seq_len=64), model=Cfg(type='Toy')))
    assert a.fp8 is None and a.gcfg.fp8 is None and a.gcfg.qrange == (-128.0, 127.0)


@pytest.mark.parametrize('weight,special,reason', [
    (dict(fp8_semantics='cast'), None, 'NaN'),
    (dict(calib_algo='mse'), None, 'calib_algo=mse'),
    (dict(calib_algo='hqq'), None, 'hqq'),
    (dict(granularity='per_block', block_size=128), None, 'per_block'),
    (dict(granularity='per_tensor'), None, 'per_tensor scale'),
    (dict(granularity='per_group', group_size=128), dict(owq=True, n_outs=[4, 4, 4]), 'owq'),
])
def test_unsupported_combinations_are_refused_with_a_reason(weight, special, reason):
    with pytest.raises(NotImplementedError, match=reason):
        construct(weight=weight, special=special)


def test_pipeline_config_takes_the_formats_and_refuses_the_rest():
    from llmc_amd.compression.quantization.gptq_pipeline import GptqConfig
    assert GptqConfig(bit='e4m3', group_size=0).fp8 == 'e4m3' and GptqConfig(bit='e5m2').symmetric
    assert GptqConfig(bit=4).fp8 is None
    with pytest.raises(NotImplementedError, match='e4m3 and e5m2'):
        GptqConfig(bit='e2m1')
    with pytest.raises(NotImplementedError, match='mse'):
        GptqConfig(bit='e4m3', mse=(True, 80, 100, 2.4))


def test_entry_point_refuses_an_unknown_format_without_touching_the_gpu():
    from llmc_amd import _ffi
    rc = _ffi.lib().llmc_gptq_quantize_fp8_cols(None, None, 8, 256, 256, 2, 0, 0, None, None, None, None, 128, None, None)
    assert rc == -95 and 'fmt' in _ffi.last_error()
