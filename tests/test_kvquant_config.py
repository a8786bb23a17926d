"""The `quant.kvcache` section (base_blockwise_quantization.py:200-216 of the reference) without a GPU: the four shipped configs
that carry it construct a cache of the right class or are refused with a reason, the registry, the cache's bookkeeping
(_reset_states, use_org_kv, deploy's switch) and the attention pre-hook under both spellings of the keyword."""
import copy
import json
import os

import pytest
import torch

from conftest import GOLDEN

SHIPPED = {
    'methods/RTN/rtn_w_a_kv.yml': 'Naive',
    'methods/KVQuant/rtn_w_a_naive_quant_kv.yml': 'Naive',
    'methods/KVQuant/rtn_w_a_kivi_quant_kv.yml': 'Kivi',
    'methods/KVQuant/rtn_w_a_pertensor_static_naive_quant_kv.yml': None,       # act.static: refused
}
W = {'bit': 8, 'symmetric': True, 'granularity': 'per_channel'}
KV8 = {'method': 'Naive', 'bit': 8, 'symmetric': True, 'granularity': 'per_token'}


def _shipped(rel):
    with open(os.path.join(GOLDEN, 'ref_quant_configs.json')) as f:
        return copy.deepcopy(json.load(f)[rel])


def _construct(quant, config=None):
    import llmc_amd.compression.quantization as Q
    from toy_model import ToyModel, calib_input
    model = ToyModel()
    cfg = {'quant': quant, **(config or {})}
    return getattr(Q, quant['method'])(model, quant, calib_input(model), None, cfg), model


@pytest.mark.parametrize('rel', sorted(SHIPPED))
def test_shipped_kvcache_sections_construct_or_are_refused_with_a_reason(rel):
    from llmc_amd.compression.quantization import kvquant
    cfg = _shipped(rel)
    assert 'kvcache' in cfg['quant']
    if SHIPPED[rel] is None:
        assert cfg['quant']['act']['static'] is True
        with pytest.raises(NotImplementedError, match='KV-cache.*static'):
            _construct(cfg['quant'], {'calib': cfg.get('calib') or {}})
        return
    algo, model = _construct(cfg['quant'])
    cls = {'Naive': kvquant.NaiveQuantKVCache, 'Kivi': kvquant.KiviQuantKVCache}[SHIPPED[rel]]
    assert type(algo.kv_module) is cls and algo.quant_kvcache is True
    assert model.kvcache_buffer == [algo.kv_module]
    assert algo.kv_module.num_hidden_layers == 2              # ToyModel's config has no num_hidden_layers: the number of blocks
    q = algo.kv_module.kvquantizer
    assert (q.bit, q.sym, q.granularity) == (8, True, 'per_token') and algo.kv_module.use_org_kv is False
    if SHIPPED[rel] == 'Kivi':
        assert algo.kv_module.residual_length == 128


def test_num_hidden_layers_comes_from_the_model_config_when_it_has_one():
    import llmc_amd.compression.quantization as Q
    from toy_model import ToyModel, calib_input
    model = ToyModel()
    model.model_config.num_hidden_layers = 7
    algo = Q.RTN(model, {'method': 'RTN', 'weight': W, 'kvcache': dict(KV8)}, calib_input(model), None, {})
    assert algo.kv_module.num_hidden_layers == 7


def test_registry_and_transformers_base_class():
    from llmc_amd.compression.quantization import kvquant
    from llmc_amd.utils.registry_factory import KV_REGISTRY
    assert KV_REGISTRY['Naive'] is kvquant.NaiveQuantKVCache and KV_REGISTRY['Kivi'] is kvquant.KiviQuantKVCache
    assert issubclass(kvquant.KiviQuantKVCache, kvquant.NaiveQuantKVCache)
    from transformers import DynamicCache
    assert isinstance(kvquant.NaiveQuantKVCache('int-quant', dict(KV8), 2), DynamicCache)


def test_unknown_methods_incomplete_sections_and_static_caches_raise():
    from llmc_amd.compression.quantization import kvquant
    with pytest.raises(NotImplementedError, match='KV-cache method'):
        _construct({'method': 'RTN', 'weight': W, 'kvcache': dict(KV8, method='SinkKV')})
    for drop in ('bit', 'symmetric', 'granularity'):
        kv = {k: v for k, v in KV8.items() if k != drop}
        with pytest.raises(NotImplementedError, match=f'KV-cache.*{drop}'):
            _construct({'method': 'RTN', 'weight': W, 'kvcache': kv})
    with pytest.raises(NotImplementedError, match='KV-cache.*per_channel'):
        _construct({'method': 'RTN', 'weight': W, 'kvcache': dict(KV8, granularity='per_channel')})
    with pytest.raises(NotImplementedError, match='static'):
        kvquant.NaiveQuantKVCache('int-quant', dict(KV8, static=True), 2)
    with pytest.raises(NotImplementedError, match='KIVI'):
        kvquant.KiviQuantKVCache('int-quant', dict(KV8, static=True), 2)
    with pytest.raises(ValueError):
        kvquant.NaiveQuantKVCache('no-quant', dict(KV8), 2)


@pytest.mark.parametrize('method', ['Naive', 'Kivi'])
def test_use_org_kv_is_plain_concatenation_and_reset_states_empties_the_cache(method):
    from llmc_amd.utils.registry_factory import KV_REGISTRY
    from llmc_amd.compression.quantization import kvquant  # noqa: F401
    cache = KV_REGISTRY[method]('int-quant', dict(KV8, method=method), 2, initial_capacity=4)
    assert cache.initial_capacity == 4 and cache.get_seq_length() == 0
    cache.use_org_kv = True
    g = torch.Generator().manual_seed(0)
    parts = [(torch.randn(1, 2, n, 16, generator=g).bfloat16(), torch.randn(1, 2, n, 16, generator=g).bfloat16()) for n in (3, 1, 2)]
    for layer in (0, 1):
        for i, (k, v) in enumerate(parts):
            ko, vo = cache.update(k, v, layer, {})
            assert torch.equal(ko, torch.cat([p[0] for p in parts[:i + 1]], dim=-2))
            assert torch.equal(vo, torch.cat([p[1] for p in parts[:i + 1]], dim=-2))
    assert cache.get_seq_length() == 6 and cache.get_seq_length(1) == 6 and cache.get_mask_sizes(2, 0) == (8, 0)
    cache._reset_states()
    assert cache.get_seq_length() == 0 and cache.get_seq_length(1) == 0 and not cache._layers and not cache._org
    ko, _ = cache.update(*parts[0], 0, {})
    assert ko.shape[-2] == 3


def test_deploy_switches_use_org_kv_by_format():
    algo, model = _construct({'method': 'RTN', 'weight': W, 'kvcache': dict(KV8)})
    model.replace_language_module_all = lambda *a, **k: None          # the Linear swap needs a GPU and is not what is tested
    for fmt, want in (('origin_float', True), ('fake_quant', False), ('fake_quant_wo_kv', True), ('fake_quant', False)):
        algo.deploy(fmt)
        assert algo.kv_module.use_org_kv is want, fmt


class _AttnOld(torch.nn.Module):
    def forward(self, hidden_states, past_key_value=None, **kwargs):
        self.got = dict(kwargs, past_key_value=past_key_value)
        return hidden_states


class _AttnNew(torch.nn.Module):
    def forward(self, hidden_states, past_key_values=None, **kwargs):
        self.got = dict(kwargs, past_key_values=past_key_values)
        return hidden_states


@pytest.mark.parametrize('attn_cls, key, other', [(_AttnOld, 'past_key_value', 'past_key_values'),
                                                  (_AttnNew, 'past_key_values', 'past_key_value')])
def test_the_hook_sets_the_keyword_the_attention_module_accepts(attn_cls, key, other):
    algo, _ = _construct({'method': 'RTN', 'weight': W, 'kvcache': dict(KV8)})
    block = torch.nn.Module()
    block.self_attn = attn_cls()
    algo.block_opt(block)                          # RTN.block_opt registers the cache when quant_kvcache is set
    assert block.self_attn.kvcache is algo.kv_module
    x = torch.zeros(1, 3, 8)
    block.self_attn(hidden_states=x)
    assert block.self_attn.got[key] is algo.kv_module and other not in block.self_attn.got
    assert 'cache_position' not in block.self_attn.got
    # eval.type decode_ppl: positions follow the cache's length
    algo.config = {'eval': {'type': 'decode_ppl'}}
    algo.kv_module.use_org_kv = True
    algo.kv_module.update(torch.zeros(1, 2, 5, 4), torch.zeros(1, 2, 5, 4), 0, {})
    block.self_attn(hidden_states=x)
    assert block.self_attn.got['cache_position'].tolist() == [5, 6, 7]
    assert block.self_attn.got['position_ids'].tolist() == [[5, 6, 7]]


def test_a_block_without_attention_is_refused_by_name():
    algo, model = _construct({'method': 'RTN', 'weight': W, 'kvcache': dict(KV8)})
    with pytest.raises(NotImplementedError, match='register_kv_cache'):
        algo.register_kv_cache(model.get_blocks()[0])
