"""The reference's QuaRot configurations (tests/golden/ref_quarot_configs.json, recorded by tools/make_golden_quarot.py), read as
they are: `Quarot` constructs from every step-1 file (the weight rewrite of `preprocess` is compute and is stubbed here; the GPU
suite runs it) or refuses with the stated reason; GPTQ constructs from both step_2_gptq.yml of quarot_comb_gptq with
online_rotate / fp32_had set; the algorithms that do not implement online rotation keep refusing it."""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_quarot_configs.json')


def configs():
    with open(GOLDEN) as f:
        return json.load(f)


def construct(cfg, method=None, model=None):
    import llmc_amd.compression.quantization as Q
    from rot_adapters import rot_llama
    model = model or rot_llama()
    q = dict(cfg['quant'])
    config = {'calib': cfg.get('calib') or {}, 'model': cfg.get('model') or {}, 'quant': q}
    cls = getattr(Q, method or q['method'])

    class Stubbed(cls):
        def collect_model_qparams(self):      # GPTQ: static qparams of every block on the GPU (compute)
            pass

        def preprocess(self):                 # Quarot: rotates the embedding and the head on the GPU (compute)
            self.preprocessed = True
    return Stubbed(model, q, None, None, config)


def test_quarot_is_registered():
    from llmc_amd.compression.quantization import Quarot
    from llmc_amd.utils.registry_factory import ALGO_REGISTRY
    assert ALGO_REGISTRY['Quarot'] is Quarot


def test_every_shipped_quarot_file_constructs_or_is_refused_with_the_reason():
    files = {k: v for k, v in configs().items() if v['quant']['method'] == 'Quarot'}
    assert len(files) >= 6
    for rel, cfg in sorted(files.items()):
        sp = cfg['quant']['special']
        if cfg['model'].get('type') == 'DeepseekV3':
            with pytest.raises(NotImplementedError, match='FP8'):
                construct(cfg)
            continue
        algo = construct(cfg)
        assert algo.preprocessed and algo.rotate_mode == 'hadamard', rel
        assert algo.online_rotate == sp['online_rotate'] and algo.fp32_had == sp['fp32_had'], rel
        assert (algo.hidden_size, algo.num_heads, algo.head_dim, algo.intermediate_size) == (256, 4, 64, 448)


def test_unsupported_quarot_settings_are_refused_with_a_reason():
    cfg = json.loads(json.dumps(configs()['methods/QuaRot/quarot_w_a.yml']))
    cfg['quant']['special']['rotate_mode'] = 'random'
    with pytest.raises(NotImplementedError, match='random'):
        construct(cfg)
    cfg['quant']['special']['rotate_mode'] = 'hadamard'
    for mtype in ('Opt', 'StableLm'):
        cfg['model']['type'] = mtype
        with pytest.raises(NotImplementedError, match='LayerNorm'):
            construct(cfg)
    cfg['model']['type'] = 'Llama'
    from toy_model import ToyModel
    with pytest.raises(NotImplementedError, match='get_embed_layers'):
        construct(cfg, model=ToyModel())                      # an adapter without the accessors QuaRot needs


def test_gptq_step_2_constructs_with_online_rotation():
    for rel in ('combination/quarot_comb_gptq/w4a4/step_2_gptq.yml', 'combination/quarot_comb_gptq/w8a8/step_2_gptq.yml'):
        algo = construct(configs()[rel])
        assert algo.online_rotate is True and algo.fp32_had is True and algo.true_sequential is True, rel
        p = algo.get_replacement_params(mode='online_rotate', w_only=algo.w_only, name='mlp.down_proj')
        assert p['K'] == 28 and tuple(p['had_K'].shape) == (28, 28) and p['online_full_had'] and not p['online_partial_had']
        assert p['had_dim'] is None and p['fp32_had'] is True
        p = algo.get_replacement_params(mode='online_rotate', w_only=algo.w_only, name='self_attn.o_proj')
        assert p['K'] == 1 and p['had_K'] is None and p['online_partial_had'] and not p['online_full_had'] and p['had_dim'] == 64


def test_online_rotation_without_true_sequential_is_refused_by_gptq():
    cfg = json.loads(json.dumps(configs()['combination/quarot_comb_gptq/w4a4/step_2_gptq.yml']))
    cfg['quant']['special']['true_sequential'] = False
    with pytest.raises(NotImplementedError, match='true_sequential'):
        construct(cfg)


@pytest.mark.parametrize('method', ['RTN', 'Awq'])
def test_other_algorithms_keep_refusing_online_rotation(method):
    cfg = json.loads(json.dumps(configs()['combination/quarot_comb_gptq/w4a4/step_2_gptq.yml']))
    q = cfg['quant']
    q['method'] = method
    q['weight']['calib_algo'] = 'minmax'
    q['special'] = {'online_rotate': True, 'fp32_had': True}
    if method == 'Awq':
        q['special'].update({'trans': True, 'trans_version': 'v2', 'weight_clip': False})
    with pytest.raises(NotImplementedError, match='online rotation'):
        construct(cfg)


def test_a_size_without_a_supported_factor_fails_at_construction():
    """Llama-2-7B's intermediate size 11008 = 172 * 64 needs a Williamson matrix"""
    from rot_adapters import rot_llama
    model = rot_llama()
    model.model_config.intermediate_size = 11008
    with pytest.raises(NotImplementedError, match='172'):
        construct(configs()['combination/quarot_comb_gptq/w4a4/step_2_gptq.yml'], model=model)
