"""SmoothQuant and OsPlus on the CPU: the shipped configurations, the classes' surface, the registry, the host threshold
loop against the reference's own list (tests/golden/smooth_osplus.npz, tools/make_golden_smooth_osplus.py) and the refusals."""
import ast
import inspect
import json
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden', 'smooth_osplus.npz')
CONFIGS = os.path.join(HERE, 'golden', 'ref_smooth_osplus_configs.json')
REF_DIR = os.path.join(os.path.dirname(HERE), 'oracle', '_ref', 'llmc', 'compression', 'quantization')
DT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}


def _gold():
    return np.load(GOLD)


def _section(cfg):
    """the section that names the method: `quant`, or one modality level down (quant.video_gen)"""
    q = cfg['quant']
    if 'method' in q:
        return q
    return next(v for v in q.values() if isinstance(v, dict) and 'method' in v)


def _construct(q, cfg=None):
    import llmc_amd.compression.quantization as Q
    from toy_model import ToyModel, calib_input
    model = ToyModel()
    cfg = cfg or {}
    config = {'calib': cfg.get('calib') or {}, 'model': cfg.get('model') or {}, 'quant': q}
    return getattr(Q, q['method'])(model, dict(q), calib_input(model), None, config)


# ---- configuration -------------------------------------------------------------------------------------------------------
def test_every_shipped_configuration_is_accepted_or_refused_with_a_reason():
    with open(CONFIGS) as f:
        configs = json.load(f)
    assert len(configs) == 14
    methods = {}
    for rel in sorted(configs):
        q = _section(configs[rel])
        assert q['method'] in ('SmoothQuant', 'OsPlus')
        try:
            obj = _construct(q, configs[rel])
        except NotImplementedError as e:
            assert str(e).strip(), rel                   # a refusal says what it refuses
            methods[rel] = 'refused'
            continue
        methods[rel] = 'accepted'
        assert not obj.w_only and obj.aquantizer is not None, rel
        if q['method'] == 'SmoothQuant':
            assert obj.alpha == (q.get('special') or {}).get('alpha', 0.5), rel
    for rel in ('backend/vllm/smoothquant_w8a8.yml', 'backend/vllm/fp8/smoothquant_fp8.yml', 'backend/sglang/smoothquant_w8a8.yml',
                'backend/sglang/fp8/smoothquant_fp8.yml', 'backend/trtllm/smoothquant_w8a8.yml',
                'methods/OsPlus/osplus_w_a.yml', 'methods/SmoothQuant/smoothquant_w_a.yml',
                'deepseekv3/osplus_w_a_dsv3.yml', 'deepseekv3/smoothquant_w_a_dsv3.yml'):
        assert methods[rel] == 'accepted', (rel, methods[rel])


def test_smoothquant_alpha_default():
    q = {'method': 'SmoothQuant', 'weight': dict(bit=8, symmetric=True, granularity='per_channel'),
         'act': dict(bit=8, symmetric=True, granularity='per_token')}
    assert _construct(q).alpha == 0.5
    q['special'] = {'alpha': 0.75}
    assert _construct(q).alpha == 0.75


def test_osplus_refusals_say_why():
    w = dict(bit=8, symmetric=True, granularity='per_channel')
    with pytest.raises(NotImplementedError, match='act'):
        _construct({'method': 'OsPlus', 'weight': w})
    with pytest.raises(NotImplementedError, match='static'):
        _construct({'method': 'OsPlus', 'weight': w,
                    'act': dict(bit=8, symmetric=True, granularity='per_tensor', static=True, calib_algo='static_minmax')})
    with pytest.raises(NotImplementedError, match='hqq'):
        _construct({'method': 'OsPlus', 'weight': dict(bit=4, symmetric=False, granularity='per_group', group_size=128,
                                                       calib_algo='hqq'),
                    'act': dict(bit=8, symmetric=True, granularity='per_token')})
    with pytest.raises(NotImplementedError, match='KV-cache'):
        _construct({'method': 'OsPlus', 'weight': w, 'act': dict(bit=8, symmetric=True, granularity='per_token'),
                    'kvcache': {'method': 'Naive', 'bit': 8}})


# ---- registry ------------------------------------------------------------------------------------------------------------
def test_register_into_binds_the_new_classes_on_request():
    import llmc_amd
    from llmc_amd.compression.quantization import OsPlus, SmoothQuant
    from llmc_amd.utils.registry_factory import ALGO_REGISTRY
    assert ALGO_REGISTRY['SmoothQuant'] is SmoothQuant and ALGO_REGISTRY['OsPlus'] is OsPlus
    d = {}
    assert sorted(llmc_amd.register_into(d)) == ['Awq', 'GPTQ', 'RTN', 'SpQR'] and len(d) == 4
    d = {}
    bound = llmc_amd.register_into(d, names=('GPTQ', 'Awq', 'RTN', 'SpQR', 'SmoothQuant', 'OsPlus'))
    assert d['SmoothQuant'] is SmoothQuant and d['OsPlus'] is OsPlus and len(bound) == 6


# ---- surface ---------------------------------------------------------------------------------------------------------------
def _ref_methods(path, cls_name):
    tree = ast.parse(open(path).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls_name)
    return {fn.name: [a.arg for a in fn.args.args] for fn in cls.body if isinstance(fn, ast.FunctionDef)}


@pytest.mark.skipif(not os.path.isdir(REF_DIR), reason='oracle/_ref (the reference build) is absent')
@pytest.mark.parametrize('mod,cls', [('smoothquant', 'SmoothQuant'), ('osplus', 'OsPlus')])
def test_surface_matches_reference(mod, cls):
    import llmc_amd.compression.quantization as Q
    ours = getattr(Q, cls)
    want = _ref_methods(os.path.join(REF_DIR, mod + '.py'), cls)
    mine = {n for n, f in vars(ours).items() if callable(f) and not n.startswith('_')} | {'__init__'}
    assert mine == set(want), (sorted(mine), sorted(want))
    for name, args in want.items():
        assert list(inspect.signature(getattr(ours, name)).parameters) == args, name


@pytest.mark.skipif(not os.path.isdir(REF_DIR), reason='oracle/_ref (the reference build) is absent')
def test_shift_folds_match_reference_signatures():
    from llmc_amd.compression.quantization import BaseBlockwiseQuantization as B
    want = _ref_methods(os.path.join(REF_DIR, 'base_blockwise_quantization.py'), 'BaseBlockwiseQuantization')
    for name in ('apply_shift', 'shift_fc_fc', 'shift_ln_fcs'):
        assert list(inspect.signature(getattr(B, name)).parameters) == want[name], name


def test_the_classes_carry_the_reference_method_names():
    """the same surface check from names written down here, for checkouts without oracle/_ref"""
    from llmc_amd.compression.quantization import BaseBlockwiseQuantization as B
    from llmc_amd.compression.quantization import OsPlus, SmoothQuant
    sig = lambda f: list(inspect.signature(f).parameters)         # noqa: E731
    assert sig(SmoothQuant.search_scale_subset) == ['self', 'layers', 'tensors']
    assert sig(SmoothQuant.get_weight_scale) == ['self', 'layers'] and sig(SmoothQuant.get_act_scale) == ['self', 'tensors']
    assert sig(SmoothQuant.filter_subset) == ['self', 'prev_op']
    assert sig(SmoothQuant.subset_transform) == ['self', 'subset', 'input_feat', 'subset_kwargs']
    assert sig(OsPlus.search_scale_shift_subset) == ['self', 'layers', 'input_feats', 'inspect_module', 'subset_kwargs']
    assert sig(OsPlus.get_original_out) == ['self', 'x', 'inspect_module', 'subset_kwargs']
    assert sig(OsPlus.subset_transform) == ['self', 'subset', 'input_feat', 'subset_kwargs']
    assert sig(B.apply_shift) == ['self', 'shifts', 'prev_op', 'layers']
    assert sig(B.shift_fc_fc) == ['self', 'fc1', 'fc2', 'shifts'] and sig(B.shift_ln_fcs) == ['self', 'ln', 'fcs', 'shifts']


# ---- the host threshold loop -----------------------------------------------------------------------------------------------
def _os_names():
    return [str(n) for n in _gold()['os_names']]


@pytest.mark.parametrize('name', _os_names())
def test_threshold_loop_reproduces_the_reference_list(name):
    from llmc_amd.compression.quantization import smooth_ops
    z = _gold()
    want = z[name + '/thresholds']
    got = smooth_ops.osplus_thresholds(float(z[name + '/amx']), float(z[name + '/amn']))
    assert len(got) == len(want) and len(want) >= 100
    assert np.array_equal(np.array(got, np.float64).view(np.uint64), want.view(np.uint64))
    # one upload of the whole list rounds every entry like the reference's torch.tensor(st, dtype=...) per point
    dt = DT[str(z[name + '/dt'])]
    whole = torch.tensor(got, dtype=dt)
    each = torch.stack([torch.tensor(s, dtype=dt) for s in got])
    assert torch.equal(whole, each)
    assert torch.equal(torch.tensor([-s for s in got], dtype=dt), -whole)         # min_range = tensor(-st) is the negation


def test_threshold_loop_edge_cases():
    from llmc_amd.compression.quantization import smooth_ops
    assert len(smooth_ops.osplus_thresholds(float('nan'), 0.0)) == 0              # `nan >= 1.0` is False: no point
    assert smooth_ops.osplus_thresholds(0.5, -0.25) == []                         # bounds[1] < 1: the loop never runs
    t = smooth_ops.osplus_thresholds(3.0, -400.0)                                 # the negative side sets the bound, amx the count
    assert t[0] == 400.0 and len(t) in (100, 101) and t[-1] >= 1.0


def test_golden_metadata():
    z = _gold()
    assert 'clone' in str(z['note']) and 'alias' in str(z['note'])
    clear = [n for n in _os_names() if int(z[n + '/clear'])]
    assert len(clear) >= 3
    for n in _os_names():
        loss = z[n + '/loss']
        assert len(loss) == len(z[n + '/thresholds'])
        win = int(z[n + '/win'])
        assert loss[win] == loss.min() and int(np.argmax(loss == loss.min())) == win       # the first minimum
    assert float(z['transform/before_after_maxabs']) < 0.01 * float(z['transform/out_absmax'])
