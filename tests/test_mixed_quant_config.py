"""QUIK and LLM.int8() without a GPU: registry, reference-named surface, QUIK's index choice (golden, ties, no outliers,
fp_relative, last_fc_bit), the quantizer's argument checks, the shipped configs, and the entry point's own argument checks."""
import ast
import inspect
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden', 'mixed_quant.npz')
CONFIGS = os.path.join(HERE, 'golden', 'ref_mixed_configs.json')
REF_DIR = os.path.join(os.path.dirname(HERE), 'oracle', '_ref', 'llmc', 'compression', 'quantization')


def _shipped(rel):
    return json.load(open(CONFIGS))[rel]


def _construct(cfg, monkeypatch=None, scales=None):
    """the class named by the config on the toy adapter; QUIK's calibration forward (GPU) is replaced by a given table"""
    import llmc_amd.compression.quantization as Q
    from toy_model import ToyModel, calib_input
    q = cfg['quant']
    model = ToyModel()
    config = {'calib': cfg.get('calib') or {}, 'model': cfg.get('model') or {}, 'quant': q}
    if q['method'] == 'QUIK':
        monkeypatch.setattr(Q.QUIK, 'get_act_scale_shift', lambda self, stat='scales': dict(scales or {}))
    return getattr(Q, q['method'])(model, dict(q), calib_input(model), None, config), model


def test_both_methods_are_registered_and_exported():
    import llmc_amd.compression.quantization as Q
    from llmc_amd.utils.registry_factory import ALGO_REGISTRY
    assert ALGO_REGISTRY['QUIK'] is Q.QUIK
    assert ALGO_REGISTRY['LlmInt8'] is Q.LlmInt8


def _ref_methods(fname, cls):
    tree = ast.parse(open(os.path.join(REF_DIR, fname)).read())
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    return {m.name: [a.arg for a in m.args.posonlyargs + m.args.args] for m in node.body if isinstance(m, ast.FunctionDef)}


@pytest.mark.skipif(not os.path.isdir(REF_DIR), reason='oracle/_ref is built by __graft_entry__.build() where the reference exists')
@pytest.mark.parametrize('fname,cls', [('quik.py', 'QUIK'), ('llmint8.py', 'LlmInt8')])
def test_every_reference_method_exists_with_the_same_argument_names(fname, cls):
    import llmc_amd.compression.quantization as Q
    ours = getattr(Q, cls)
    missing, diff = [], []
    for name, want in _ref_methods(fname, cls).items():
        if inspect.getattr_static(ours, name, None) is None:
            missing.append(name)
            continue
        mine = [p.name for p in inspect.signature(getattr(ours, name)).parameters.values()
                if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
        if mine[:len(want)] != want:
            diff.append((name, want, mine))
    assert not missing, missing
    assert not diff, diff
    # a_qdq keeps the base protocol's trailing input_index=0
    assert inspect.signature(ours.a_qdq).parameters['input_index'].default == 0


def _block(K, names=('q_proj', 'down_proj')):
    block = nn.Module()
    for n in names:
        setattr(block, n, nn.Linear(K, 8, bias=False))
    return block


def _quik(scales, fp_features, fp_threshold=0.0, fp_relative=False, hidden_size=None, last_fc_bit=None):
    import llmc_amd.compression.quantization as Q
    from toy_model import ToyModel
    q = object.__new__(Q.QUIK)
    q.model = ToyModel.__new__(ToyModel)
    q.prefix, q.block_idx = 'blocks', 0
    q.fp_relative, q.fp_features, q.fp_threshold = fp_relative, fp_features, fp_threshold
    q.hidden_size = hidden_size
    if last_fc_bit is not None:
        q.last_fc_bit = last_fc_bit
    q.act_scales = dict(scales)
    return q


def test_quik_index_choice_equals_the_reference():
    g = np.load(GOLD)
    block = _block(40)
    scales = {f'blocks.0.{n}': torch.from_numpy(g[f'quik/{n}/scales']) for n in ('q_proj', 'down_proj')}
    q = _quik(scales, fp_features=4)
    q.block_opt(block)
    for n in ('q_proj', 'down_proj'):
        m = getattr(block, n)
        assert m.buf_int_ids.tolist() == g[f'quik/{n}/int_ids'].tolist()
        assert m.buf_fp_ids.tolist() == g[f'quik/{n}/fp_ids'].tolist()
        assert not hasattr(m, 'buf_current_bit')
    assert q.act_scales == {}


def test_quik_ties_follow_the_stable_order():
    K = 64
    s = torch.tensor([float(i % 4) for i in range(K)])         # sixteen-fold ties
    block = _block(K, ('q_proj',))
    q = _quik({'blocks.0.q_proj': s}, fp_features=10)
    q.block_opt(block)
    order = torch.sort(s, stable=True)[1]
    assert torch.equal(block.q_proj.buf_int_ids, order[:K - 10])
    assert torch.equal(block.q_proj.buf_fp_ids, order[K - 10:])
    # ascending scale, then ascending column
    key = [(float(s[i]), int(i)) for i in torch.cat([block.q_proj.buf_int_ids, block.q_proj.buf_fp_ids])]
    assert key == sorted(key)


@pytest.mark.parametrize('fp_features,fp_threshold', [(0, 0.0), (4, 100.0)])
def test_quik_without_outliers_quantizes_every_column(fp_features, fp_threshold):
    K = 40
    block = _block(K, ('q_proj',))
    q = _quik({'blocks.0.q_proj': torch.rand(K) + 0.5}, fp_features=fp_features, fp_threshold=fp_threshold)
    q.block_opt(block)
    assert block.q_proj.buf_int_ids.tolist() == list(range(K))
    assert block.q_proj.buf_fp_ids.numel() == 0 and block.q_proj.buf_fp_ids.dtype == torch.long


def test_quik_fp_relative_reads_the_linears_own_width():
    hidden = 16
    block = nn.Module()
    block.q_proj = nn.Linear(hidden, 8, bias=False)
    block.down_proj = nn.Linear(3 * hidden, 8, bias=False)
    scales = {'blocks.0.q_proj': torch.rand(hidden) + 0.5, 'blocks.0.down_proj': torch.rand(3 * hidden) + 0.5}
    q = _quik(scales, fp_features=2, fp_relative=True, hidden_size=hidden)
    q.block_opt(block)
    assert block.q_proj.buf_fp_ids.numel() == 2
    assert block.down_proj.buf_fp_ids.numel() == 6 and block.down_proj.buf_int_ids.numel() == 3 * hidden - 6


def test_quik_last_fc_bit_marks_down_proj_and_doubles_its_threshold():
    K = 40
    s = torch.rand(K) + 0.5                                    # max in (0.5, 1.5)
    block = _block(K)
    q = _quik({'blocks.0.q_proj': s.clone(), 'blocks.0.down_proj': s.clone()}, fp_features=4,
              fp_threshold=float(s.max()) * 0.75, last_fc_bit=8)
    q.block_opt(block)
    assert block.q_proj.buf_fp_ids.numel() == 4 and not hasattr(block.q_proj, 'buf_current_bit')
    assert block.down_proj.buf_fp_ids.numel() == 0             # max <= 2 * threshold
    assert int(block.down_proj.buf_current_bit) == 8
    args = q._mixed_args(block.down_proj)
    assert int(args['current_bit']) == 8 and args['int_indices'] is block.down_proj.buf_int_ids


def test_quantizer_refuses_ragged_groups_empty_lists_and_unreached_paths():
    from llmc_amd.compression.quantization import FloatQuantizer, IntegerQuantizer
    w = torch.zeros(4, 48)
    pg = IntegerQuantizer(4, False, 'per_group', group_size=16)
    with pytest.raises(ValueError, match='group size'):
        pg.fake_quant_weight_dynamic(w, {'int_indices': torch.arange(40), 'fp_indices': torch.arange(40, 48)})
    with pytest.raises(ValueError, match='group size'):
        pg.fake_quant_act_dynamic(w[None], {'int_indices': torch.arange(40), 'fp_indices': torch.arange(40, 48)})
    pt = IntegerQuantizer(8, True, 'per_token')
    empty = torch.empty(0, dtype=torch.long)
    with pytest.raises(ValueError, match='empty'):
        pt.fake_quant_act_dynamic(w[None], {'int_indices': empty, 'fp_indices': torch.arange(48)})
    with pytest.raises(ValueError, match='empty'):
        pt.fake_quant_weight_dynamic(w, {'int_indices': empty, 'fp_indices': torch.arange(48)})
    for algo in ('mse', 'hqq', 'learnable'):
        q = IntegerQuantizer(4, False, 'per_group', group_size=16, calib_algo=algo)
        with pytest.raises(NotImplementedError):
            q.fake_quant_weight_dynamic(w, {'int_indices': torch.arange(32), 'fp_indices': torch.arange(32, 48)})
    with pytest.raises(NotImplementedError):
        pt.fake_quant_weight_static(w, {'int_indices': torch.arange(32), 'fp_indices': torch.arange(32, 48)})
    with pytest.raises(NotImplementedError):
        pt.fake_quant_act_static(w[None], {'int_indices': torch.arange(32), 'fp_indices': torch.arange(32, 48)})
    # the float quantizer has no mixed path in the reference either: its methods do not read the keys
    assert 'int_indices' not in inspect.getsource(FloatQuantizer)


def test_mixed_ops_refuses_what_is_free_to_check():
    from llmc_amd.compression.quantization import mixed_ops
    x = torch.zeros(2, 8)
    with pytest.raises(ValueError, match='duplicates'):
        mixed_ops._check(x, torch.zeros(9, dtype=torch.long), 9)
    with pytest.raises(ValueError, match='groups'):
        mixed_ops._check(x, torch.arange(6), 4)
    with pytest.raises(ValueError, match='empty'):
        mixed_ops._check(x, torch.empty(0, dtype=torch.long), 1)
    role = mixed_ops.make_roles(8, torch.tensor([5, 0, 3]), torch.tensor([3, 7]), 'cpu')
    assert role.tolist() == [1, 0, 0, 3, 0, 1, 0, 2]          # 3: named in both lists


def test_entry_point_argument_checks():
    """Argument checks only: nothing reaches a GPU."""
    from llmc_amd import _ffi
    L = _ffi.lib()
    one = 1        # a non-null stand-in pointer; the calls return before touching it
    assert L.llmc_quant_dynamic_mixed_fits(_ffi.BF16, 28672) == 1 and L.llmc_quant_dynamic_mixed_fits(_ffi.F16, 4096) == 1
    assert L.llmc_quant_dynamic_mixed_fits(_ffi.F32, 14336) == 1
    assert L.llmc_quant_dynamic_mixed_fits(_ffi.F32, 1 << 16) == 0 and L.llmc_quant_dynamic_mixed_fits(_ffi.BF16, 1 << 17) == 0
    assert L.llmc_quant_dynamic_mixed_fits(7, 64) == 0 and L.llmc_quant_dynamic_mixed_fits(_ffi.F16, 0) == 0

    def call(K=64, n_int=32, g=16, idx=one, dt=_ffi.F16):
        return L.llmc_quant_dynamic_mixed(one, dt, 4, K, one, idx, n_int, g, 1, 1, -128.0, 127.0, one, None)
    assert call(n_int=40) == -22                   # ragged groups
    assert call(n_int=0, g=16) == -22              # nothing to quantize
    assert call(n_int=-16) == -22
    assert call(n_int=128, g=16) == -22            # more integer columns than columns
    assert call(idx=None) == -22                   # several groups per row need the order
    assert call(dt=9) == -22
    assert call(K=1 << 17, n_int=1 << 16, g=1 << 16, idx=None) == -95       # the row does not fit: callers compose
    assert 'LDS' in _ffi.last_error()


@pytest.mark.parametrize('rel,cls', [('methods/QUIK/quik_w_a.yml', 'QUIK'), ('methods/LlmInt8/llmint8_w_only.yml', 'LlmInt8')])
def test_shipped_configs_parse_into_the_classes_attributes(rel, cls, monkeypatch):
    cfg = _shipped(rel)
    special = cfg['quant']['special']
    algo, model = _construct(cfg, monkeypatch, scales={'blocks.0.gate_proj': torch.ones(256)})
    assert type(algo).__name__ == cls == cfg['quant']['method']
    assert not algo.w_only and algo.wquantizer.granularity == 'per_channel' and algo.aquantizer.granularity == 'per_token'
    assert algo.wquantizer.bit == algo.aquantizer.bit == 8 and algo.wquantizer.sym and algo.aquantizer.sym
    if cls == 'QUIK':
        assert (algo.fp_relative, algo.fp_features, algo.fp_threshold) == (special['fp_relative'], special['fp_features'],
                                                                           special['fp_threshold'])
        assert algo.last_fc_bit == special['last_fc_bit'] == 8          # read from `special`, where the config has it
        assert algo.prefix == model.block_name_prefix and set(algo.act_scales) == {'blocks.0.gate_proj'}
    else:
        assert algo.threshold == special['threshold'] == 6.0
        assert algo.block_opt(model.get_blocks()[0]) is None
        with pytest.raises(NotImplementedError, match='fake_quant'):
            algo.deploy('vllm_quant')
