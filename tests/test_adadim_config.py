"""AdaDim without a GPU: registry, the shipped config on the toy adapter, the reference-named surface, the decision rule on
given loss tables, w_qdq's argument, the real-quant deploy refusal, and the column kernel's host-side argument checks."""
import ast
import inspect
import json
import os

import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = os.path.join(HERE, 'golden', 'ref_adadim_configs.json')
REF_DIR = os.path.join(os.path.dirname(HERE), 'oracle', '_ref', 'llmc', 'compression', 'quantization')
SHIPPED = 'methods/AdaDim/adadim_w_a.yml'


def _shipped():
    return json.load(open(CONFIGS))[SHIPPED]


def _construct(cfg):
    import llmc_amd.compression.quantization as Q
    from toy_model import ToyModel, calib_input
    q = cfg['quant']
    model = ToyModel()
    config = {'calib': cfg.get('calib') or {}, 'model': cfg.get('model') or {}, 'quant': q}
    return getattr(Q, q['method'])(model, dict(q), calib_input(model), None, config), model


def test_adadim_is_registered_exported_and_bound_by_name():
    import llmc_amd
    import llmc_amd.compression.quantization as Q
    from llmc_amd.utils.registry_factory import ALGO_REGISTRY
    assert ALGO_REGISTRY['AdaDim'] is Q.AdaDim
    reg = {}
    bound = llmc_amd.register_into(reg, names=('RTN', 'AdaDim'))
    assert reg['AdaDim'] is Q.AdaDim and bound['AdaDim'] is Q.AdaDim


def test_shipped_config_constructs_the_class():
    cfg = _shipped()
    assert cfg['quant']['method'] == 'AdaDim'
    algo, model = _construct(cfg)
    assert type(algo).__name__ == 'AdaDim'
    assert not algo.w_only and algo.quant_out
    assert algo.wquantizer.granularity == 'per_channel' and algo.wquantizer.bit == 8 and algo.wquantizer.sym
    assert algo.wquantizer.calib_algo == 'minmax'
    assert algo.aquantizer.granularity == 'per_token'
    assert algo.n_samples == 6 and algo.dim_losses == {}


def test_float_quant_is_refused_with_the_reason():
    cfg = _shipped()
    cfg['quant']['weight'] = dict(cfg['quant']['weight'], quant_type='float-quant', bit='e4m3', use_qtorch=True)
    with pytest.raises(NotImplementedError, match="ignores args\\['dim'\\]"):
        _construct(cfg)


def _ref_methods():
    tree = ast.parse(open(os.path.join(REF_DIR, 'adadim.py')).read())
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'AdaDim')
    return {m.name: [a.arg for a in m.args.posonlyargs + m.args.args] for m in node.body if isinstance(m, ast.FunctionDef)}


@pytest.mark.skipif(not os.path.isdir(REF_DIR), reason='oracle/_ref is built by __graft_entry__.build() where the reference exists')
def test_every_reference_method_exists_with_the_same_argument_names():
    import llmc_amd.compression.quantization as Q
    ref = _ref_methods()
    assert {'get_layer_out', 'search_dim_subset', 'block_transform', 'w_qdq'} <= set(ref)
    missing, diff = [], []
    for name, want in ref.items():
        if inspect.getattr_static(Q.AdaDim, name, None) is None:
            missing.append(name)
            continue
        if name == '__init__':       # the recorded exception: this package's (model, quant_config, input, padding_mask, config)
            continue
        mine = [p.name for p in inspect.signature(getattr(Q.AdaDim, name)).parameters.values()
                if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
        if mine[:len(want)] != want:
            diff.append((name, want, mine))
    assert not missing, missing
    assert not diff, diff
    assert list(inspect.signature(Q.AdaDim.__init__).parameters) == ['self', 'model', 'quant_config', 'input', 'padding_mask',
                                                                     'config']


def _bare(n_samples):
    import llmc_amd.compression.quantization as Q
    a = object.__new__(Q.AdaDim)
    a.n_samples = n_samples
    a.dim_losses = {}
    return a


@pytest.mark.parametrize('oc,ic,want', [
    ([4.0, 4.0], [1.0, 1.0], 0),                    # ic < oc
    ([2.0, 2.0], [2.0, 2.0], 1),                    # a tie goes to oc
    ([1.0, 1.0], [4.0, 4.0], 1),
    ([1.0, 1.0], [float('nan'), 0.0], 1),           # NaN compares false: oc
    ([float('nan'), 1.0], [0.5, 0.5], 1),
])
def test_decision_rule_on_given_loss_tables(monkeypatch, oc, ic, want):
    import llmc_amd.compression.quantization as Q
    a = _bare(2)
    layers = {'q': nn.Linear(8, 4, bias=False), 'k': nn.Linear(8, 4, bias=False)}
    monkeypatch.setattr(Q.AdaDim, 'layer_sample_means', lambda self, layer, input, xpacks: torch.tensor([oc, ic]))
    a.search_dim_subset(layers, [torch.zeros(1, 3, 8), torch.zeros(1, 3, 8)])
    for m in layers.values():                        # registered on every layer of the subset
        assert int(m.buf_qdim) == want and 'buf_qdim' in dict(m.named_buffers())
    assert set(a.dim_losses) == {'q', 'k'}


def test_sample_weight_is_rows_over_n_samples_per_sample(monkeypatch):
    import llmc_amd.compression.quantization as Q
    # batches of 1 and 3 rows, n_samples = 4: weights 0.25 and 0.75
    a = _bare(4)
    layer = nn.Linear(8, 4, bias=False)
    table = torch.tensor([[8.0, 1.0], [1.0, 3.0]], dtype=torch.float32)
    monkeypatch.setattr(Q.AdaDim, 'layer_sample_means', lambda self, layer, input, xpacks: table)
    a.search_dim_subset({'fc': layer}, [torch.zeros(1, 3, 8), torch.zeros(3, 3, 8)])
    loss_oc, loss_ic = a.dim_losses['fc']
    assert loss_oc == 0 + 1 / 4 * 8.0 + 3 / 4 * 1.0 and loss_ic == 0 + 1 / 4 * 1.0 + 3 / 4 * 3.0
    assert int(layer.buf_qdim) == 0                 # ic 2.5 < oc 2.75
    # a table whose decision flips with the weighting: equal weights give ic 2.0 < oc 2.5, the reference's give 2.5 vs 1.75
    table2 = torch.tensor([[4.0, 1.0], [1.0, 3.0]], dtype=torch.float32)
    monkeypatch.setattr(Q.AdaDim, 'layer_sample_means', lambda self, layer, input, xpacks: table2)
    a.search_dim_subset({'fc': layer}, [torch.zeros(1, 3, 8), torch.zeros(3, 3, 8)])
    assert a.dim_losses['fc'] == (1.75, 2.5) and int(layer.buf_qdim) == 1


class _Recorder:
    def __init__(self):
        self.calls = []

    def fake_quant_weight_dynamic(self, weight, args={}):
        self.calls.append((weight, dict(args)))
        return weight


@pytest.mark.parametrize('qdim,dim', [(0, 'ic'), (1, 'oc')])
def test_w_qdq_passes_the_axis_of_buf_qdim(qdim, dim):
    a = _bare(1)
    m = nn.Linear(8, 4, bias=False)
    m.register_buffer('buf_qdim', torch.tensor(qdim))
    rec = _Recorder()
    out = a.w_qdq(m, rec)
    assert out is m.weight and len(rec.calls) == 1
    assert rec.calls[0][0] is m.weight and rec.calls[0][1] == {'dim': dim}


def test_real_quant_deploy_with_an_ic_layer_raises():
    from toy_model import ToyModel
    from llmc_amd.compression.quantization.module_utils import _REALQUANT_LINEAR_MAP_
    a = _bare(1)
    a.model = ToyModel()
    for b in a.model.get_blocks():
        for m in a.model.get_block_linears(b).values():
            m.register_buffer('buf_qdim', torch.tensor(1))
    a.model.get_blocks()[1].up_proj.buf_qdim = torch.tensor(0)
    fmt = sorted(_REALQUANT_LINEAR_MAP_)[0]
    with pytest.raises(NotImplementedError, match='per-input-channel'):
        a.deploy(fmt)


def test_quantizer_route_conditions():
    """which calls go to the column kernel: a pure host decision"""
    from llmc_amd import _ffi
    from llmc_amd.compression.quantization import IntegerQuantizer
    w = torch.zeros(96, 128)
    assert IntegerQuantizer(8, True, 'per_channel')._cols_group(w) == 96
    assert IntegerQuantizer(4, False, 'per_group', group_size=32)._cols_group(w) == 32
    assert IntegerQuantizer(4, False, 'per_group', group_size=128)._cols_group(w) == 96      # a short axis stays whole
    assert IntegerQuantizer(4, False, 'per_group', group_size=64)._cols_group(w) is None     # 96 % 64: the old route raises
    assert IntegerQuantizer(8, True, 'per_tensor')._cols_group(w) is None
    assert IntegerQuantizer(8, True, 'per_channel')._cols_group(torch.zeros(96)) is None
    for algo in ('mse', 'learnable'):
        assert IntegerQuantizer(8, True, 'per_channel', calib_algo=algo)._cols_group(w) is None
    assert IntegerQuantizer(4, False, 'per_group', group_size=32, calib_algo='hqq')._cols_group(w) is None
    assert _ffi.HOST_OPTIONS['quant_cols'] == 1
    with _ffi.option(quant_cols=0):
        assert IntegerQuantizer(8, True, 'per_channel')._cols_group(w) is None


def test_entry_point_argument_checks():
    """Argument checks and the plan only: nothing reaches a GPU."""
    from llmc_amd import _ffi
    from llmc_amd.compression.quantization import quant_cols_ops
    L = _ffi.lib()
    one = 16       # a non-null, 16-byte aligned stand-in pointer; the calls return before touching it
    assert L.llmc_quant_dynamic_cols_paths() >= 3
    # the plan: tile for short groups, slabs for long columns, scalar where 16-byte vectors do not fit
    assert L.llmc_quant_dynamic_cols_path(one, _ffi.BF16, 384, 4096, 4096, 128) == 0
    assert L.llmc_quant_dynamic_cols_path(one, _ffi.BF16, 4096, 4096, 4096, 4096) == 1
    assert L.llmc_quant_dynamic_cols_path(one + 2, _ffi.BF16, 384, 4096, 4096, 128) == 2          # base off by one element
    assert L.llmc_quant_dynamic_cols_path(one, _ffi.BF16, 384, 4093, 4096, 128) == 2              # ragged vector tail
    assert L.llmc_quant_dynamic_cols_path(one, _ffi.F32, 384, 4096, 4098, 128) == 2               # ld off the vector grid
    assert L.llmc_quant_dynamic_cols_path(one, _ffi.F32, 384, 4096, 4100, 128) == 0
    # workspace: none for the tile path, per-slab and folded fp32 min / max otherwise
    assert L.llmc_quant_dynamic_cols_ws_bytes(384, 4096, 128) == 0
    R = 2 * quant_cols_ops.SLAB_ROWS + 5 + quant_cols_ops.TILE_MAX_G
    assert L.llmc_quant_dynamic_cols_ws_bytes(R, 24, R) == (-(-R // quant_cols_ops.SLAB_ROWS) + 1) * 24 * 8
    assert L.llmc_quant_dynamic_cols_ws_bytes(100, 24, 7) == 0                                    # g does not divide R

    def path(dt=_ffi.F16, R=96, K=128, ld=128, g=32, W=one):
        return L.llmc_quant_dynamic_cols_path(W, dt, R, K, ld, g)

    def call(dt=_ffi.F16, R=96, K=128, ld=128, g=32, W=one, out=one + 4096 * 64, kind=_ffi.OUT_FAKE, ws=None):
        return L.llmc_quant_dynamic_cols(W, dt, R, K, ld, g, 1, 1, -128.0, 127.0, kind, out, None, None, ws, None)
    for fn in (path, call):
        assert fn(g=36) == -22 and 'divide' in _ffi.last_error()
        assert fn(ld=120) == -22 and 'ld' in _ffi.last_error()
        assert fn(dt=9) == -22 and 'dtype' in _ffi.last_error()
        assert fn(W=None) == -22 and 'null' in _ffi.last_error()
        assert fn(g=0) == -22
    assert call(out=None) == -22 and 'null' in _ffi.last_error()
    assert call(out=one) == -22 and 'overlap' in _ffi.last_error()
    assert call(out=one + 4096 * 64 + 2) == -22 and 'aligned' in _ffi.last_error()
    assert call(kind=7) == -22 and 'out_kind' in _ffi.last_error()
    assert call(R=1024, g=1024, out=one + (1 << 24)) == -22 and 'workspace' in _ffi.last_error()
