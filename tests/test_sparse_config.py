"""Sparsification without a GPU: registry, the two shipped configs on the toy adapter, the config keys, the reference-named
surface, and the pruning kernels' host-side queries and argument checks (everything that must return before a launch)."""
import ast
import inspect
import json
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = os.path.join(HERE, 'golden', 'ref_sparse_configs.json')
REF_DIR = os.path.join(os.path.dirname(HERE), 'oracle', '_ref', 'llmc', 'compression', 'sparsification')

EINVAL, ENOTSUP = -22, -95


def _shipped(rel):
    return json.load(open(CONFIGS))[rel]


def _construct(cfg, with_input=True):
    import llmc_amd.compression.sparsification as S
    from toy_model import ToyModel, calib_input
    s = cfg['sparse']
    model = ToyModel()
    config = {'calib': cfg.get('calib') or {}, 'sparse': s}
    return getattr(S, s['method'])(model, dict(s), calib_input(model) if with_input else None, None, config), model


def test_both_methods_are_registered_exported_and_bound_by_name():
    import llmc_amd
    import llmc_amd.compression.quantization as Q
    import llmc_amd.compression.sparsification as S
    from llmc_amd.utils.registry_factory import ALGO_REGISTRY
    assert ALGO_REGISTRY['Wanda'] is S.Wanda and ALGO_REGISTRY['Magnitude'] is S.Magnitude
    reg = {}
    bound = llmc_amd.register_into(reg, names=('GPTQ', 'Wanda', 'Magnitude'))
    assert reg['Wanda'] is S.Wanda and reg['Magnitude'] is S.Magnitude and reg['GPTQ'] is Q.GPTQ and set(bound) == set(reg)
    assert set(llmc_amd.register_into({})) == {'GPTQ', 'Awq', 'RTN', 'SpQR'}          # the default tuple is unchanged
    with pytest.raises(AttributeError):
        llmc_amd.register_into({}, names=('NoSuchMethod',))


def test_shipped_wanda_config_constructs_the_class():
    cfg = _shipped('Wanda/wanda.yml')
    assert cfg['sparse'] == {'method': 'Wanda', 'weight': {'sparsity': 0.5}, 'sparsity_out': False} and cfg['calib']['bs'] == -1
    algo, _ = _construct(cfg)
    assert type(algo).__name__ == 'Wanda'
    assert algo.sparsity == 0.5 and algo.sparser.sparsity == 0.5 and algo.sparsity_out is False and algo.nm is None
    assert algo.W_mask is None and algo.sparse_kvcache is False and algo.n_samples == 6 and not algo.data_free
    assert algo.sparsity_config is algo.quant_config


def test_shipped_magnitude_config_constructs_the_class_with_and_without_data():
    cfg = _shipped('Magnitude/magnitude.yml')
    assert cfg['sparse'] == {'method': 'Magnitude', 'weight': {'sparsity': 0.5}}
    algo, _ = _construct(cfg)
    assert type(algo).__name__ == 'Magnitude' and algo.sparsity == 0.5 and algo.sparsity_out is False
    free, _ = _construct(cfg, with_input=False)
    assert free.data_free and free.needs_input_feat is False


def test_wanda_needs_calibration_data():
    with pytest.raises(ValueError, match='calibration'):
        _construct(_shipped('Wanda/wanda.yml'), with_input=False)


def test_sparsity_type_n_m():
    cfg = _shipped('Wanda/wanda.yml')
    cfg['sparse']['weight'] = {'sparsity_type': '2:4'}
    algo, _ = _construct(cfg)
    assert algo.nm == (2, 4) and algo.sparsity == 0.5 and algo.sparser.sparsity == 0.5
    cfg['sparse']['weight'] = {'sparsity_type': '2:4', 'sparsity': 0.5}
    assert _construct(cfg)[0].nm == (2, 4)
    cfg['sparse']['weight'] = {'sparsity_type': 'unstructured', 'sparsity': 0.3}
    algo, _ = _construct(cfg)
    assert algo.nm is None and algo.sparsity == 0.3
    cfg['sparse']['weight'] = {'sparsity_type': '2:4', 'sparsity': 0.3}
    with pytest.raises(ValueError, match='contradicts'):
        _construct(cfg)
    for bad in ('2:3', '5:4', 'two:four', '2-4'):
        cfg['sparse']['weight'] = {'sparsity_type': bad}
        with pytest.raises(ValueError):
            _construct(cfg)
    cfg = _shipped('Magnitude/magnitude.yml')
    cfg['sparse']['weight'] = {'sparsity_type': '2:4'}
    with pytest.raises(NotImplementedError):
        _construct(cfg)


def test_kvcache_and_replace_attention_raise_with_a_reason():
    cfg = _shipped('Wanda/wanda.yml')
    cfg['sparse']['kvcache'] = {'method': 'SinkKV', 'window_length': 256, 'num_sink_tokens': 4}
    with pytest.raises(NotImplementedError, match='KV-cache'):
        _construct(cfg)
    algo, model = _construct(_shipped('Wanda/wanda.yml'))
    with pytest.raises(NotImplementedError, match='KV-sparse'):
        algo.replace_attention(model.get_blocks()[0])


def test_n_prune_layers_is_read():
    import llmc_amd.compression.sparsification as S
    from toy_model import ToyModel

    class Probe(S.BaseBlockwiseSparsification):
        def subset_transform(self, subset, input_feat, subset_kwargs):
            pass
    algo = Probe(ToyModel(), {'weight': {'n_prune_layers': 3}, 'sparsity_out': True}, None, None, {})
    assert algo.n_prune_layers == 3 and algo.sparsity_out is True and not hasattr(algo, 'sparser')


def test_a_subclass_written_against_the_reference_attribute_works():
    """self.sparser.sparsity is what the reference's subset_transforms read (wanda.py:54, magnitude.py:28)"""
    import llmc_amd.compression.sparsification as S
    from toy_model import ToyModel
    seen = []

    class Mine(S.BaseBlockwiseSparsification):
        def subset_transform(self, subset, input_feat, subset_kwargs):
            seen.append((sorted(subset['layers']), self.sparser.sparsity, subset_kwargs))
    model = ToyModel()
    algo = Mine(model, {'weight': {'sparsity': 0.25}}, None, None, {})
    algo.block_idx = 0
    algo.block_transform(model.get_blocks()[0], {}, [])          # the protocol: (subset, input_feat, subset_kwargs)
    assert seen == [(['gate_proj', 'up_proj'], 0.25, {}), (['down_proj'], 0.25, {})]


# ---- the reference's method names --------------------------------------------------------------------------------------------
# the KV-sparse caches are out of scope (their entry points raise); these helpers exist only to build them
OUT_OF_SCOPE = {'set_kv_sparse_config', 'set_cos_sin_cache', 'register_kv_cache'}


def _ref_methods(fname, cls):
    tree = ast.parse(open(os.path.join(REF_DIR, fname)).read())
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    return {m.name: [a.arg for a in m.args.posonlyargs + m.args.args] for m in node.body if isinstance(m, ast.FunctionDef)}


@pytest.mark.skipif(not os.path.isdir(REF_DIR), reason='oracle/_ref is built by __graft_entry__.build() where the reference exists')
@pytest.mark.parametrize('fname,cls', [('base_blockwise_sparsification.py', 'BaseBlockwiseSparsification'), ('wanda.py', 'Wanda'),
                                       ('magnitude.py', 'Magnitude')])
def test_every_reference_method_exists_with_the_same_argument_names(fname, cls):
    import llmc_amd.compression.sparsification as S
    ours = getattr(S, cls)
    ref = _ref_methods(fname, cls)
    assert ref
    missing, diff = [], []
    for name, want in ref.items():
        if name in OUT_OF_SCOPE:
            continue
        if inspect.getattr_static(ours, name, None) is None:
            missing.append(name)
            continue
        mine = [p.name for p in inspect.signature(getattr(ours, name)).parameters.values()
                if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
        if mine[:len(want)] != want:
            diff.append((name, want, mine))
    assert not missing, missing
    assert not diff, diff


# ---- host-side queries and argument checks of csrc/prune.hip: none of these touches a GPU ----------------------------------------
def _lib():
    from llmc_amd import _ffi
    return _ffi, _ffi.lib()


def test_workspace_queries_are_pure_host_calls():
    _ffi, L = _lib()
    assert L.llmc_col_sqsum_ws_bytes(2048, 4096, _ffi.BF16) == 32 * 4096 * 4          # 32 row chunks of 64 rows
    assert L.llmc_col_sqsum_ws_bytes(1, 8, _ffi.F32) == 8 * 4
    assert L.llmc_col_sqsum_ws_bytes(0, 8, _ffi.F32) == 0 and L.llmc_col_sqsum_ws_bytes(8, 8, 7) == 0
    ws = L.llmc_magnitude_prune_ws_bytes(_ffi.BF16, 4096, 4096)
    assert ws >= 32768 * 4 and ws == L.llmc_magnitude_prune_ws_bytes(_ffi.F32, 64, 250)          # does not grow with R * K
    assert L.llmc_magnitude_prune_ws_bytes(7, 4, 4) == 0 and L.llmc_magnitude_prune_ws_bytes(_ffi.F16, 0, 4) == 0


def test_prune_rows_path_is_a_pure_host_call():
    _ffi, L = _lib()
    from llmc_amd.compression.sparsification.sparse_ops import PATH_NAMES
    assert L.llmc_prune_rows_paths() == len(PATH_NAMES) == 6
    A = 0x10000          # a 16-byte aligned address; the query does not read it

    def p(dt, R, K, ld, m, W=A):
        return L.llmc_prune_rows_path(dt, R, K, ld, m, W)
    name = lambda *a, **k: PATH_NAMES[p(*a, **k)]          # noqa: E731
    assert name(_ffi.BF16, 5, 64, 64, 64) == 'wave' and name(_ffi.BF16, 5, 2048, 2048, 2048) == 'wave'
    assert name(_ffi.F32, 5, 1024, 1024, 1024) == 'wave' and name(_ffi.F32, 5, 1028, 1028, 1028) == 'block256'
    assert name(_ffi.BF16, 5, 4096, 4096, 4096) == 'block256' and name(_ffi.F16, 5, 8192, 8192, 8192) == 'block256'
    assert name(_ffi.BF16, 5, 14336, 14336, 14336) == 'block1024' and name(_ffi.F32, 5, 28672, 28672, 28672) == 'block1024'
    assert name(_ffi.BF16, 5, 32768, 32768, 32768) == 'block1024'
    assert name(_ffi.BF16, 5, 250, 250, 250) == 'scalar' and name(_ffi.BF16, 5, 250, 256, 250) == 'scalar'
    assert name(_ffi.BF16, 5, 256, 260, 256) == 'scalar' and name(_ffi.BF16, 5, 256, 256, 256, A + 2) == 'scalar'
    assert name(_ffi.BF16, 5, 256, 256, 4) == 'nm' and name(_ffi.F32, 5, 4100, 4100, 2) == 'nm'
    assert name(_ffi.BF16, 5, 4100, 4100, 4) == 'nm_scalar' and name(_ffi.F32, 5, 256, 256, 16, A + 4) == 'nm_scalar'
    assert p(_ffi.BF16, 5, 32776, 32776, 32776) == ENOTSUP and 'resident' in _ffi.last_error()
    assert p(_ffi.BF16, 5, 65536, 65536, 4) == PATH_NAMES.index('nm')          # n:m has no width limit


def test_invalid_prune_rows_calls_return_before_touching_the_gpu():
    _ffi, L = _lib()
    A = 0x10000
    call = lambda W, dt, R, K, ld, n, m: L.llmc_prune_rows(W, dt, R, K, ld, None, n, m, None, None)          # noqa: E731
    assert call(A, 7, 4, 64, 64, 1, 64) == EINVAL and 'dtype' in _ffi.last_error()
    assert call(None, _ffi.BF16, 4, 64, 64, 1, 64) == EINVAL and 'null W' in _ffi.last_error()
    assert call(A, _ffi.BF16, 4, 64, 63, 1, 64) == EINVAL and 'ld < K' in _ffi.last_error()
    assert call(A, _ffi.BF16, 4, 66, 66, 1, 4) == EINVAL and 'divide' in _ffi.last_error()
    assert call(A, _ffi.BF16, 4, 64, 64, 1, 32) == ENOTSUP and 'n:m' in _ffi.last_error()
    assert call(A, _ffi.BF16, 4, 63, 63, 1, 3) == ENOTSUP
    assert call(A, _ffi.BF16, 4, 64, 64, -1, 64) == EINVAL and 'n_prune' in _ffi.last_error()
    assert call(A, _ffi.BF16, 4, 64, 64, 65, 64) == EINVAL
    assert call(A, _ffi.BF16, 4, 64, 64, 5, 4) == EINVAL
    assert call(A, _ffi.BF16, 0, 64, 64, 1, 64) == EINVAL
    assert call(A, _ffi.F32, 4, 40000, 40000, 1, 40000) == ENOTSUP and 'resident' in _ffi.last_error()
    assert L.llmc_prune_rows_path(7, 4, 64, 64, 64, A) == EINVAL and L.llmc_prune_rows_path(_ffi.BF16, 4, 64, 64, 64, None) == EINVAL


def test_invalid_magnitude_and_col_sqsum_calls_return_before_touching_the_gpu():
    _ffi, L = _lib()
    A = 0x10000
    mag = lambda W, dt, R, K, ld, kth, ws: L.llmc_magnitude_prune(W, dt, R, K, ld, kth, None, None, ws, None)          # noqa: E731
    assert mag(A, 7, 4, 64, 64, 0, A) == EINVAL and 'dtype' in _ffi.last_error()
    assert mag(None, _ffi.F16, 4, 64, 64, 0, A) == EINVAL and 'null W' in _ffi.last_error()
    assert mag(A, _ffi.F16, 4, 64, 60, 0, A) == EINVAL and 'ld < K' in _ffi.last_error()
    assert mag(A, _ffi.F16, 4, 64, 64, -1, A) == EINVAL and 'kth' in _ffi.last_error()
    assert mag(A, _ffi.F16, 4, 64, 64, 256, A) == EINVAL and 'kth' in _ffi.last_error()          # sparsity 1.0
    assert mag(A, _ffi.F16, 4, 64, 64, 0, None) == EINVAL and 'workspace' in _ffi.last_error()
    sq = lambda X, dt, N, K, acc, ws: L.llmc_col_sqsum(X, dt, N, K, 1, acc, None, 1, ws, None)          # noqa: E731
    assert sq(A, 7, 4, 64, A, A) == EINVAL and 'dtype' in _ffi.last_error()
    assert sq(None, _ffi.F32, 4, 64, A, A) == EINVAL and sq(A, _ffi.F32, 4, 64, None, A) == EINVAL
    assert sq(A, _ffi.F32, 0, 64, A, A) == EINVAL
    assert sq(A, _ffi.F32, 4, 64, A, None) == EINVAL and 'workspace' in _ffi.last_error()
    assert L.llmc_col_sqsum(A, _ffi.F32, 4, 64, 1, A, A, 0, A, None) == EINVAL and 'nsamples' in _ffi.last_error()


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from llmc_amd import _ffi
    from llmc_amd.compression.sparsification import sparse_ops
    w = torch.zeros(4, 64)
    for call in (lambda: sparse_ops.prune_rows(w, None, 1), lambda: sparse_ops.prune_rows_composed(w, None, 1),
                 lambda: sparse_ops.magnitude_prune(w, 0), lambda: sparse_ops.col_sqsum(w)):
        with pytest.raises(_ffi.LlmcHipError):
            call()
    assert sparse_ops.path(w) == 'wave' and sparse_ops.path(w, 4) == 'nm'          # path() is a host query: no GPU needed
    assert sparse_ops.path(torch.zeros(2, 40000)) == 'composed'
    with pytest.raises(ValueError):
        sparse_ops.path(torch.zeros(4))
    with pytest.raises(ValueError):
        sparse_ops.path(torch.zeros(4, 66), 4)
    with pytest.raises(NotImplementedError):
        sparse_ops.path(torch.zeros(4, 64), 32)
