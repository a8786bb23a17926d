"""SparseGPT without a GPU, in the manner of tests/test_sparse_config.py: registry, construction on the toy adapter from an inline
config, the config keys, and the column loop's host-side query and argument checks (everything that returns before a launch)."""
import pytest
import torch

EINVAL, ENOTSUP = -22, -95


def _construct(sparse, with_input=True):
    import llmc_amd.compression.sparsification as S
    from toy_model import ToyModel, calib_input
    model = ToyModel()
    s = dict(sparse, method='SparseGPT')
    return S.SparseGPT(model, dict(s), calib_input(model) if with_input else None, None, {'sparse': s}), model


def test_registered_exported_and_bound_by_name():
    import llmc_amd
    import llmc_amd.compression.sparsification as S
    from llmc_amd.utils.registry_factory import ALGO_REGISTRY
    assert ALGO_REGISTRY['SparseGPT'] is S.SparseGPT and issubclass(S.SparseGPT, S.BaseBlockwiseSparsification)
    reg = {}
    bound = llmc_amd.register_into(reg, names=('SparseGPT', 'Wanda'))
    assert reg['SparseGPT'] is S.SparseGPT and set(bound) == {'SparseGPT', 'Wanda'}
    assert set(llmc_amd.register_into({})) == {'GPTQ', 'Awq', 'RTN', 'SpQR'}          # the default tuple is unchanged


def test_construction_from_an_inline_config():
    algo, model = _construct({'weight': {'sparsity': 0.5}, 'sparsity_out': True})
    assert type(algo).__name__ == 'SparseGPT' and algo.sparsity == 0.5 and algo.sparser.sparsity == 0.5 and algo.nm is None
    assert algo.percdamp == 0.01 and algo.blocksize == 128 and algo.sparsity_out is True and not algo.data_free
    assert algo.needs_input_feat is True and algo.n_samples == 6
    algo, _ = _construct({'weight': {'sparsity': 0.3}, 'special': {'percdamp': 0.1, 'blocksize': 128}})
    assert algo.percdamp == 0.1 and algo.sparsity_out is False
    algo.block_init(model.get_blocks()[0])
    assert algo._input_names == {'gate_proj', 'down_proj'}          # the subsets' first input names: up_proj carries no Hessian
    feat = {}
    algo.cache_input_hook(None, (torch.zeros(1, 4, 256),), None, 'up_proj', feat)          # ignored before anything is touched
    assert feat == {}


def test_sparsity_type_n_m_through_the_base_class():
    algo, _ = _construct({'weight': {'sparsity_type': '2:4'}})
    assert algo.nm == (2, 4) and algo.sparsity == 0.5
    assert _construct({'weight': {'sparsity_type': '4:8', 'sparsity': 0.5}})[0].nm == (4, 8)
    with pytest.raises(ValueError, match='contradicts'):
        _construct({'weight': {'sparsity_type': '2:4', 'sparsity': 0.3}})
    with pytest.raises(ValueError):
        _construct({'weight': {'sparsity_type': '2:3'}})


def test_refusals_of_the_constructor():
    with pytest.raises(ValueError, match='calibration'):
        _construct({'weight': {'sparsity': 0.5}}, with_input=False)
    with pytest.raises(NotImplementedError, match='blocksize'):
        _construct({'weight': {'sparsity': 0.5}, 'special': {'blocksize': 64}})
    with pytest.raises(ValueError, match='sparsity'):
        _construct({'weight': {'n_prune_layers': 2}})
    with pytest.raises(ValueError, match=r'\[0, 1\)'):
        _construct({'weight': {'sparsity': 1.0}})


# ---- host-side query and argument checks of csrc/sparsegpt_loop.hip: none of these touches a GPU -----------------------------
def _lib():
    from llmc_amd import _ffi
    return _ffi, _ffi.lib()


def test_workspace_query_is_a_pure_host_call():
    _ffi, L = _lib()
    ws = L.llmc_sparsegpt_prune_ws_bytes(4096, 4096)
    assert ws >= 4096 * 128 * 4 + (32768 + 65536) * 4          # the block's errors, the two histograms
    assert L.llmc_sparsegpt_prune_ws_bytes(1, 128) > 0
    assert L.llmc_sparsegpt_prune_ws_bytes(0, 128) == 0 and L.llmc_sparsegpt_prune_ws_bytes(128, 0) == 0
    assert L.llmc_sparsegpt_prune_ws_bytes(-1, 128) == 0


def test_invalid_calls_return_before_touching_the_gpu():
    _ffi, L = _lib()
    A = 0x10000          # an aligned address; a refused call does not read it

    def call(W=A, U=A, R=4, K=256, sparsity=0.5, n=0, m=0, Wout=A, blocksize=128, ws=A):
        return L.llmc_sparsegpt_prune(W, U, R, K, sparsity, n, m, Wout, None, None, blocksize, ws, None)

    def refused(code, **kw):
        rc = call(**kw)
        return rc == code and 'sparsegpt_prune' in _ffi.last_error()
    assert refused(EINVAL, W=None) and refused(EINVAL, U=None) and refused(EINVAL, Wout=None) and refused(EINVAL, ws=None)
    assert refused(EINVAL, R=0) and refused(EINVAL, K=0)
    assert refused(EINVAL, blocksize=64) and 'blocksize' in _ffi.last_error()
    assert refused(EINVAL, sparsity=1.0) and 'sparsity' in _ffi.last_error()          # kth == numel
    assert refused(EINVAL, sparsity=-0.1) and refused(EINVAL, sparsity=float('nan')) and refused(EINVAL, sparsity=1.5)
    assert refused(EINVAL, n=5, m=4) and 'prune_n' in _ffi.last_error()
    assert refused(EINVAL, n=-1, m=4)
    assert refused(ENOTSUP, K=254) and 'multiple of 4' in _ffi.last_error()
    assert refused(ENOTSUP, n=1, m=3) and refused(ENOTSUP, n=1, m=32) and refused(ENOTSUP, n=1, m=-4)
    assert refused(ENOTSUP, n=4, m=8, K=132) and 'divide' in _ffi.last_error()


def test_wrapper_checks_its_arguments_then_refuses_cpu_tensors():
    from llmc_amd import _ffi
    from llmc_amd.compression.sparsification import sparse_ops
    W, U = torch.zeros(4, 256), torch.zeros(256, 256)
    with pytest.raises(ValueError, match='exactly one'):
        sparse_ops.sparsegpt_prune(W, U)
    with pytest.raises(ValueError, match='exactly one'):
        sparse_ops.sparsegpt_prune(W, U, sparsity=0.5, nm=(2, 4))
    with pytest.raises(ValueError):
        sparse_ops.sparsegpt_prune(W, U, sparsity=1.0)
    with pytest.raises(ValueError):
        sparse_ops.sparsegpt_prune(W, U, nm=(5, 4))
    with pytest.raises(ValueError):
        sparse_ops.sparsegpt_prune(W, torch.zeros(128, 128), sparsity=0.5)
    with pytest.raises(ValueError):
        sparse_ops.sparsegpt_prune(W.half(), U, sparsity=0.5)
    with pytest.raises(NotImplementedError):
        sparse_ops.sparsegpt_prune(W, U, nm=(1, 3))
    with pytest.raises(NotImplementedError):
        sparse_ops.sparsegpt_prune(torch.zeros(4, 132), torch.zeros(132, 132), nm=(4, 8))
    with pytest.raises(NotImplementedError):
        sparse_ops.sparsegpt_prune(torch.zeros(4, 254), torch.zeros(254, 254), sparsity=0.5)
    for kw in (dict(sparsity=0.5), dict(nm=(2, 4))):
        with pytest.raises(_ffi.LlmcHipError):
            sparse_ops.sparsegpt_prune(W, U, **kw)
