"""`sparse.method: TokenReduction` / `special.method: DivPrune` without a GPU: the registries, the hook on a stub Llava-named model
(prefill pruned, decode passed through, the kept positions, the mask), the refusals, and the reference's surface."""
import ast
import inspect
import os

import pytest
import torch

from conftest import ROOT

REF = os.path.join(ROOT, 'oracle', '_ref', 'llmc', 'compression', 'token_reduction')
IMAGE_TOKEN_INDEX = -200
L_IMG, START, TAIL, WIDTH = 24, 5, 4, 16


class _Vlm:
    """what LLaVA's prepare_inputs_labels_for_multimodal does to the tensors the hook reads: the one image token of input_ids becomes
    L_IMG embeddings"""
    calls = 0

    def prepare_inputs_labels_for_multimodal(self, input_ids, position_ids, attention_mask, past_key_values, labels, images=None):
        self.calls += 1
        if input_ids.shape[1] == 1:
            return input_ids, position_ids, attention_mask, past_key_values, None, labels
        n = input_ids.shape[1] - 1 + L_IMG
        g = torch.Generator().manual_seed(3)
        embeds = torch.randn(1, n, WIDTH, generator=g)
        return None, torch.arange(n)[None], torch.ones(1, n, dtype=torch.bool), past_key_values, embeds, labels


class Llava:
    def __init__(self, with_index=True):
        self.vlm_model = _Vlm()
        self.pruning_config = {'is_video_model': False, 'image_token_length': L_IMG}
        if with_index:
            self.pruning_config['image_token_index'] = IMAGE_TOKEN_INDEX

    def get_blocks(self):
        return [torch.nn.Identity(), torch.nn.Identity()]


class Qwen2VL(Llava):
    pass


def _algo(model, rate=0.25, method='DivPrune'):
    from llmc_amd.utils.registry_factory import ALGO_REGISTRY
    import llmc_amd.compression.token_reduction  # noqa: F401
    cfg = {'method': 'TokenReduction', 'special': {'method': method, 'rate': rate}}
    return ALGO_REGISTRY['TokenReduction'](model, cfg, None, None, {'sparse': cfg})


def _prompt():
    ids = torch.arange(10, 10 + START + 1 + TAIL)[None]
    ids[0, START] = IMAGE_TOKEN_INDEX
    return ids, torch.ones_like(ids, dtype=torch.bool)


def test_the_registries_hold_the_family():
    from llmc_amd.utils.registry_factory import ALGO_REGISTRY, TOKEN_REDUCTION_REGISTRY
    from llmc_amd.compression.token_reduction import DivPrune, TokenReduction, TokenReductionModule
    assert ALGO_REGISTRY['TokenReduction'] is TokenReduction
    assert TOKEN_REDUCTION_REGISTRY['DivPrune'] is DivPrune and issubclass(DivPrune, TokenReductionModule)


@pytest.mark.parametrize('rate', [0.25, 0.1, 0.52])
def test_the_hook_prunes_a_prefill_and_keeps_every_other_position(rate):
    from llmc_amd.compression.token_reduction.divprune import divprune
    model = Llava()
    algo = _algo(model, rate)
    algo.block_opt(model.get_blocks()[0])                 # nothing to do per block
    ids, mask = _prompt()
    out = model.vlm_model.prepare_inputs_labels_for_multimodal(ids, None, mask, None, None)
    _, position_ids, attention_mask, _, embeds, _ = out
    k = int(round(rate * L_IMG))
    n = START + k + TAIL
    assert tuple(embeds.shape) == (1, n, WIDTH) and tuple(attention_mask.shape) == (1, n) and tuple(position_ids.shape) == (1, n)
    keep = position_ids[0]                                # the stub's ids are arange: what is left IS keep_indexs
    assert torch.equal(keep, keep.sort().values) and len(set(keep.tolist())) == n
    assert keep[:START].tolist() == list(range(START)) and keep[-TAIL:].tolist() == list(range(START + L_IMG, START + L_IMG + TAIL))
    full = _Vlm().prepare_inputs_labels_for_multimodal(ids, None, mask, None, None)[4]
    assert torch.equal(embeds[0], full[0][keep])
    want, _ = divprune(full[0][START:START + L_IMG], L_IMG, None, rate)
    assert keep[START:START + k].tolist() == sorted((want + START).tolist())
    assert algo.reduction_module.pruning_paras['image_token_start_index'] == START


def test_the_hook_passes_a_decode_step_through():
    model = Llava()
    algo = _algo(model)
    assert 'prepare_inputs_labels_for_multimodal' in vars(model.vlm_model)               # the wrapper is on the instance
    ids = torch.tensor([[42]])
    out = model.vlm_model.prepare_inputs_labels_for_multimodal(ids, None, torch.ones(1, 30, dtype=torch.bool), None, None)
    assert out[0] is ids and out[4] is None and model.vlm_model.calls == 1
    assert 'image_token_start_index' not in algo.reduction_module.pruning_paras


def test_a_padded_prompt_is_searched_under_its_mask():
    model = Llava()
    algo = _algo(model)
    ids, mask = _prompt()
    ids = torch.cat([torch.full((1, 2), IMAGE_TOKEN_INDEX), ids], 1)           # two masked-out pad positions that look like the token
    mask = torch.cat([torch.zeros(1, 2, dtype=torch.bool), mask], 1)
    model.vlm_model.prepare_inputs_labels_for_multimodal(ids, None, mask, None, None)
    assert algo.reduction_module.pruning_paras['image_token_start_index'] == START


def test_each_unbuilt_method_is_refused_by_name():
    from llmc_amd.compression.token_reduction.base_blockwise_token_reduction import BUILT, UNBUILT
    assert len(UNBUILT) == 12 and BUILT == ('DivPrune',)
    for method in UNBUILT:
        with pytest.raises(NotImplementedError, match=rf'{method} is not built \(built: DivPrune'):
            _algo(Llava(), method=method)
    with pytest.raises(NotImplementedError, match='no token-reduction method'):
        _algo(Llava(), method='NoSuchMethod')


def test_a_model_that_is_not_llava_registers_nothing_and_says_so_once(capsys):
    model = Qwen2VL()
    _algo(model)
    _algo(model)
    assert 'prepare_inputs_labels_for_multimodal' not in vars(model.vlm_model)           # the class's own method, not a wrapper
    err = capsys.readouterr().err
    assert err.count('Qwen2VL is not Llava') == 1


def test_the_image_token_index_comes_from_the_pruning_config_and_llava_is_imported_only_without_it():
    import sys
    assert 'llava' not in sys.modules
    _algo(Llava())
    assert 'llava' not in sys.modules
    with pytest.raises(ImportError):
        _algo(Llava(with_index=False))                    # no `llava` package in the test environment


def test_deploy_reports(capsys):
    algo = _algo(Llava())
    algo.deploy('fake_quant')
    err = capsys.readouterr().err
    assert 'deploy_token_reduction_model start' in err and "'rate': 0.25" in err


def _ref_class_methods(fname, cls):
    tree = ast.parse(open(os.path.join(REF, fname)).read())
    node = {n.name: n for n in tree.body if isinstance(n, ast.ClassDef)}[cls]
    return {m.name: [a.arg for a in m.args.posonlyargs + m.args.args] for m in node.body if isinstance(m, ast.FunctionDef)}


def _ref_functions(fname):
    tree = ast.parse(open(os.path.join(REF, fname)).read())
    return {m.name: [a.arg for a in m.args.posonlyargs + m.args.args] for m in tree.body if isinstance(m, ast.FunctionDef)}


@pytest.mark.skipif(not os.path.isdir(REF), reason='oracle/_ref is built by __graft_entry__.build() where the reference tree exists')
@pytest.mark.parametrize('fname,cls', [('base_blockwise_token_reduction.py', 'TokenReduction'),
                                       ('token_reduction_module.py', 'TokenReductionModule'), ('divprune.py', 'DivPrune')])
def test_every_reference_method_exists_with_the_same_argument_names(fname, cls):
    import llmc_amd.compression.token_reduction as T
    ours = getattr(T, cls)
    for name, want in _ref_class_methods(fname, cls).items():
        f = inspect.getattr_static(ours, name, None)
        assert f is not None, f'{cls}.{name} is missing'
        mine = [p.name for p in inspect.signature(getattr(ours, name)).parameters.values()
                if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
        assert mine[:len(want)] == want, (cls, name, want, mine)


@pytest.mark.skipif(not os.path.isdir(REF), reason='oracle/_ref is built by __graft_entry__.build() where the reference tree exists')
def test_the_module_functions_take_the_reference_arguments():
    from llmc_amd.compression.token_reduction import divprune as ours
    ref = _ref_functions('divprune.py')
    assert set(ref) == {'pairwise_cosine_similarity', 'divprune', 'divprune_post_hook'}
    for name, want in ref.items():
        mine = [p.name for p in inspect.signature(getattr(ours, name)).parameters.values()]
        assert mine == want, (name, want, mine)
