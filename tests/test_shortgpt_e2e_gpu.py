"""ShortGPT end to end on the GPU: the six-block ToyModel of tests/shortgpt_flow.py in bf16 and fp32 (scores equal the oracle's
on the very features the class scored, the blocks the fp64 truth ranks lowest are removed), and a four-layer Llama built from a
config, which afterwards runs with a KV cache, saves and loads as a two-layer model."""
import json

import numpy as np
import pytest
import torch

import shortgpt_flow as F
import shortgpt_oracle as O

pytestmark = pytest.mark.gpu


class Cfg(dict):
    __getattr__ = dict.get


def _run_recording(algo):
    """run_block_loop with every block's (inputs, outputs) kept as the class handed them to block_transform"""
    seen = []
    transform = algo.block_transform

    def record(input_feat, output_feat):
        seen.append((list(input_feat), list(output_feat)))
        return transform(input_feat, output_feat)

    algo.block_transform = record
    algo.run_block_loop()
    return seen


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_the_toy_flow_scores_like_the_oracle_and_removes_the_lowest_blocks(dtype):
    import llmc_amd.compression.sparsification as S
    dt = F.DT_NAME[dtype]
    model, inp = F.toy(dtype)
    blocks = list(model.model.blocks)
    sparse = {'method': 'ShortGPT', 'weight': {'n_prune_layers': 2}}
    algo = S.ShortGPT(model, sparse, inp, None, {'sparse': sparse})
    seen = _run_recording(algo)
    assert algo.importances.is_cuda and algo.importances.dtype == torch.float64          # on the device until deploy
    assert len(seen) == 6 and all(len(i) == len(o) == 6 for i, o in seen)
    # the input list is advanced by the dense outputs: block b + 1 scores the very tensors block b returned
    for (_, out), (nxt, _) in zip(seen, seen[1:]):
        assert all(a is b for a, b in zip(out, nxt))
    assert all(a is b for a, b in zip(seen[-1][1], algo.input['data']))
    with torch.no_grad():
        again = blocks[0].cuda()(seen[0][0][0])
    blocks[0].cpu()
    assert torch.equal(again, seen[0][1][0])
    feats = [list(zip(i, o)) for i, o in seen]
    want, truth = F.scores(feats, dt, exact=False), F.scores(feats, dt, exact=True)
    got = algo.importances.cpu().numpy()
    assert np.array_equal(got, want), (got, want)
    tokens, d = 6 * 64, 256
    summed_bound = tokens * O.bound(d, dt)
    gaps = np.diff(np.sort(truth))
    print(dt, 'importances', got, 'smallest gap', gaps.min(), 'summed bound', summed_bound)
    assert gaps.min() > 100 * summed_bound and np.abs(got - truth).max() <= summed_bound
    removed = algo.deploy('fake_quant')
    assert sorted(removed) == sorted(np.argsort(truth)[:2].tolist()) == [1, 3]
    assert len(model.model.blocks) == 4 and [blocks.index(b) for b in model.model.blocks] == [0, 2, 4, 5]
    assert algo.num_blocks == 4 and len(algo.blocks) == 4


def _llama4(seed=0):
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(seed)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=4, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=160, max_position_embeddings=256, attn_implementation='eager')
    cfg.use_cache = False
    return LlamaForCausalLM(cfg)


def test_a_four_layer_llama_loses_two_layers_and_still_runs_with_a_cache(tmp_path):
    import hf_adapters as H
    import llmc_amd.compression.sparsification as S
    from transformers import LlamaForCausalLM
    model = H.HFLlama(_llama4(), torch.bfloat16)
    # down_proj of two layers made small: their influence, and which layers go, is then far from a tie
    small = (1, 2)
    for i in small:
        model.model.model.layers[i].mlp.down_proj.weight.data *= 0.05
        model.model.model.layers[i].self_attn.o_proj.weight.data *= 0.05
    twin = _llama4().to(torch.bfloat16)                     # the same weights: what the kept layers compute, applied in sequence
    twin.load_state_dict(model.model.state_dict())
    inp = model.collect_first_block_input(H.calib_ids(4, 64, 160))
    sparse = Cfg(method='ShortGPT', weight=Cfg(n_prune_layers=2))
    algo = S.ShortGPT(model, sparse, inp, None, Cfg(calib=Cfg(seq_len=64), model=Cfg(type='Llama'), sparse=sparse))
    seen = _run_recording(algo)
    want = F.scores([list(zip(i, o)) for i, o in seen], 'bf16', exact=False)
    assert np.array_equal(algo.importances.cpu().numpy(), want)
    removed = algo.deploy('fake_quant')
    assert sorted(removed) == sorted(np.argsort(want, kind='stable')[:2].tolist()) == list(small)
    net = model.model
    layers = net.model.layers
    assert len(layers) == 2 and net.config.num_hidden_layers == 2 and model.model_config.num_hidden_layers == 2
    assert [l.self_attn.layer_idx for l in layers] == [0, 1]
    kept = [i for i in range(4) if i not in removed]
    twin.model.layers = torch.nn.ModuleList([twin.model.layers[i] for i in kept])
    twin.config.num_hidden_layers = 2
    ids = H.calib_ids(1, 48, 160, seed=9)[0].cuda()
    net.cuda()
    twin.cuda()
    with torch.no_grad():
        out = net(ids, use_cache=True)
        ref = twin(ids, use_cache=False).logits.float()
    logits = out.logits.float()
    assert out.past_key_values is not None and out.past_key_values.get_seq_length() == 48
    # the same layers on the same input, with and without a cache: a few bf16 roundings of the largest logit at the most (a
    # wrong or missing layer moves the logits by their own size)
    tol = 2.0 ** -6 * float(ref.abs().max())
    print('llama: removed', removed, 'scores', want, 'max |logits - kept layers in sequence|', float((logits - ref).abs().max()), 'tol', tol)
    assert torch.isfinite(logits).all() and float((logits - ref).abs().max()) <= tol
    net.cpu()
    algo.save_model(str(tmp_path))
    with open(tmp_path / 'config.json') as fh:
        assert json.load(fh)['num_hidden_layers'] == 2
    loaded = LlamaForCausalLM.from_pretrained(str(tmp_path), dtype=torch.bfloat16, attn_implementation='eager').cuda()
    assert len(loaded.model.layers) == 2
    with torch.no_grad():
        again = loaded(ids, use_cache=True).logits.float()
    print('llama: reloaded, max |logits - kept layers in sequence|', float((again - ref).abs().max()))
    assert float((again - ref).abs().max()) <= tol
