"""SparseGPT over the two-block toy adapter (hidden 256, inner 384, 6 x 64 tokens, bf16), end to end on the GPU. Every call of
sparse_ops.sparsegpt_prune is recorded; the oracle (tests/sparsegpt_oracle.py) is replayed on the recorded (W, U) on the CPU and
each layer's stored weight must equal the oracle's Wout cast to the model dtype, bit for bit.

The proxy loss tr((W - W') H (W - W')^T), H from the captured inputs in float64, must be strictly below that of the same mask
applied without the update: the only assertion is `< 1`. Measured ratios on the toy's inputs: 0.73 - 0.74 for gate_proj /
up_proj, 0.37 - 0.39 for down_proj, in both modes."""
import numpy as np
import pytest
import torch

import sparsegpt_oracle as O
from toy_model import ToyModel, calib_input

pytestmark = pytest.mark.gpu

N_SEQ, SEQ = 6, 64
LINEARS = ('gate_proj', 'up_proj', 'down_proj')
INPUT_OF = {'gate_proj': 'gate_proj', 'up_proj': 'gate_proj', 'down_proj': 'down_proj'}


def run(sparse, monkeypatch):
    import llmc_amd.compression.sparsification as S
    from llmc_amd.compression.quantization.hessian import HessianAccumulator
    from llmc_amd.compression.sparsification import sparse_ops
    model = ToyModel()
    dense = [{n: getattr(b, n).weight.data.clone() for n in LINEARS} for b in model.get_blocks()]
    log = {'calls': [], 'inputs': {}, 'feat': []}
    real = sparse_ops.sparsegpt_prune

    def recording(W, Hinv, sparsity=None, nm=None, want_losses=False, want_mask=False):
        w_in, u_in = W.detach().cpu().numpy().copy(), Hinv.detach().cpu().numpy().copy()
        out = real(W, Hinv, sparsity=sparsity, nm=nm, want_losses=want_losses, want_mask=want_mask)
        log['calls'].append(dict(W=w_in, U=u_in, sparsity=sparsity, nm=nm, Wout=out[0].detach().cpu().numpy().copy()))
        return out
    monkeypatch.setattr(sparse_ops, 'sparsegpt_prune', recording)

    class Recording(S.SparseGPT):
        def cache_input_hook(self, m, x, y, name, feat_dict):
            log['inputs'].setdefault((self.block_idx, name), []).append(x[0].detach().cpu())
            super().cache_input_hook(m, x, y, name, feat_dict)

        def block_transform(self, block, input_feat, block_kwargs):
            log['feat'].append({k: type(v) for k, v in input_feat.items()})
            super().block_transform(block, input_feat, block_kwargs)
    cfg = dict(sparse, method='SparseGPT')
    algo = Recording(model, cfg, calib_input(model, N_SEQ, SEQ), None, {'sparse': cfg})
    algo.run_block_loop()
    for feat in log['feat']:
        assert feat == {'gate_proj': HessianAccumulator, 'down_proj': HessianAccumulator}          # only the subsets' input names
    return model, dense, log


def hessian64(acts):
    x = torch.cat(acts, 0).double().reshape(-1, acts[0].shape[-1]).numpy()
    return 2.0 / N_SEQ * (x.T @ x)


def proxy(dW, H):
    return float(np.einsum('rk,kj,rj->', dW, H, dW))


@pytest.mark.parametrize('sparsity_out', [False, True])
@pytest.mark.parametrize('weight', [{'sparsity': 0.5}, {'sparsity_type': '2:4'}])
def test_sparsegpt_equals_the_replayed_oracle(weight, sparsity_out, monkeypatch):
    model, dense, log = run({'weight': weight, 'sparsity_out': sparsity_out}, monkeypatch)
    calls = log['calls']
    assert len(calls) == 2 * len(LINEARS)          # gate, up, down per block, in subset order
    kw = dict(nm=(2, 4)) if 'sparsity_type' in weight else dict(sparsity=0.5)
    for b, blk in enumerate(model.get_blocks()):
        cg, cu, cd = calls[3 * b:3 * b + 3]
        assert np.array_equal(O.bits(cg['U']), O.bits(cu['U']))          # the layers of one subset share the factor
        assert cd['U'].shape == (384, 384) and cg['U'].shape == (256, 256)
        for name, c in zip(LINEARS, (cg, cu, cd)):
            assert (c['sparsity'], c['nm']) == (kw.get('sparsity'), kw.get('nm'))
            w0 = dense[b][name]
            assert np.array_equal(O.bits(c['W']), O.bits(w0.float().numpy())), 'the loop starts from the fp32 weight'
            want = O.prune(c['W'], c['U'], **kw)
            assert np.array_equal(O.bits(c['Wout']), O.bits(want['Wout'])), (b, name)
            stored = getattr(blk, name).weight.data
            assert stored.dtype == torch.bfloat16 and stored.device.type == 'cpu'
            cast = torch.from_numpy(want['Wout']).to(torch.bfloat16)
            assert torch.equal(stored.view(torch.int16), cast.view(torch.int16)), (b, name)
            # the update pays: against the same mask applied to the dense weight, the proxy loss tr(dW H dW^T) is lower
            H = hessian64(log['inputs'][(b, INPUT_OF[name])])
            w064 = w0.double().numpy()
            masked = np.where(want['mask'] != 0, 0.0, w064)
            ours, plain = proxy(want['Wout'].astype(np.float64) - w064, H), proxy(masked - w064, H)
            print(f'sparsegpt e2e {weight} sparsity_out={sparsity_out} block {b} {name}: proxy loss ratio {ours / plain:.4f}')
            assert ours < plain, (b, name, ours, plain)


def test_a_dead_input_channel_is_zeroed_in_every_layer_of_the_subset(monkeypatch):
    """diag(H) == 0: the weight column is zeroed before the loop, in gate_proj AND up_proj — the call that fixes the dead diagonal
    is the only one that knows the dead columns, so the subset's weights go through it together"""
    import llmc_amd.compression.sparsification as S
    from llmc_amd.compression.quantization.hessian import HessianAccumulator
    from llmc_amd.compression.sparsification import sparse_ops
    model = ToyModel()
    cfg = {'method': 'SparseGPT', 'weight': {'sparsity_type': '2:4'}}
    algo = S.SparseGPT(model, cfg, calib_input(model, N_SEQ, SEQ), None, {'sparse': cfg})
    block = model.get_blocks()[0].cuda()
    subset = model.get_subsets_in_block(block)[0]
    x = torch.randn(2, SEQ, 256, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).cuda()
    x[..., 5] = 0
    acc = HessianAccumulator(256, x.device)
    acc.add(x)
    seen, real = [], sparse_ops.sparsegpt_prune
    monkeypatch.setattr(sparse_ops, 'sparsegpt_prune', lambda W, U, **kw: (seen.append(W.detach().cpu().clone()), real(W, U, **kw))[1])
    algo.subset_transform(subset, {'gate_proj': acc}, {})
    assert len(seen) == 2
    for w_in, layer in zip(seen, (block.gate_proj, block.up_proj)):
        assert bool((w_in[:, 5] == 0).all()) and bool((w_in[:, 4] != 0).any())
        assert bool((layer.weight.data[:, 5] == 0).all())
    block.cpu()


def test_sparsity_out_changes_what_the_second_block_sees(monkeypatch):
    _, _, dense_log = run({'weight': {'sparsity': 0.5}, 'sparsity_out': False}, monkeypatch)
    _, _, pruned_log = run({'weight': {'sparsity': 0.5}, 'sparsity_out': True}, monkeypatch)
    a, b = dense_log['inputs'][(1, 'gate_proj')], pruned_log['inputs'][(1, 'gate_proj')]
    assert len(a) == len(b) == N_SEQ and not all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(torch.equal(x, y) for x, y in zip(dense_log['inputs'][(0, 'gate_proj')], pruned_log['inputs'][(0, 'gate_proj')]))
