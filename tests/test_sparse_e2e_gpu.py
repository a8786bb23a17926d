"""Wanda and Magnitude on the toy adapter (hidden 256, inner 384, 6 x 64 tokens, bf16), end to end on the GPU, against the oracle
flow: the reference's expressions in torch (tests/sparse_oracle.py) fed the inputs the class itself captured.

Wanda's statistic is an fp32 sum whose order differs between the kernel and torch, so two elements of a row whose metrics lie
within the summation error of each other may swap sides. An element pruned by one side and kept by the other must be such a
near-tie: its fp64 metric |w| * sqrt(S64 / n) lies within the relative eps = 2 * (N + 2) * 2^-24 of the fp64 selection boundary
of its row or group, N the token count — the summation bound (N + 1) * 2^-24 halved by the square root, plus the product's
rounding, doubled for the two sides. Rows holding such a disagreement may be at most 1 % of all rows: a condition on the seeded
inputs, not a tolerance."""
import copy
import gc
import weakref

import pytest
import torch

import sparse_oracle as O
from toy_model import ToyModel, calib_input

pytestmark = pytest.mark.gpu

N_SEQ, SEQ = 6, 64
N_TOK = N_SEQ * SEQ
EPS = 2 * (N_TOK + 2) * 2.0 ** -24
LINEARS = ('gate_proj', 'up_proj', 'down_proj')


def S():
    import llmc_amd.compression.sparsification as S
    return S


def make(method, sparse, with_input=True, record=False):
    model = ToyModel()
    dense = [{n: getattr(b, n).weight.data.clone() for n in LINEARS} for b in model.get_blocks()]
    cfg = dict(sparse, method=method)
    cls = getattr(S(), method)
    log = {'inputs': {}, 'refs': [], 'feat': []}
    if record:
        class Recording(cls):
            def cache_input_hook(self, m, x, y, name, feat_dict):
                log['inputs'].setdefault((self.block_idx, name), []).append(x[0].detach().cpu())
                log['refs'].append(weakref.ref(x[0]))
                super().cache_input_hook(m, x, y, name, feat_dict)

            def block_transform(self, block, input_feat, block_kwargs):
                log['feat'].append({k: v for k, v in input_feat.items()})
                super().block_transform(block, input_feat, block_kwargs)
        cls = Recording
    algo = cls(model, cfg, calib_input(model, N_SEQ, SEQ) if with_input else None, None, {'sparse': cfg})
    return algo, model, dense, log


def weights(model):
    return [{n: getattr(b, n).weight.data.detach().cpu() for n in LINEARS} for b in model.get_blocks()]


# ---- Magnitude -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_input', [True, False])
def test_magnitude_equals_the_oracle_flow_exactly(with_input):
    algo, model, dense, _ = make('Magnitude', {'weight': {'sparsity': 0.5}}, with_input)
    algo.run_block_loop()
    for b, ws in enumerate(weights(model)):
        for n in LINEARS:
            w = dense[b][n]
            want, _, mask = O.magnitude_prune(w, int(w.numel() * 0.5))
            assert torch.equal(O.bits(ws[n]), O.bits(want)), (b, n)          # every layer of a subset, not only the last
            assert int(mask.sum()) >= w.numel() // 2
    assert all(getattr(b, n).weight.device.type == 'cpu' for b in model.get_blocks() for n in LINEARS)


# ---- Wanda ---------------------------------------------------------------------------------------------------------------------
def oracle_layer(w, acts, n_prune, m):
    """-> (oracle mask, fp64 metric, boundary lo / hi) for one layer from the captured batches"""
    act = torch.cat(acts, 0)          # [n_seq, T, K]
    assert act.shape[0] == N_SEQ and act.shape[1] == SEQ
    scaler = O.row_scale(act)
    _, mask = O.prune_rows(w, scaler, n_prune, m)
    m64 = w.double().abs() * torch.sqrt(O.col_sqsum64(act) / act.shape[0]).reshape(1, -1)
    lo, hi = O.selection_boundary64(m64, n_prune, m)
    return mask.bool(), m64, lo, hi


def compare_with_oracle(model, dense, log, n_of, m):
    rows = bad_rows = diffs = 0
    for b, ws in enumerate(weights(model)):
        for n in LINEARS:
            w0, w1 = dense[b][n], ws[n]
            R, K = w0.shape
            n_prune = n_of(K)
            ours = (w1 == 0) & (w0 != 0)
            assert bool(((w1 == w0) | ours).all()), 'a kept element changed'
            added = ours.reshape(-1, m or K).sum(1)
            assert bool((added == n_prune).all()), (b, n, 'zeros per row / group')          # the seeded weights hold no zero
            want, m64, lo, hi = oracle_layer(w0, log['inputs'][(b, 'gate_proj' if n != 'down_proj' else n)], n_prune, m)
            diff = ours != want
            near = (m64 >= lo * (1 - EPS)) & (m64 <= hi * (1 + EPS))
            assert bool(near[diff].all()), (b, n, 'a disagreement that is not a near-tie')
            rows += R
            bad_rows += int(diff.any(1).sum())
            diffs += int(diff.sum())
    assert bad_rows <= 0.01 * rows, (bad_rows, rows)
    return diffs


@pytest.mark.parametrize('sparse,m', [({'weight': {'sparsity': 0.5}}, None), ({'weight': {'sparsity_type': '2:4'}}, 4),
                                      ({'weight': {'sparsity': 0.3}, 'sparsity_out': True}, None)])
def test_wanda_matches_the_oracle_flow(sparse, m):
    algo, model, dense, log = make('Wanda', sparse, record=True)
    assert all(bool((w != 0).all()) for d in dense for w in d.values())
    algo.run_block_loop()
    s = sparse['weight'].get('sparsity', 0.5)
    compare_with_oracle(model, dense, log, (lambda K: 2) if m else (lambda K: int(K * s)), m)


def block_outputs(block_weights, model, b, data):
    blk = copy.deepcopy(model.get_blocks()[b]).cuda()
    for n in LINEARS:
        getattr(blk, n).weight.data = block_weights[n].cuda()
    with torch.no_grad():
        return [blk(x.cuda()).cpu() for x in data]


@pytest.mark.parametrize('sparsity_out', [False, True])
def test_sparsity_out_decides_what_feeds_the_next_block(sparsity_out):
    algo, model, dense, log = make('Wanda', {'weight': {'sparsity': 0.5}, 'sparsity_out': sparsity_out}, record=True)
    data = [x.clone() for x in algo.input['data']]
    algo.run_block_loop()
    pruned = weights(model)
    assert algo.sparsity_out is sparsity_out
    from_dense = block_outputs(dense[0], model, 0, data)
    from_pruned = block_outputs(pruned[0], model, 0, data)
    assert not all(torch.equal(a, b) for a, b in zip(from_dense, from_pruned))
    feeds = from_pruned if sparsity_out else from_dense
    # block 2's LayerNorm output is what its gate_proj captured: recompute it from what should have fed the block
    ln = copy.deepcopy(model.get_blocks()[1].ln).cuda()
    with torch.no_grad():
        want = [ln(x.cuda()).cpu() for x in feeds]
        other = [ln(x.cuda()).cpu() for x in (from_dense if sparsity_out else from_pruned)]
    got = log['inputs'][(1, 'gate_proj')]
    assert len(got) == N_SEQ and all(torch.equal(O.bits(a), O.bits(b)) for a, b in zip(got, want))
    assert not all(torch.equal(a, b) for a, b in zip(got, other))          # the two settings differ
    compare_with_oracle(model, dense, log, lambda K: K // 2, None)          # and each matches the oracle flow run its way


def test_wanda_keeps_sums_not_activations():
    algo, model, dense, log = make('Wanda', {'weight': {'sparsity': 0.5}}, record=True)
    algo.block_idx = 0
    algo.block_opt(model.get_blocks()[0])
    gc.collect()
    assert len(log['refs']) == 3 * N_SEQ and all(r() is None for r in log['refs']), 'a captured activation is still referenced'
    (feat,) = log['feat']
    assert set(feat) == set(LINEARS)
    for name, st in feat.items():
        K = dense[0][name].shape[1]
        assert st.n == N_SEQ and st.acc.shape == (K,) and st.acc.dtype == torch.float32 and st.scaler_row.shape == (K,)
        want = O.col_sqsum64(torch.cat(log['inputs'][(0, name)], 0))
        assert ((st.acc.cpu().double() - want).abs() <= (N_TOK + 1) * 2.0 ** -24 * want).all()


def test_get_row_scale_keeps_the_reference_meaning():
    algo, model, _, _ = make('Wanda', {'weight': {'sparsity': 0.5}})
    layer = model.get_blocks()[0].gate_proj.cuda()
    g = torch.Generator().manual_seed(3)
    act = torch.randint(-8, 9, (3, 20, 256), generator=g).to(torch.bfloat16)
    got = algo.get_row_scale(layer, act.cuda())
    assert torch.equal(got.cpu(), (O.col_sqsum64(act) / 3).float())          # exact sums: sum / act.shape[0]
    got2 = algo.get_row_scale(layer, act[0].cuda())                           # a 2-D act is one sequence
    assert torch.equal(got2.cpu(), O.col_sqsum64(act[0]).float())
    layer.cpu()
