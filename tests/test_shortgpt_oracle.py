"""tests/shortgpt_oracle.py against tests/golden/shortgpt.npz (the reference's ShortGPT.compute_bi on CPU) without a GPU: the
numpy restatement of llmc_block_influence stays within its derived bound of the fp64 truth, is nearer to it than the reference on
16-bit features and agrees with the reference on fp32 ones; the composed path (what CPU tensors run) holds the same bound."""
import numpy as np
import pytest
import torch

import shortgpt_oracle as O

CASES = ['random_f16', 'random_bf16', 'random_f32', 'zero_token_bf16', 'same_bf16']


@pytest.fixture(scope='module')
def g(golden):
    return golden('shortgpt')


def test_the_golden_file_holds_the_cases_the_tests_name(g):
    assert [str(n) for n in g['names']] == CASES
    assert len(set(g['importances'].tolist())) == g['importances'].size == 6          # (a): no ties


@pytest.mark.parametrize('name', CASES)
def test_oracle_tokens_stay_within_the_derived_bound_of_the_fp64_truth(g, name):
    dt, x, y, ref_bi, ref_total, ref_dist = O.golden_case(g, name)
    assert x.shape == (48, 96) and ref_bi.shape == (48,)
    bi, tr = O.block_influence(x, y, dt), O.truth(x, y)
    b = O.bound(96, dt)
    assert bi.dtype == np.float32 and 0 < b < 3e-6                                    # (2 L + 20) u with L = 8 or 4
    assert np.abs(bi.astype(np.float64) - tr).max() <= b
    assert abs(float(O.total(bi)) - tr.sum()) <= 48 * b
    if name == 'zero_token_bf16':
        assert bi[29] == 0.5 and ref_bi[29] == 0.5
    if name == 'same_bf16':
        assert np.abs(bi).max() <= b and np.abs(tr).max() < 1e-15


@pytest.mark.parametrize('name', [c for c in CASES if not c.endswith('f32')])
def test_on_16_bit_features_the_oracle_total_is_nearer_the_truth_than_the_reference(g, name):
    dt, x, y, ref_bi, ref_total, ref_dist = O.golden_case(g, name)
    tr = O.truth(x, y).sum()
    assert abs(float(O.total(O.block_influence(x, y, dt))) - tr) <= abs(ref_total - tr)          # (b)


def test_on_fp32_features_every_reference_token_lies_within_the_bound_plus_its_own_distance(g):
    dt, x, y, ref_bi, ref_total, ref_dist = O.golden_case(g, 'random_f32')
    assert np.abs(ref_bi.astype(np.float64) - O.truth(x, y)).max() == ref_dist
    bi = O.block_influence(x, y, dt)
    assert (np.abs(bi.astype(np.float64) - ref_bi) <= O.bound(96, dt) + ref_dist).all()          # (c)


def test_the_order_is_the_stated_one_on_a_row_where_it_shows():
    """Lane 0 holds 2^24, every other element is 1: a lane's own chain absorbs its ones one by one only where it starts at 2^24.
    Slot l of bf16 is the elements 8 l .. 8 l + 7; lane 0 folds slots 0 and 64. The butterfly adds lane sums, which are exact."""
    d = 8 * 65
    x = np.ones((1, d), np.float32)
    x[0, 0] = 2.0 ** 24
    y = np.ones((1, d), np.float32)
    dot, sx, sy = O.row_sums(x, y, 'bf16')
    # lane 0: 2^24 + 15 ones, each absorbed (round to even); lanes 1 .. 63: 8 each, exact
    assert dot[0] == np.float32(2.0 ** 24 + 63 * 8) and sy[0] == d and sx[0] == np.float32(2.0 ** 48 + 63 * 8)
    # the fp32 slots are 4 wide: lane 0 folds slots 0, 64, 128: 2^24 + 11 ones absorbed; lanes 1 .. 63 hold 8 or 12
    dot4 = O.row_sums(x, y, 'f32')[0]
    assert dot4[0] == np.float32(2.0 ** 24 + (d - 12))


def test_total_is_an_fp64_sum_in_chunks_of_4096_and_folds():
    rng = np.random.default_rng(3)
    bi = rng.random(70000).astype(np.float32)
    t = O.total(bi)
    assert abs(t - bi.astype(np.float64).sum()) <= 1e-9 * t
    parts = [O.total(bi[i:i + 4096]) for i in range(0, 70000, 4096)]          # a chunk's value is the total of the chunk alone
    assert len(parts) == 18 and t == O._strided_sum(np.array(parts)[None])[0]
    assert O.total(bi[:100], running=t) == t + O.total(bi[:100])


@pytest.mark.parametrize('name', CASES)
def test_the_composed_path_holds_the_same_bound_and_cpu_tensors_run_it(g, name):
    from llmc_amd.compression.sparsification import sparse_ops
    dt, x, y, ref_bi, ref_total, ref_dist = O.golden_case(g, name)
    tdt = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}[dt]
    xt, yt = torch.from_numpy(x).to(tdt).reshape(2, 24, 96), torch.from_numpy(y).to(tdt).reshape(2, 24, 96)
    assert torch.equal(xt.float().reshape(48, 96), torch.from_numpy(x))
    composed = sparse_ops.block_influence_composed(xt, yt)
    assert composed.dtype == torch.float32 and composed.shape == (48,)
    # torch sums a row in another order than the kernel: the bound's chain of L + 6 adds covers any order of at most that depth;
    # a pairwise or sequential sum of 96 elements is bounded by the sequential depth 96
    b = O.bound(96 * 64, dt)
    assert np.abs(composed.numpy().astype(np.float64) - O.truth(x, y)).max() <= b
    bi, total = sparse_ops.block_influence(xt, yt)
    assert torch.equal(bi, composed) and total.dtype == torch.float64 and total.shape == ()
    assert total.item() == composed.double().sum().item()
    run = torch.zeros(3, dtype=torch.float64)
    sparse_ops.block_influence(xt, yt, run[1], init=True)
    sparse_ops.block_influence(xt[:1], yt[:1], run[1], init=False)
    assert run[0] == 0 and run[2] == 0 and run[1].item() == total.item() + composed[:24].double().sum().item()
    with pytest.raises(ValueError, match='init=False'):
        sparse_ops.block_influence(xt, yt, init=False)
    with pytest.raises(ValueError, match='fp64'):
        sparse_ops.block_influence(xt, yt, torch.zeros(1))
