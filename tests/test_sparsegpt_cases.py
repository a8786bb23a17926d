"""The inputs of tests/test_sparsegpt_widths_gpu.py (tests/sparsegpt_cases.py) reach what they are named for: shown here on the
oracle (tests/sparsegpt_oracle.py) and on the arrays themselves, never on the kernel's output, so that no GPU test passes
because its input stayed clear of the edge."""
import time

import numpy as np
import pytest

import sparsegpt_cases as C
import sparsegpt_oracle as O

TINY = np.float32(2.0 ** -126)          # the smallest normal fp32


def blocks(K):
    return [(i1, min(i1 + 128, K)) for i1 in range(0, K, 128)]


def prune(name, mode):
    W, U = C.select_case(name)
    return W, U, O.prune(W, U, **C.mode_kw(mode))


def test_one_bin_leaves_the_choice_to_the_second_digit():
    """in each of the 3 blocks the scores share the upper 16 bits of their pattern and spread over more than 10000 of the
    lower 65536; the threshold still cuts the panel in half"""
    W, U, o = prune('one_bin', 's0.5')
    assert W.shape == C.ONE_BIN_SHAPE and np.array_equal(U, np.eye(W.shape[1], dtype=np.float32))
    b = O.bits(o['scores'])
    assert len(blocks(W.shape[1])) == 3
    for i1, i2 in blocks(W.shape[1]):
        assert len(np.unique(b[:, i1:i2] >> 16)) == 1
        assert len(np.unique(b[:, i1:i2] & 0xffff)) > 10000
    assert abs(o['mask'].mean() - 0.5) <= 0.001, o['mask'].mean()
    assert np.array_equal(O.bits(o['W']), O.bits(W))          # the identity moves nothing: the later blocks are as written


def test_zero_floor_puts_the_threshold_on_plus_zero():
    """sparsity 0.5: every block's threshold is +0.0 exactly, the mask is W == 0 (either sign), nothing moves and nothing is
    lost, and a pruned -0.0 is stored as +0. Sparsity 0.59: the first two blocks still select a zero, the last (64 columns, one
    of them all zero) does not."""
    W, U, o = prune('zero_floor', 's0.5')
    R, K = W.shape
    assert (R, K) == C.EDGE_SHAPE and np.signbit(W[W == 0]).sum() * 4 > (W == 0).sum() > 0.6 * R * K
    assert ((W == 0).all(0)).sum() >= 3
    assert len(o['thresh']) == 3 and all(O.bits(t) == 0 for t in o['thresh'])
    assert np.array_equal(o['mask'], (W == 0).astype(np.uint8))
    assert o['mask'].mean() == (W == 0).mean() and 0.6 < o['mask'].mean() < 0.61, o['mask'].mean()
    assert np.array_equal(O.bits(o['W']), O.bits(W)) and not o['losses'].any()
    assert not np.signbit(o['Wout'][o['Wout'] == 0]).any()
    t = prune('zero_floor', 's0.59')[2]['thresh']
    assert O.bits(t[0]) == 0 and O.bits(t[1]) == 0 and t[2] > 0, t


def test_subnormal_scores_thresholds_and_losses():
    W, U, o = prune('subnormal', 's0.5')
    s = o['scores']
    assert ((s > 0) & (s < TINY)).mean() > 0.9 and (s == 0).any()
    assert all(0 < t < TINY for t in o['thresh']), o['thresh']
    assert 0.45 < o['mask'].mean() < 0.55          # a select that took every subnormal score for 0 would prune them all
    assert ((o['losses'] > 0) & (o['losses'] < TINY)).mean() > 0.4
    assert np.isfinite(W).all() and (W != 0).all()
    nm = prune('subnormal', '2:4')[2]
    assert (nm['mask'].reshape(-1, 4).sum(1) == 2).all()


def test_overflow_scores_are_inf_from_finite_weights():
    """sparsity 0.5: more than 200 scores are +inf, none of them is pruned and everything stored stays finite. Sparsity 0.985:
    the selected rank is one of them in every block, so +inf is the threshold, everything is pruned, losses hold +inf — and
    nothing is NaN."""
    W, U, o = prune('overflow', 's0.5')
    assert np.isfinite(W).all()
    inf = np.isposinf(o['scores'])
    assert inf.sum() > 200 and not o['mask'][inf].any()
    assert all(np.isfinite(o[k]).all() for k in ('W', 'Wout', 'losses'))
    o = prune('overflow', 's0.985')[2]
    assert all(np.isposinf(t) for t in o['thresh']), o['thresh']
    assert o['mask'].all() and not O.bits(o['Wout']).any()
    assert np.isposinf(o['losses']).any()
    assert not any(np.isnan(o[k]).any() for k in ('W', 'Wout', 'losses', 'scores'))


def test_the_last_rank_of_a_panel():
    R, K = C.RANK_SHAPE
    assert O.kth_of(R * 128, C.RANK_SPARSITY) == R * 128 - 1
    W, U, o = prune('rank_last', 's%r' % C.RANK_SPARSITY)
    assert W.shape == (R, K) and o['mask'].all() and not O.bits(o['Wout']).any()
    assert all(t == o['scores'][:, i1:i2].max() for t, (i1, i2) in zip(o['thresh'], blocks(K)))


@pytest.mark.parametrize('R,K,mode', C.RAGGED)
def test_ragged_cases_through_the_oracle(R, K, mode):
    """every (R, K) of the list with every mode that divides K; n:m prunes exactly n of every group, unstructured at least the
    selected rank and one more"""
    kw = C.mode_kw(mode)
    W, U = C.general(R, K)
    o = O.prune(W, U, **kw)
    assert o['Wout'].shape == (R, K) and np.isfinite(o['Wout']).all() and np.isfinite(o['losses']).all()
    if 'nm' in kw:
        n, m = kw['nm']
        assert K % m == 0 and (o['mask'].reshape(-1, m).sum(1) == n).all()
    else:
        for i1, i2 in blocks(K):
            assert o['mask'][:, i1:i2].sum() >= O.kth_of(R * (i2 - i1), kw['sparsity']) + 1


def test_the_lists_hold_what_the_kernel_branches_on():
    shapes = {(R, K) for R, K, _ in C.RAGGED}
    assert shapes == set(C.RAGGED_SHAPES) and len(C.RAGGED) == 8 * 2 + 3 + 2          # 4:8 at K = 136, 144, 128; 8:16 at 144, 128
    assert {K for _, K in shapes if K < 128} == {4, 20, 100, 124}
    assert ('4:8' in {m for R, K, m in C.RAGGED if K == 136}) and ('8:16' in {m for R, K, m in C.RAGGED if K == 144})
    assert {R for R, _ in shapes} == {1, 3, 4, 5, 15, 16, 31, 33}
    assert C.TALL[0][0] * 128 > 256 * 8192 and all(K % 128 in (0, 4) for _, K in C.TALL)
    assert [(K + 127) // 128 for _, K in C.WIDE] == [32, 86]
    assert C.SEQUENCE[0] == C.SEQUENCE[-1]
    V = C.nan_below(C.general(5, 20)[1])
    assert np.isnan(V[np.tril_indices(20, -1)]).all() and np.array_equal(np.triu(V), C.general(5, 20)[1])


def test_real_hessian_is_the_one_of_test_a_real_factor():
    import torch
    K = 512
    g = torch.Generator().manual_seed(7)
    X = torch.randn(2048, K, generator=g) * (1 + 3 * torch.rand(K, generator=g))
    H = (2.0 / 2048 * (X.T @ X)).float()
    H += 0.01 * torch.diagonal(H).mean() * torch.eye(K)
    got = C.real_hessian(K, 7)
    assert got.device.type == 'cpu' and got.dtype == torch.float32 and torch.equal(got, H)


def test_oracle_run_time_of_every_gpu_case(capsys):
    """prints the oracle's time for every case the GPU tests use (pytest -s shows it); nothing is asserted about time. WIDE runs
    on synth_upper here: the time does not depend on the factor's values."""
    rows = []

    def timed(what, W, U, mode):
        t0 = time.perf_counter()
        O.prune(W, U, **C.mode_kw(mode))
        rows.append((time.perf_counter() - t0, what, mode))

    for name, mode in C.SELECT:
        timed(name, *C.select_case(name), mode)
    for R, K, mode in C.RAGGED:
        timed(f'ragged {R}x{K}', *C.general(R, K), mode)
    for R, K in C.TALL + C.LOWER:
        for mode in C.BIG_MODES:
            timed(f'{R}x{K}', *C.general(R, K), mode)
    for R, K in C.WIDE:
        U = np.eye(K, dtype=np.float32) + np.triu(np.full((K, K), 2.0 ** -10, dtype=np.float32), 1)
        for mode in C.BIG_MODES:
            timed(f'wide {R}x{K}', C.weights(R, K), U, mode)
    for name, R, K, mode in C.SEQUENCE[:-1]:
        timed(f'sequence {name} {R}x{K}', *C.build(name, R, K), mode)
    with capsys.disabled():
        print()
        for t, what, mode in rows:
            print(f'  oracle {what:32s} {mode:10s} {t:7.3f} s')
        print(f'  slowest {max(rows)[0]:.3f} s, all {sum(r[0] for r in rows):.1f} s')
