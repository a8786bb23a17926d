"""tests/divprune_oracle.py and the CPU route of the token-selection operators against the reference's goldens
(tests/golden/divprune.npz, tools/make_golden_divprune.py): the selection rules on supplied matrices in three dtypes, and the exact
features on which the reference's own matrix is the fp64 value and most steps tie."""
import numpy as np
import pytest
import torch

import divprune_oracle as O

TDT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}


def test_the_goldens_hold_every_case_the_tests_lean_on(golden):
    g = golden('divprune')
    names = [str(n) for n in g['names']]
    assert sorted(names) == sorted(f'a_{c}_{d}' for c in ('sym', 'asym', 'ties', 'nan', 'dup', 'full') for d in TDT)
    assert [str(n) for n in g['exact']] == [f'b_{N}_{d}' for N, d, _ in O.EXACT_SHAPES]
    for dt in TDT:
        assert len(set(g[f'a_dup_{dt}/sel'].tolist())) < int(g[f'a_dup_{dt}/k'])           # an index chosen twice
        assert int(g[f'a_full_{dt}/k']) == g[f'a_full_{dt}/D_bits'].shape[0]              # k = N
        assert np.isnan(O.golden_matrix(g, f'a_nan_{dt}').float().numpy()).any()
    for N, d, k in O.EXACT_SHAPES:
        assert int(g[f'b_{N}_{d}/ties']) * 8 >= 7 * k                                      # the tie rule decides most steps


def test_select_reproduces_every_golden(golden):
    g = golden('divprune')
    for case in (str(n) for n in g['names']):
        D = O.golden_matrix(g, case).float().numpy()
        assert np.array_equal(O.select(D, int(g[f'{case}/k'])), g[f'{case}/sel']), case
    for case in (str(n) for n in g['exact']):
        for dt in TDT:
            assert np.array_equal(O.select(g[f'{case}/D'], int(g[f'{case}/k'])), g[f'{case}/sel_{dt}']), (case, dt)


def test_select_states_the_ordering_rules():
    nan = np.float32('nan')
    D = np.array([[0, 5, nan, 1], [5, 0, 2, -0.0], [nan, 2, 0, 0.0], [1, 0.0, -0.0, 0]], np.float32)
    # column seconds: [1, 0, 0 (-0 = +0; the NaN sorts last), 0]: the greatest is column 0
    assert O.select(D, 1).tolist() == [0]
    # step 1 is row 0 alone: [0, 5, nan, 1]: the NaN is the greatest; step 2: min(row 0, row 2) = [nan, 2, nan, 0]: the first NaN
    assert O.select(D, 3).tolist() == [0, 2, 0]
    with pytest.raises(ValueError):
        O.select(np.zeros((1, 1), np.float32), 1)
    assert O.select(D, 0).shape == (0,)


def test_the_exact_features_are_exact_and_the_bound_is_what_the_docstring_derives(golden):
    g = golden('divprune')
    for N, d, _ in O.EXACT_SHAPES:
        x = O.exact_tokens(N, d, int(g[f'b_{N}_{d}/seed']))
        for dt in TDT.values():
            assert np.array_equal(torch.from_numpy(x).to(dt).float().numpy(), x)
        truth = O.truth_dist(x)
        assert np.array_equal(g[f'b_{N}_{d}/D'].astype(np.float64), truth)
    assert 9.7e-4 < O.bound(4096, 'bf16') < 9.8e-4 and O.bound(4096, 'f32') > O.bound(4096, 'f16') == O.bound(4096, 'bf16')
    assert 2.0 ** -22 < O.bound(2, 'bf16') < 2.0 ** -20          # one addition: 2 u + 6 e and second-order terms


def test_the_composed_operators_reproduce_the_goldens_on_cpu_tensors(golden):
    from llmc_amd.compression.token_reduction import token_ops
    g = golden('divprune')
    for case in (str(n) for n in g['names']):
        D = O.golden_matrix(g, case)
        k = int(g[f'{case}/k'])
        assert torch.equal(token_ops.maxmin_select_composed(D, k), torch.from_numpy(g[f'{case}/sel'])), case
        assert torch.equal(token_ops.maxmin_select(D, k), torch.from_numpy(g[f'{case}/sel'])), case             # CPU: the same route
    for N, d, k in O.EXACT_SHAPES:
        case = f'b_{N}_{d}'
        x = torch.from_numpy(O.exact_tokens(N, d, int(g[f'{case}/seed'])))
        for name, dt in TDT.items():
            D = token_ops.cosine_distance_composed(x.to(dt))
            assert D.dtype == torch.float32 and np.array_equal(D.numpy().view(np.uint32), g[f'{case}/D'].view(np.uint32)), (case, name)
            assert torch.equal(token_ops.cosine_distance(x.to(dt)), D)
            assert torch.equal(token_ops.maxmin_select_composed(D, k), torch.from_numpy(g[f'{case}/sel_{name}']))


def test_divprune_on_cpu_tensors_returns_the_golden_indices(golden):
    from llmc_amd.compression.token_reduction.divprune import divprune
    g = golden('divprune')
    for N, d, k in O.EXACT_SHAPES:
        case = f'b_{N}_{d}'
        x = torch.from_numpy(O.exact_tokens(N, d, int(g[f'{case}/seed'])))
        for name, dt in TDT.items():
            s, D = divprune(x.to(dt), N, None, k / N)
            assert s.dtype == torch.long and torch.equal(s, torch.from_numpy(g[f'{case}/sel_{name}'])), (case, name)
            assert D.dtype == torch.float32 and tuple(D.shape) == (N, N)
    for case in (str(n) for n in g['names']):
        D = O.golden_matrix(g, case)
        k = int(g[f'{case}/k'])
        s, same = divprune(D, k, D, 1.0)
        assert same is D and torch.equal(s, torch.from_numpy(g[f'{case}/sel'])), case


def test_the_wrappers_refuse_what_the_reference_cannot_run():
    from llmc_amd.compression.token_reduction import token_ops
    with pytest.raises(ValueError, match='N = 1 < 2'):
        token_ops.maxmin_select(torch.zeros(1, 1), 1)
    with pytest.raises(ValueError, match='k = -1'):
        token_ops.maxmin_select(torch.zeros(3, 3), -1)
    with pytest.raises(ValueError, match='square'):
        token_ops.maxmin_select(torch.zeros(3, 4), 1)
    with pytest.raises(ValueError, match=r'\[N, d\]'):
        token_ops.cosine_distance(torch.zeros(3))
    assert token_ops.maxmin_select(torch.zeros(3, 3), 0).shape == (0,)
    L = __import__('llmc_amd._ffi', fromlist=['lib']).lib()
    assert L.llmc_maxmin_select_max_n() == token_ops.MAX_RESIDENT_N == 16384
    assert L.llmc_maxmin_select_ws_bytes(16384) == 4 * 16384 and L.llmc_maxmin_select_ws_bytes(16385) == 0
    assert L.llmc_cosine_dist_ws_bytes(576, 4096) == 16 * 15 * 128 * 128 * 4       # 15 upper tiles, 16 slices of 256
    assert L.llmc_cosine_dist_ws_bytes(2880, 4096) == 2 * 276 * 128 * 128 * 4
    assert L.llmc_cosine_dist_ws_bytes(46341, 8) == 0
    assert L.llmc_cosine_dist(None, 7, 1, 1, 1, None, None, None) == -22
    assert L.llmc_maxmin_select(None, 2, 1, 1, 1, None, None, None) == -22
    assert L.llmc_maxmin_select(None, 2, 4, 3, 1, None, None, None) == -22         # ldd < N
    assert L.llmc_maxmin_select(None, 2, 4, 4, 0, None, None, None) == 0           # k == 0 writes nothing
