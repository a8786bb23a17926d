"""llmc_cosine_dist and llmc_maxmin_select (csrc/token_select.hip) on the GPU: the distance kernel against the fp64 value within the
bound tests/divprune_oracle.py derives, bit for bit on the exact features, symmetric, repeatable and independent of the operand's
alignment; the selection kernel bit for bit against the oracle's select on the reference's goldens, on the distance kernel's own
output and at the sizes where a thread takes its next column; divprune() end to end on the goldens."""
import numpy as np
import pytest
import torch

import divprune_oracle as O

pytestmark = pytest.mark.gpu

TDT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}

# (N, d): one pair; below one tile with a ragged d (40 = two and a half 16-steps); across a tile edge with a ragged d and a thin
# last slice (520 = 2 x 256 + 8); model width, 16 slices; LLaVA's N: 15 tiles of which 5 hold the matrix's edge, two slices
SHAPES = [(2, 8), (33, 40), (130, 520), (300, 4096), (576, 256)]

_CASES = {}


def features(N, d, dt):
    """inputs of a shape in a dtype and their fp64 distances, computed once"""
    key = (N, d, dt)
    if key not in _CASES:
        g = torch.Generator().manual_seed(11 * N + d)
        x = (torch.randn(N, d, generator=g) * torch.exp(0.5 * torch.randn(d, generator=g))).to(TDT[dt])
        _CASES[key] = (x, O.truth_dist(x.float().numpy()))
    return _CASES[key]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def ops():
    from llmc_amd.compression.token_reduction import token_ops
    return token_ops


@pytest.mark.parametrize('dt', list(TDT))
@pytest.mark.parametrize('N,d', SHAPES)
def test_distance_kernel_within_the_derived_bound_symmetric_repeatable_and_layout_free(N, d, dt):
    x, truth = features(N, d, dt)
    xg = x.cuda()
    D = ops().cosine_distance(xg)
    assert D.dtype == torch.float32 and tuple(D.shape) == (N, N) and D.is_contiguous()
    err = np.abs(D.cpu().numpy().astype(np.float64) - truth).max()
    comp = ops().cosine_distance_composed(xg)
    diff = (D.double() - comp.double()).abs().max().item()
    print(f'{N} x {d} {dt}: |kernel - truth| {err:.3e} (bound {O.bound(d, dt):.3e}), |kernel - composed| {diff:.3e}')
    assert err <= O.bound(d, dt)
    # the composition normalises in fp32 first, so its products are rounded: its own error is the fp32 bound
    assert diff <= O.bound(d, dt) + O.bound(d, 'f32')
    assert torch.equal(bits(D), bits(D.t()))
    assert torch.equal(bits(D), bits(ops().cosine_distance(xg)))
    wide = torch.zeros(N, d + 3, dtype=x.dtype, device='cuda')          # a row stride that keeps no row but the first aligned
    wide[:, :d] = xg
    assert wide[:, :d].stride(0) == d + 3
    assert torch.equal(bits(D), bits(ops().cosine_distance(wide[:, :d])))
    flat = torch.zeros(N * d + 1, dtype=x.dtype, device='cuda')         # a view that starts one element in
    flat[1:] = xg.reshape(-1)
    off = flat[1:].view(N, d)
    assert off.data_ptr() % 16 != 0
    assert torch.equal(bits(D), bits(ops().cosine_distance(off)))


@pytest.mark.parametrize('dt', list(TDT))
def test_distance_kernel_is_bit_identical_on_the_exact_features(golden, dt):
    g = golden('divprune')
    for N, d, _ in O.EXACT_SHAPES:
        x = torch.from_numpy(O.exact_tokens(N, d, int(g[f'b_{N}_{d}/seed']))).to(TDT[dt]).cuda()
        D = ops().cosine_distance(x).cpu().numpy()
        assert np.array_equal(D.view(np.uint32), g[f'b_{N}_{d}/D'].view(np.uint32)), (N, d, np.abs(D - g[f'b_{N}_{d}/D']).max())


def test_a_zero_row_gives_nan_in_its_row_and_column_and_the_selection_still_follows_the_rules():
    x, _ = features(33, 40, 'bf16')
    x = x.clone()
    x[5] = 0
    D = ops().cosine_distance(x.cuda())
    nan = torch.isnan(D).cpu()
    want = torch.zeros(33, 33, dtype=torch.bool)
    want[5, :] = want[:, 5] = True
    assert torch.equal(nan, want)
    assert np.array_equal(ops().maxmin_select(D, 12).cpu().numpy(), O.select(D.cpu().numpy(), 12))


def test_selection_kernel_equals_select_on_every_golden_matrix(golden):
    g = golden('divprune')
    for case in (str(n) for n in g['names']):
        D = O.golden_matrix(g, case)
        k = int(g[f'{case}/k'])
        got = ops().maxmin_select(D.cuda(), k)
        assert got.dtype == torch.long and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), g[f'{case}/sel']), case
        assert np.array_equal(got.cpu().numpy(), O.select(D.float().numpy(), k)), case


@pytest.mark.parametrize('dt', list(TDT))
@pytest.mark.parametrize('N,d', SHAPES)
def test_selection_kernel_equals_select_on_the_distance_kernels_own_matrix(N, d, dt):
    x, _ = features(N, d, dt)
    D = ops().cosine_distance(x.cuda())
    k = max(1, N // 2)
    assert np.array_equal(ops().maxmin_select(D, k).cpu().numpy(), O.select(D.cpu().numpy(), k))


# (N, k, dtype): the smallest matrix; one column past a wave with k = N; a thread's second column (1025 > 1024), its third and
# its fifth
@pytest.mark.parametrize('N,k,dt', [(2, 1, 'f32'), (65, 65, 'bf16'), (1025, 40, 'f32'), (2049, 12, 'f16'), (4097, 8, 'f32')])
def test_selection_kernel_at_the_sweep_boundaries_and_with_a_row_stride(N, k, dt):
    g = torch.Generator().manual_seed(N)
    D = torch.rand(N, N, generator=g).to(TDT[dt])
    want = O.select(D.float().numpy(), k)
    assert np.array_equal(ops().maxmin_select(D.cuda(), k).cpu().numpy(), want)
    wide = torch.full((N, N + 5), float('nan'), dtype=D.dtype, device='cuda')          # ldd > N: what lies behind a row is not read
    wide[:, :N] = D.cuda()
    assert np.array_equal(ops().maxmin_select(wide[:, :N], k).cpu().numpy(), want)
    assert np.array_equal(ops().maxmin_select(D.cuda(), k + N).cpu().numpy()[:k], want)          # k > N is legal


@pytest.mark.parametrize('N,k', [(8193, 6), (16384, 4)])
def test_selection_kernel_at_a_threads_ninth_and_last_column_against_the_loop_on_distinct_values(N, k):
    """Every thread's loop over its columns is one unrolled body with a guard, so the sizes above cover its paths; these two are the
    sizes a numpy oracle is too slow for: a thread's ninth column and the largest resident N. All N * N values are distinct
    (a permutation of 0 .. N * N - 1 as the bit patterns of positive floats, whose order is the integers'), so no step can tie
    and the reference's loop from torch ops on the GPU, checked on the goldens above, has one possible answer."""
    perm = torch.randperm(N * N, device='cuda', generator=torch.Generator('cuda').manual_seed(N))
    D = (perm.to(torch.int32) + 0x30000000).view(torch.float32).reshape(N, N)
    del perm
    got = ops().maxmin_select(D, k)
    assert torch.equal(got, ops().maxmin_select_composed(D, k))
    assert int(got.max()) < N and int(got.min()) >= 0


def test_more_columns_than_stay_resident_take_the_composed_route_and_say_so(capsys):
    N = ops().MAX_RESIDENT_N + 1
    D = torch.rand(N, N, dtype=torch.float16, device='cuda', generator=torch.Generator('cuda').manual_seed(1))
    got = ops().maxmin_select(D, 2)
    again = ops().maxmin_select(D, 2)
    err = capsys.readouterr().err
    assert err.count('maxmin_select') == 1 and f'more than {N - 1} columns' in err and 'torch ops' in err
    assert torch.equal(got, ops().maxmin_select_composed(D, 2)) and torch.equal(got, again)
    with pytest.raises(NotImplementedError, match='16384'):
        from llmc_amd import _ffi
        ws = torch.empty(4 * N, dtype=torch.uint8, device='cuda')
        _ffi.check(_ffi.lib().llmc_maxmin_select(D.data_ptr(), _ffi.dt(D), N, N, 2, got.data_ptr(), ws.data_ptr(), _ffi.stream()), 'x')


@pytest.mark.parametrize('dt', list(TDT))
def test_divprune_end_to_end_returns_the_golden_indices(golden, dt):
    from llmc_amd.compression.token_reduction.divprune import divprune
    g = golden('divprune')
    for N, d, k in O.EXACT_SHAPES:
        case = f'b_{N}_{d}'
        x = torch.from_numpy(O.exact_tokens(N, d, int(g[f'{case}/seed']))).to(TDT[dt]).cuda()
        s, D = divprune(x, N, None, k / N)
        assert s.is_cuda and D.is_cuda and D.dtype == torch.float32
        assert np.array_equal(s.cpu().numpy(), g[f'{case}/sel_{dt}']), case
    for name in ('sym', 'asym', 'ties', 'nan', 'dup', 'full'):
        case = f'a_{name}_{dt}'
        D = O.golden_matrix(g, case).cuda()
        k = int(g[f'{case}/k'])
        s, same = divprune(D, k, D, 1.0)
        assert same is D and np.array_equal(s.cpu().numpy(), g[f'{case}/sel']), case
