"""The pruning kernels (csrc/prune.hip through sparse_ops) against tests/sparse_oracle.py on the GPU: exact equality of bit
patterns and masks on every launch path, at ties, n:m groups, NaN / inf / signed zeros, padded and unaligned views; the column
sums of squares exactly on small integers and within the fp32 summation bound on random data; the golden cases of the
reference."""
import numpy as np
import pytest
import torch

import sparse_oracle as O
from conftest import load_golden, report

pytestmark = pytest.mark.gpu

DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
SENTINEL = 7.0


def ops():
    from llmc_amd.compression.sparsification import sparse_ops
    return sparse_ops


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rand_w(g, R, K, dt):
    return (torch.randn(R, K, generator=g) * 0.05).to(dt)


def rand_scaler(g, K):
    return torch.exp(torch.randn(K, generator=g)) ** 2


def gpu_view(w, ld=None, offset=0):
    """w [R, K] on the CPU -> (a GPU view with the same values, row stride ld, `offset` elements into its storage; the buffer)"""
    R, K = w.shape
    ld = K if ld is None else ld
    buf = torch.full((R * ld + offset,), SENTINEL, dtype=w.dtype, device='cuda')
    view = buf[offset:].view(R, ld)[:, :K]
    view.copy_(w)
    return view, buf


def check_rows(w, scaler, n_prune, m=None, ld=None, offset=0, path=None):
    S = ops()
    view, buf = gpu_view(w, ld, offset)
    if path is not None:
        assert S.path(view, m) == path
    s = None if scaler is None else scaler.cuda()
    mask = S.prune_rows(view, s, n_prune, m, want_mask=True)
    want, want_mask = O.prune_rows(w, scaler, n_prune, m)
    assert torch.equal(O.bits(view.cpu()), O.bits(want)), (tuple(w.shape), n_prune, m)
    assert torch.equal(mask.cpu(), want_mask)
    R, K = w.shape
    if ld is not None and ld > K:
        pad = buf[offset:].view(R, ld)[:, K:]
        assert bool((pad == SENTINEL).all()), 'padding columns were touched'
    if offset:
        assert bool((buf[:offset] == SENTINEL).all())


# (K, ld, offset in elements) -> the path per dtype
ROW_CASES = [
    (64, None, 0, {'bf16': 'wave', 'f16': 'wave', 'f32': 'wave'}),
    (256, None, 0, {'bf16': 'wave', 'f16': 'wave', 'f32': 'wave'}),
    (250, None, 0, {'bf16': 'scalar', 'f16': 'scalar', 'f32': 'scalar'}),
    (250, 256, 0, {'bf16': 'scalar', 'f16': 'scalar', 'f32': 'scalar'}),
    (256, 264, 0, {'bf16': 'wave', 'f16': 'wave', 'f32': 'wave'}),
    (256, None, 1, {'bf16': 'scalar', 'f16': 'scalar', 'f32': 'scalar'}),
    (2048, None, 0, {'bf16': 'wave', 'f16': 'wave', 'f32': 'block256'}),
    (4096, None, 0, {'bf16': 'block256', 'f16': 'block256', 'f32': 'block256'}),
    (4096, 4104, 0, {'bf16': 'block256', 'f16': 'block256', 'f32': 'block256'}),
    (4098, None, 0, {'bf16': 'scalar', 'f16': 'scalar', 'f32': 'scalar'}),
    (14336, None, 0, {'bf16': 'block1024', 'f16': 'block1024', 'f32': 'block1024'}),
    (28672, None, 0, {'bf16': 'block1024', 'f16': 'block1024', 'f32': 'block1024'}),
]


@pytest.mark.parametrize('dname', list(DTYPES))
@pytest.mark.parametrize('K,ld,offset,paths', ROW_CASES, ids=lambda v: str(v) if not isinstance(v, dict) else '')
def test_prune_rows_per_row_matches_the_stable_sort(K, ld, offset, paths, dname):
    dt = DTYPES[dname]
    g = gen(K * 7 + (ld or 0) + offset)
    scaler = rand_scaler(g, K)
    for R in ((1, 5) if K >= 14336 else (1, 5, 130)):
        w = rand_w(g, R, K, dt)
        for n_prune in (0, 1, int(K * 0.3), K // 2, K - 1, K):
            check_rows(w, scaler, n_prune, None, ld, offset, paths[dname])
    check_rows(rand_w(g, 3, K, dt), None, K // 2, None, ld, offset, paths[dname])          # null scaler_row: the multiplier 1


def test_every_per_row_path_is_hit_by_name():
    assert {p for *_, paths in ROW_CASES for p in paths.values()} == {'wave', 'block256', 'block1024', 'scalar'}


def test_a_row_past_the_residency_limit_takes_the_announced_composition(capfd):
    S = ops()
    K = S.MAX_RESIDENT_K + 8
    g = gen(5)
    w, scaler = rand_w(g, 2, K, torch.bfloat16), rand_scaler(g, K)
    view, _ = gpu_view(w)
    assert S.path(view) == 'composed'
    S._FALLBACK_SEEN.clear()
    mask = S.prune_rows(view, scaler.cuda(), K // 2, want_mask=True)
    assert 'does not stay resident' in capfd.readouterr().err
    want, want_mask = O.prune_rows(w, scaler, K // 2)
    assert torch.equal(O.bits(view.cpu()), O.bits(want)) and torch.equal(mask.cpu(), want_mask)


def test_the_composition_equals_the_kernel():
    S = ops()
    g = gen(6)
    w, scaler = rand_w(g, 9, 512, torch.bfloat16), rand_scaler(g, 512)
    for m, n in ((None, 200), (4, 2)):
        a, _ = gpu_view(w)
        b, _ = gpu_view(w)
        ma = S.prune_rows(a, scaler.cuda(), n, m, want_mask=True)
        mb = S.prune_rows_composed(b, scaler.cuda(), n, m, want_mask=True)
        assert torch.equal(O.bits(a), O.bits(b)) and torch.equal(ma, mb)


# ---- ties ------------------------------------------------------------------------------------------------------------------------
TIE_SHAPES = [(256, None, 'wave'), (250, None, 'scalar'), (1002, None, 'scalar'), (1024, None, 'wave'), (4096, None, 'block256'),
              (14336, None, 'block1024'), (16384, 16385, 'scalar')]
VALUES7 = torch.tensor([-0.5, -0.25, 0.0, 0.125, 0.25, 0.5, 1.0])


def tie_counts(K):
    return (1, K // 3, K // 2, K - 1)


@pytest.mark.parametrize('dname', list(DTYPES))
@pytest.mark.parametrize('K,ld,path', TIE_SHAPES)
def test_ties_go_by_lower_column(K, ld, path, dname):
    dt = DTYPES[dname]
    g = gen(K + 11)
    R = 5 if K <= 4096 else 2
    w7 = VALUES7[torch.randint(7, (R, K), generator=g)].to(dt)
    ones = torch.ones(K)
    two = torch.ones(K)
    two[torch.rand(K, generator=g) < 0.5] = 4.0
    for n_prune in tie_counts(K):
        check_rows(w7, ones, n_prune, None, ld, 0, path)          # the threshold bucket holds about a seventh of the row
        check_rows(w7, two, n_prune, None, ld, 0, path)           # and straddles n_prune under a two-valued scaler_row
    flat = torch.full((R, K), 0.375).to(dt)
    flat[1:] *= -1
    for n_prune in tie_counts(K):
        check_rows(flat, ones, n_prune, None, ld, 0, path)        # rows that are all equal
    # metric-0 ties: zero scaler entries and signed zeros in W, pruned in column order
    wz = rand_w(g, R, K, dt)
    wz[torch.rand(R, K, generator=g) < 0.3] = 0.0
    wz[torch.rand(R, K, generator=g) < 0.2] = -0.0
    sz = rand_scaler(g, K)
    sz[torch.rand(K, generator=g) < 0.4] = 0.0
    for n_prune in tie_counts(K):
        check_rows(wz, sz, n_prune, None, ld, 0, path)


@pytest.mark.parametrize('dname', list(DTYPES))
@pytest.mark.parametrize('K,path', [(256, 'wave'), (250, 'scalar'), (4096, 'block256')])
def test_nan_sorts_last_and_kept_elements_keep_their_bits(K, path, dname):
    dt = DTYPES[dname]
    g = gen(K + 3)
    w = rand_w(g, 4, K, dt)
    w[:, 5] = float('inf')
    w[:, 9] = float('-inf')
    w[:, 17] = float('nan')
    w[0, 40] = -float('nan')
    w[:, 23] = -0.0
    scaler = rand_scaler(g, K)
    scaler[9] = 0.0          # inf * 0: a NaN metric
    scaler[60] = float('inf')
    w[:, 60] = 0.0           # 0 * inf as well
    w[:, 61] = 0.0
    for n_prune in (1, K // 2, K - 5, K - 4, K - 3, K - 2, K - 1, K):
        check_rows(w, scaler, n_prune, None, None, 0, path)
    # NaN payloads survive where kept
    iw = O.bits(w).clone()
    iw[1, 17] = iw[1, 17] | 1
    w2 = iw.view(dt)
    check_rows(w2, scaler, K // 2, None, None, 0, path)


# ---- n:m -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dname', list(DTYPES))
@pytest.mark.parametrize('n,m', [(2, 4), (1, 4), (4, 8), (1, 2), (8, 16)])
def test_n_m_groups(n, m, dname):
    dt = DTYPES[dname]
    S = ops()
    g = gen(100 * n + m)
    seen = set()
    for K in (m, 256, 4096 + m):
        scaler = rand_scaler(g, K)
        for R in (1, 37):
            w = rand_w(g, R, K, dt)
            view, _ = gpu_view(w)
            seen.add(S.path(view, m))
            check_rows(w, scaler, n, m)
            check_rows(VALUES7[torch.randint(7, (R, K), generator=g)].to(dt), torch.ones(K), n, m)          # ties inside groups
        check_rows(rand_w(g, 3, K, dt), scaler, 0, m)
        check_rows(rand_w(g, 3, K, dt), None, m, m)
    check_rows(rand_w(g, 5, 256, dt), rand_scaler(g, 256), n, m, 264, 0, 'nm')
    check_rows(rand_w(g, 5, 256, dt), rand_scaler(g, 256), n, m, None, 1, 'nm_scalar')
    assert seen <= {'nm', 'nm_scalar', 'wave', 'scalar'} and 'nm' in seen          # K == m is the per-row mode


def test_both_n_m_paths_are_hit_by_name():
    S = ops()
    assert S.path(torch.empty(3, 256, dtype=torch.bfloat16, device='cuda'), 4) == 'nm'
    assert S.path(torch.empty(3, 4100, dtype=torch.bfloat16, device='cuda'), 4) == 'nm_scalar'
    assert S.path(torch.empty(3, 4098, dtype=torch.float32, device='cuda'), 2) == 'nm_scalar'


# ---- column sums of squares ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dname', list(DTYPES))
def test_col_sqsum_is_exact_on_small_integers(dname):
    dt = DTYPES[dname]
    S = ops()
    g = gen(21)
    for N in (1, 63, 64, 65, 2051):
        for K in (1, 8, 250, 4096):
            x = torch.randint(-8, 9, (N, K), generator=g).to(dt)
            want = O.col_sqsum64(x)
            acc, out = S.col_sqsum(x.cuda(), nsamples=3)
            assert torch.equal(acc.cpu().double(), want), (N, K)
            assert torch.equal(out.cpu(), want.float() / 3.0)
            # folding two batches equals one call on their concatenation
            cut = N // 2
            if cut:
                acc2 = S.col_sqsum(x[:cut].cuda())
                S.col_sqsum(x[cut:].cuda(), acc2, init=False)
                assert torch.equal(acc2, acc)
    x3 = torch.randint(-8, 9, (3, 20, 64), generator=g).to(dt)          # leading axes are flattened
    assert torch.equal(S.col_sqsum(x3.cuda()).cpu().double(), O.col_sqsum64(x3))
    off = torch.randint(-8, 9, (65 * 64 + 1,), generator=g).to(dt)      # an unaligned X takes scalar loads, same sums
    xo = off.cuda()[1:].view(65, 64)
    assert torch.equal(S.col_sqsum(xo).cpu().double(), O.col_sqsum64(off[1:].view(65, 64)))


def test_col_sqsum_is_deterministic_and_within_the_fp32_summation_bound():
    S = ops()
    g = gen(22)
    N, K = 2048, 1024
    x = (torch.randn(N, K, generator=g) * torch.exp(torch.randn(K, generator=g))).to(torch.bfloat16)
    xd = x.cuda()
    a, b = S.col_sqsum(xd), S.col_sqsum(xd)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    want = O.col_sqsum64(x)
    rel = ((a.cpu().double() - want).abs() / want).max().item()
    bound = (N + 1) * 2.0 ** -24          # any order of an fp32 sum of N rounded non-negative terms
    report('test_col_sqsum_is_deterministic_and_within_the_fp32_summation_bound', rel_err=rel, bound=bound)
    assert rel <= bound
    for dt in (torch.float16, torch.float32):
        y = torch.randn(777, 250, generator=g).to(dt).cuda()
        assert torch.equal(S.col_sqsum(y).view(torch.int32), S.col_sqsum(y).view(torch.int32))


@pytest.mark.parametrize('N,K,dname', O.SQSUM_ORDER_CASES)
def test_col_sqsum_adds_in_the_order_the_header_promises(N, K, dname):
    """bit for bit against O.col_sqsum_ordered, the numpy restatement of include/llmc_hip.h's order, on inputs on which other
    orders give other bits (test_sparse_oracle.py)"""
    dt = DTYPES[dname]
    S = ops()
    x = O.sqsum_order_input(N, K, dt)
    want = O.col_sqsum_ordered(x, dt)
    acc, out = S.col_sqsum(x.cuda(), nsamples=7)
    assert torch.equal(O.bits(acc.cpu()), O.bits(want)), (N, K, dname)
    assert torch.equal(O.bits(out.cpu()), O.bits(want / 7.0))


@pytest.mark.parametrize('dname', ['bf16', 'f32'])
def test_col_sqsum_keeps_its_order_on_scalar_loads_and_folds_a_second_batch(dname):
    dt = DTYPES[dname]
    S = ops()
    # the same data at an address that is no multiple of 16 bytes: other loads, the same order
    x = O.sqsum_order_input(130, 64, dt)
    want = O.col_sqsum_ordered(x, dt)
    buf = torch.empty(130 * 64 + 1, dtype=dt, device='cuda')
    view = buf[1:].view(130, 64)
    view.copy_(x)
    assert view.data_ptr() % 16 != 0
    assert torch.equal(O.bits(S.col_sqsum(view).cpu()), O.bits(want))
    assert torch.equal(O.bits(S.col_sqsum(x.cuda()).cpu()), O.bits(want))
    # a K that is no whole number of vectors: scalar loads again, and the chunk count still takes the dtype's vector width
    y = O.sqsum_order_input(300, 70, dt, seed=32)
    first = O.col_sqsum_ordered(y, dt)
    acc = S.col_sqsum(y.cuda())
    assert torch.equal(O.bits(acc.cpu()), O.bits(first))
    # init=False: acc + batch, one fp32 add, and out = acc / float32(nsamples)
    z = O.sqsum_order_input(65, 70, dt, seed=33)
    acc2, out = S.col_sqsum(z.cuda(), acc, init=False, nsamples=3)
    assert acc2 is acc
    both = first + O.col_sqsum_ordered(z, dt)
    assert torch.equal(O.bits(acc.cpu()), O.bits(both))
    assert torch.equal(O.bits(out.cpu()), O.bits(both / 3.0))


# ---- global magnitude pruning ----------------------------------------------------------------------------------------------------
MAG_CASES = [('bf16', 384, 256, None, 0), ('f16', 384, 256, None, 0), ('f32', 64, 250, None, 0), ('f32', 64, 256, None, 0),
             ('bf16', 384, 256, 264, 0), ('f32', 64, 256, 260, 0), ('f16', 100, 250, 251, 0), ('bf16', 384, 256, None, 1)]


@pytest.mark.parametrize('dname,R,K,ld,offset', MAG_CASES)
def test_magnitude_prune_matches_the_sorted_threshold(dname, R, K, ld, offset):
    dt = DTYPES[dname]
    S = ops()
    g = gen(R + K)
    w = rand_w(g, R, K, dt)
    w[0, :7] = 0.0
    w[1, :7] = -0.0
    if dname == 'f32':
        w[2] = w[3]          # fp32 ties
    numel = R * K
    for kth in (0, numel // 2, numel - 1, int(numel * 0.3)):
        view, buf = gpu_view(w, ld, offset)
        thresh, mask = S.magnitude_prune(view, kth, want_mask=True)
        want, want_thresh, want_mask = O.magnitude_prune(w, kth)
        assert torch.equal(O.bits(thresh.reshape(1).cpu()), O.bits(want_thresh.reshape(1))), kth
        assert torch.equal(mask.cpu(), want_mask)
        assert torch.equal(O.bits(view.cpu()), O.bits(want))
        assert int(mask.sum()) >= kth + 1
        if ld is not None:
            assert bool((buf[offset:].view(R, ld)[:, K:] == SENTINEL).all())


def test_magnitude_prune_refuses_sparsity_one():
    S = ops()
    w = torch.zeros(4, 64, dtype=torch.bfloat16, device='cuda')
    with pytest.raises(ValueError, match='kth'):
        S.magnitude_prune(w, 256)


# ---- the reference's own results -------------------------------------------------------------------------------------------------
def golden_tensor(arr, dt):
    if dt == torch.float32:
        return torch.from_numpy(arr.view(np.int32).copy()).view(torch.float32)
    return torch.from_numpy(arr.view(np.int16).copy()).view(dt)


def golden_dtype(name):
    return next((dt for k, dt in DTYPES.items() if f'_{k}' in name), torch.bfloat16)


def test_prune_rows_reproduces_the_reference_given_its_scaler_row():
    S = ops()
    G = load_golden('sparse')
    for name in (str(n) for n in G['wanda_names']):
        dt = golden_dtype(name)
        w = golden_tensor(G[f'{name}/w_bits'], dt).cuda()
        scaler = torch.from_numpy(G[f'{name}/scaler_row'].copy()).cuda()
        mask = S.prune_rows(w, scaler, int(G[f'{name}/n_prune']), want_mask=True)
        want = G[f'{name}/pruned_bits']
        assert np.array_equal(O.bits(w.cpu()).numpy().view(want.dtype), want), name
        if f'{name}/mask' in G.files:
            assert np.array_equal(mask.cpu().numpy(), G[f'{name}/mask'])
        # and our own statistic is the reference's up to the order of two fp32 sums of N = 60 terms ((N + 1) * 2^-24 each,
        # the bound of the summation test) and the roundings of the reference's sqrt(...) ** 2 (at most 4 * 2^-24)
        act = golden_tensor(G[f'{name}/act_bits'], dt).cuda()
        _, mine = S.col_sqsum(act, nsamples=act.shape[0])
        ref = torch.from_numpy(G[f'{name}/scaler_row'].copy())
        n_tok = act.shape[0] * act.shape[1]
        assert ((mine.cpu() - ref).abs() <= (2 * (n_tok + 1) + 4) * 2.0 ** -24 * ref).all()


def test_magnitude_prune_reproduces_the_reference():
    S = ops()
    G = load_golden('sparse')
    for name in (str(n) for n in G['magnitude_names']):
        dt = golden_dtype(name)
        w = golden_tensor(G[f'{name}/w_bits'], dt).cuda()
        thresh, mask = S.magnitude_prune(w, int(G[f'{name}/kth']), want_mask=True)
        want = G[f'{name}/pruned_bits']
        assert np.array_equal(O.bits(w.cpu()).numpy().view(want.dtype), want), name
        assert np.array_equal(O.bits(thresh.reshape(1).cpu()).numpy().view(want.dtype), G[f'{name}/thresh_bits'])
        assert np.array_equal(mask.cpu().numpy(), G[f'{name}/mask'])
