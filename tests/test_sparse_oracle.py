"""tests/sparse_oracle.py, the plain torch restatement the pruning kernels are tested against, reproduces the reference's own
results (tests/golden/sparse.npz, written by tools/make_golden_sparse.py from the reference on CPU) bit for bit."""
import numpy as np
import pytest
import torch

import sparse_oracle as O
from conftest import load_golden

DT = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}


def tensor(arr, dt):
    if dt == torch.float32:
        return torch.from_numpy(arr.view(np.int32).copy()).view(torch.float32)
    return torch.from_numpy(arr.view(np.int16).copy()).view(dt)


def case_dtype(name):
    return next((dt for k, dt in DT.items() if f'_{k}' in name), torch.bfloat16)


def np_bits(t):
    return O.bits(t).numpy()


G = load_golden('sparse')
WANDA = [str(n) for n in G['wanda_names']]
MAGNITUDE = [str(n) for n in G['magnitude_names']]


def test_the_golden_file_holds_the_cases_the_tool_writes():
    assert len(WANDA) == 7 and 'wanda_ties' in WANDA and len(MAGNITUDE) == 3


@pytest.mark.parametrize('name', WANDA)
def test_row_scale_and_selection_reproduce_the_reference(name):
    dt = case_dtype(name)
    w, act = tensor(G[f'{name}/w_bits'], dt), tensor(G[f'{name}/act_bits'], dt)
    scaler = O.row_scale(act)
    assert np.array_equal(scaler.numpy().view(np.uint32), G[f'{name}/scaler_row'].view(np.uint32))
    n_prune = int(G[f'{name}/n_prune'])
    assert n_prune == int(w.shape[1] * float(G[f'{name}/sparsity']))
    out, mask = O.prune_rows(w, scaler, n_prune)
    want = G[f'{name}/pruned_bits']
    assert np.array_equal(np_bits(out).view(want.dtype), want)
    assert (mask.sum(1) == n_prune).all()
    if f'{name}/mask' in G.files:
        assert np.array_equal(mask.numpy(), G[f'{name}/mask'])


def test_the_tie_case_is_decided_by_the_stable_sort():
    """the 7-valued weights under a two-valued norm: some row's threshold metric is shared by pruned and kept elements"""
    name = 'wanda_ties'
    w = tensor(G[f'{name}/w_bits'], torch.bfloat16)
    scaler = torch.from_numpy(G[f'{name}/scaler_row'].copy())
    n_prune = int(G[f'{name}/n_prune'])
    m = O.metric(w, scaler)
    _, mask = O.prune_rows(w, scaler, n_prune)
    straddled = 0
    for r in range(w.shape[0]):
        cut, kept = m[r][mask[r] == 1], m[r][mask[r] == 0]
        if cut.max() == kept.min():
            straddled += 1
            tie = m[r] == cut.max()
            idx_cut = torch.nonzero(tie & (mask[r] == 1)).flatten()
            idx_kept = torch.nonzero(tie & (mask[r] == 0)).flatten()
            assert idx_cut.max() < idx_kept.min()          # lower column first
    assert straddled >= w.shape[0] // 2


@pytest.mark.parametrize('name', MAGNITUDE)
def test_magnitude_reproduces_the_reference(name):
    dt = case_dtype(name)
    w = tensor(G[f'{name}/w_bits'], dt)
    out, thresh, mask = O.magnitude_prune(w, int(G[f'{name}/kth']))
    want = G[f'{name}/pruned_bits']
    assert np.array_equal(np_bits(out).view(want.dtype), want)
    assert np.array_equal(np_bits(thresh.reshape(1)).view(want.dtype), G[f'{name}/thresh_bits'])
    assert np.array_equal(mask.numpy(), G[f'{name}/mask'])
    assert int(mask.sum()) >= int(G[f'{name}/kth']) + 1


@pytest.mark.parametrize('N,K,dname', O.SQSUM_ORDER_CASES)
def test_the_ordered_column_sum_tells_its_order_from_others(N, K, dname):
    """col_sqsum_ordered on the inputs of the GPU order test: another order of the same fp32 adds gives other bits there, so a
    kernel that passes the GPU test has the header's order and not merely a sum within the fp32 bound."""
    dt = DT[dname]
    x = O.sqsum_order_input(N, K, dt)
    want = O.col_sqsum_ordered(x, dt)
    assert want.dtype == torch.float32 and want.shape == (K,)
    f = x.float().numpy()
    plain = np.zeros(K, dtype=np.float32)
    for r in range(N):
        plain = plain + f[r] * f[r]
    if N > 4:          # up to four rows, one per wave: ((x0 + x1) + x2) + x3 is the row order
        assert (plain != want.numpy()).any()
    else:
        assert np.array_equal(plain, want.numpy())
    assert not torch.equal(O.col_sqsum_ordered(x, dt, waves=2), want)
    if K == 262144:          # the block cap binds: the chunk count depends on the vector width
        assert not torch.equal(O.col_sqsum_ordered(x, dt, v=8), want)


def test_n_m_groups_and_nan_order():
    w = torch.tensor([[0.5, -0.5, 0.25, float('nan'), float('inf'), 1.0, -0.0, 0.0]])
    out, mask = O.prune_rows(w, None, 2, 4)
    assert mask.tolist() == [[1, 0, 1, 0, 0, 0, 1, 1]]          # 0.5 / -0.5 tie: lower column; NaN after 0.5; -0 and +0 tie
    out, mask = O.prune_rows(w, None, 7)
    assert mask.tolist() == [[1, 1, 1, 0, 1, 1, 1, 1]]          # NaN sorts last
    lo, hi = O.selection_boundary64(torch.tensor([[1.0, 3.0, 2.0, 4.0]], dtype=torch.float64), 2)
    assert lo[0, 0] == 2.0 and hi[0, 0] == 3.0
