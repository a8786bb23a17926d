"""k_spqr_block / llmc_spqr_quantize (llmc_amd/csrc/spqr_loop.hip) where tests/test_spqr_gpu.py does not reach: a ragged last
block (K % 128 != 0, K < 128), groups whose min / max is held by several columns when the detection looks at them, dead
columns, the threshold's edges, other bit widths, row counts around the 16-row workgroup, model widths (K = 4096, 14336, 1600)
and quantize_stacked on three layers that share a factor. The inputs are tests/spqr_cases.py's, whose conditions (outliers
found but a minority, ties present and deciding) tests/test_spqr_cases.py proves on the CPU. Every comparison with the oracle
(oracle/spqr_ref.py + csrc/spqr_canon.c, pinned to the reference's goldens) is bit for bit."""
import math

import numpy as np
import pytest
import torch

import spqr_cases as C
from oracle import spqr_ref as S

pytestmark = pytest.mark.gpu
KEYS = ('mask', 'scales', 'zeros', 'tmp', 'losses')


def run_loop(Wp, U, g, thr, simp=False, bit=4, scale_bit=3, zero_bit=3):
    """spqr_quantize on copies (W is overwritten) -> dict of host arrays with the oracle's keys. Wp / U: numpy or device tensors."""
    from llmc_amd.compression.quantization.spqr import SpqrConfig, spqr_quantize
    cfg = SpqrConfig(bit=bit, group_size=g, simplified_outliers=simp, scale_bit=scale_bit, zero_bit=zero_bit)
    Wd = torch.from_numpy(np.array(Wp, dtype=np.float32, order='C')).cuda() if isinstance(Wp, np.ndarray) else Wp.clone()
    Ud = torch.from_numpy(np.array(U, dtype=np.float32, order='C')).cuda() if isinstance(U, np.ndarray) else U
    tmp, losses, mask, s, z = spqr_quantize(Wd, Ud, cfg, thr)
    return dict(tmp=tmp.cpu().numpy(), losses=losses.cpu().numpy(), mask=mask.cpu().numpy(), scales=s.cpu().numpy(),
                zeros=z.cpu().numpy())


def assert_same(got, ref, rows=None, what=''):
    for k in KEYS:
        np.testing.assert_array_equal(got[k] if rows is None else got[k][rows], ref[k], err_msg=f'{what} {k}')


def check(Wp, U, g, thr, simp=False, bit=4, scale_bit=3, zero_bit=3, outliers=True, what=''):
    """the comparison rule: kernel == oracle on mask, scales, zeros, tmp, losses; with `outliers` the oracle's mask is neither
    empty nor more than half (asserted on the oracle, not on the kernel)."""
    ref = S.weight_transform(Wp, U, bit, g, thr, simp, scale_bit, zero_bit)
    if outliers:
        assert C.mask_share_ok(ref['mask']), (what, int(ref['mask'].sum()))
    got = run_loop(Wp, U, g, thr, simp, bit, scale_bit, zero_bit)
    assert_same(got, ref, what=what)
    return got, ref


# ---- A ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', C.MODES)
@pytest.mark.parametrize('R,K,g,rel', C.RAGGED)
def test_ragged_last_block_bit_exact(R, K, g, rel, mode):
    """`count < 128`: the guarded load of the U tile, d = 1 on the padding columns, skipped group starts, column steps on
    padding with the last group's (s, z), the guarded final writes; K < 128 has no trailing update."""
    Wp, U = C.general(R, K)
    thr, simp = C.mode_args(mode, Wp, U, rel)
    check(Wp, U, g, thr, simp, outliers=mode != 'inf', what=f'{R}x{K} g{g} {mode}')


# ---- B ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', C.GRID_U)
@pytest.mark.parametrize('R,K,g', C.GRID)
def test_grid_weights_with_duplicated_extremes_bit_exact(R, K, g, kind):
    """B1: a quarter of the groups hold their min (max) more than once; the leave-one-out min / max of a column that holds one
    copy is the extreme itself (Ext2's multiplicity). With the diagonal U every group is detected as written."""
    Wp, U = C.grid(R, K, g, kind)
    check(Wp, U, g, C.threshold(Wp, U, C.GRID_THR), what=f'grid g{g} {kind}')


@pytest.mark.parametrize('g', [16, 32])
def test_planted_groups_bit_exact(g):
    """B2: constant groups, two-valued groups, unique extremes in lane 0, lane 15 and the second register, extremes held
    twice (once with both copies in columns of large d, where nothing but the count of copies keeps them unflagged),
    +0.0 / -0.0 mixes."""
    Wp, U, where = C.planted(g)
    thr = C.threshold(Wp, U, C.PLANT_THR)
    got, ref = check(Wp, U, g, thr, what=f'planted g{g}')
    for r, groups in where.items():                      # per plant, so that a failure names it
        for q in groups:
            for k in ('scales', 'zeros'):
                assert got[k][r, q] == ref[k][r, q], (C.PLANTS[r % len(C.PLANTS)], k)


def factor_on_gpu(W, H, actorder, g):
    from llmc_amd.compression.quantization.spqr import SpqrConfig, spqr_factor
    cfg = SpqrConfig(bit=4, group_size=g, actorder=actorder, percdamp=1.0)
    perm, Wp, U, info = spqr_factor(H, W, cfg)
    assert int(info.item()) == 0
    return perm, Wp, U


@pytest.mark.parametrize('actorder', [True, False])
def test_dead_columns_from_the_product_factor_bit_exact(actorder):
    """B3: 40 of 384 input channels are zero in X; spqr_factor zeroes their weight columns and leaves d = 1 there. With
    actorder they fill the last group and a quarter of the one before (a constant group of zeros), without it they are spread."""
    R, K, g = C.DEAD_SHAPE
    W, H, dead = C.dead_inputs(R, K, C.DEAD_N)
    perm, Wp, U = factor_on_gpu(torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda(), actorder, g)
    at = dead if perm is None else np.flatnonzero(np.isin(perm.cpu().numpy(), dead))
    Wh, Uh = Wp.cpu().numpy(), U.cpu().numpy()
    assert len(at) == C.DEAD_N and not Wh[:, at].any() and np.abs(np.diag(Uh)[at] - 1.0).max() <= 1e-6
    assert (np.abs(Wh).sum(0) == 0).sum() == C.DEAD_N
    check(Wh, Uh, g, C.threshold(Wh, Uh, C.DEAD_REL), what=f'dead actorder={actorder}')


# ---- C ------------------------------------------------------------------------------------------------------------------------------

def test_threshold_edges_bit_exact():
    """thr = 0 and a tiny threshold (almost everything is an outlier; first groups with EVERY column flagged, `n_keep < 1`:
    tests/test_spqr_cases.py), a huge finite one (the detection runs and must flag nothing: the GPU's own inf output, bit
    for bit) and the two sides of `finite = !(threshold > 3.0e38f)`."""
    R, K, g = C.EDGE_SHAPE
    Wp, U = C.general(R, K)
    for thr in (0.0, C.threshold(Wp, U, C.TINY_REL)):
        _, ref = check(Wp, U, g, thr, outliers=False, what=f'thr {thr}')
        assert ref['mask'].mean() > 0.9
    inf = run_loop(Wp, U, g, math.inf)
    assert_same(inf, S.weight_transform(Wp, U, 4, g, math.inf, False), what='inf')
    for thr in (1e30, C.CUT_BELOW, C.CUT_ABOVE):
        got, ref = check(Wp, U, g, thr, outliers=False, what=f'thr {thr}')
        assert ref['mask'].sum() == 0
        assert_same(got, inf, what=f'thr {thr} against the inf run')


# ---- D ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('bit', C.BITS)
def test_weight_bit_widths_bit_exact(bit):
    R, K, g = C.EDGE_SHAPE
    Wp, U = C.general(R, K)
    check(Wp, U, g, C.threshold(Wp, U, C.bit_rel(bit)), bit=bit, what=f'bit {bit}')


@pytest.mark.parametrize('scale_bit,zero_bit', C.SECOND_LEVEL_BITS)
def test_second_level_bit_widths_bit_exact(scale_bit, zero_bit):
    R, K, g = C.EDGE_SHAPE
    Wp, U = C.general(R, K)
    check(Wp, U, g, C.threshold(Wp, U, C.EDGE_REL), scale_bit=scale_bit, zero_bit=zero_bit, what=f'second level {scale_bit}/{zero_bit}')


# ---- E ------------------------------------------------------------------------------------------------------------------------------

def test_row_counts_around_the_workgroup_bit_exact():
    """R = 1, 15, 16, 17, 63, 65: a lone row, one short of / exactly / one over a workgroup, one short of / over four. The
    inactive rows of the last workgroup read row R - 1 and must write nothing."""
    Wp, U, thr = C.rows_input()
    ref = S.weight_transform(Wp, U, 4, 16, thr, False)
    for R in C.ROWS:
        assert C.mask_share_ok(ref['mask'][:R])
        got = run_loop(np.ascontiguousarray(Wp[:R]), U, 16, thr)
        assert_same(got, {k: ref[k][:R] for k in KEYS}, what=f'R = {R}')


def test_spqr_quantize_refuses_a_layout_it_would_misread():
    """W[:, perm] of a numpy array is column-major, and torch.from_numpy keeps that: the kernel reads row-major memory, so a
    transposed view, a wrong dtype or a U of another size is an error and nothing is computed on the wrong elements."""
    from llmc_amd.compression.quantization.spqr import SpqrConfig, spqr_quantize
    Wp, U, thr = C.rows_input()
    cfg = SpqrConfig(bit=4, group_size=16)
    Wd, Ud = torch.from_numpy(Wp.copy()).cuda(), torch.from_numpy(U.copy()).cuda()
    for w, u in ((Wd.T.contiguous().T, Ud), (Wd, Ud.T), (Wd.double(), Ud), (Wd, Ud[:128, :128].contiguous())):
        assert w.shape == Wd.shape
        with pytest.raises(ValueError):
            spqr_quantize(w, u, cfg, thr)
    assert torch.equal(Wd.cpu(), torch.from_numpy(Wp.copy()))


# ---- F ------------------------------------------------------------------------------------------------------------------------------

_model = {}


def model_factor(R, K):
    """(Wp, U, U on the host) of one width, kept while consecutive cases use it (K = 4096 twice)"""
    if (R, K) not in _model:
        _model.clear()
        W, H = C.model_inputs(R, K, K + R, 'cuda')
        _, Wp, U = factor_on_gpu(W, H, True, 16)
        _model[(R, K)] = (Wp, U, U.cpu().numpy())
    return _model[(R, K)]


@pytest.mark.parametrize('R,K,g', C.MODEL)
def test_model_widths_sampled_rows_bit_exact(R, K, g):
    """The error feedback through 32 (K = 4096), 112 (K = 14336) and 12.5 (K = 1600) blocks with detection on: the kernel on
    all rows, the oracle on the first 16, the last 16 and 16 random rows (rows are independent given U and the threshold)."""
    Wp, U, Uh = model_factor(R, K)
    thr = C.MODEL_REL * (Wp.var(dim=0) / torch.diagonal(U).square()).mean().item()          # spqr.py:205-206
    rows = C.sample_rows(R, 16, K)
    ref = S.weight_transform(Wp[torch.from_numpy(rows).cuda()].cpu().numpy(), Uh, 4, g, thr, False)
    assert C.mask_share_ok(ref['mask']), int(ref['mask'].sum())
    got = run_loop(Wp, U, g, thr)
    assert_same(got, ref, rows=rows, what=f'{R}x{K} g{g}')
    assert np.isfinite(got['tmp']).all() and np.isfinite(got['losses']).all()
    if (R, K, g) == C.MODEL[-1]:
        _model.clear()


# ---- G ------------------------------------------------------------------------------------------------------------------------------

def test_quantize_stacked_three_layers_on_one_factor():
    """q / k / v (576, 192, 192 rows of bf16) at K = 576 with actorder and 5 dead input channels: each layer of the stack equals
    the layer run alone; the permutation, the dead columns, the un-permutation, the per-layer threshold and the loss are what
    spqr_factor + spqr_quantize by hand give; the loop on the product's factor is bit-exact against the oracle; the factor is
    within the project's bound (test_chol_inv_upper_vs_fp64) of an fp64 restatement of spqr_factor's recipe."""
    from conftest import report
    from llmc_amd.compression.quantization.spqr import SpqrConfig, quantize_stacked, spqr_factor, spqr_quantize
    K, rows_of = C.STACK_K, C.STACK_ROWS
    W, H, dead = C.dead_inputs(sum(rows_of), K, C.STACK_DEAD)
    Hd = torch.from_numpy(H).cuda()
    bounds = np.concatenate([[0], np.cumsum(rows_of)])
    ws = [torch.from_numpy(W[a:b]).to(torch.bfloat16).cuda() for a, b in zip(bounds[:-1], bounds[1:])]
    cfg = SpqrConfig(bit=4, group_size=16, actorder=True, percdamp=1.0, relative_threshold=C.STACK_REL)
    # H is handed over as a copy each time: hessian_prep sets the dead diagonal of its argument to 1, like the reference does
    res = quantize_stacked(ws, Hd.clone(), cfg)
    assert len(res) == 3 and all(int(r.info.item()) == 0 for r in res)
    for w, r in zip(ws, res):
        alone = quantize_stacked([w], Hd.clone(), cfg)[0]
        assert torch.equal(alone.perm, r.perm) and alone.threshold == r.threshold
        for k in ('weight', 'mask', 'scales', 'zeros'):
            assert torch.equal(getattr(alone, k), getattr(r, k)), k

    perm, Wp, U, info = spqr_factor(Hd.clone(), torch.cat(ws, 0), cfg)
    assert torch.equal(perm, res[0].perm)
    ph = perm.cpu().numpy()
    dp = np.diag(H)[ph]
    assert (np.diff(dp) <= 0).all() and sorted(ph[-C.STACK_DEAD:]) == sorted(dead) and (dp[:-C.STACK_DEAD] > 0).all()
    assert not Wp[:, -C.STACK_DEAD:].any() and Wp[:, :-C.STACK_DEAD].abs().sum(0).min() > 0
    np.testing.assert_array_equal(Wp.cpu().numpy(), torch.cat(ws, 0).float().cpu().numpy()[:, ph] * (dp != 0))
    invperm = torch.argsort(perm)
    Uh = U.cpu().numpy()
    for (a, b), r in zip(zip(bounds[:-1], bounds[1:]), res):
        Wl = Wp[a:b].contiguous()
        tmp, losses, mask, s, z = spqr_quantize(Wl.clone(), U, cfg, r.threshold)
        assert torch.equal(r.weight, tmp[:, invperm]) and torch.equal(r.mask, mask[:, invperm].bool())
        assert torch.equal(r.scales, s) and torch.equal(r.zeros, z) and torch.equal(r.loss, losses.sum())
        ref = S.weight_transform(Wl.cpu().numpy(), Uh, 4, 16, r.threshold, False)
        assert C.mask_share_ok(ref['mask'])
        assert_same(dict(tmp=tmp.cpu().numpy(), losses=losses.cpu().numpy(), mask=mask.cpu().numpy(), scales=s.cpu().numpy(),
                         zeros=z.cpu().numpy()), ref, what=f'layer rows {a}:{b}')
        t_ref = S.outlier_threshold(Wl.cpu().numpy(), Uh, C.STACK_REL)
        assert abs(r.threshold - t_ref) <= 1e-5 * t_ref, (r.threshold, t_ref)

    # the factor: permute, damp by percdamp * mean|diag| with the dead zeros in the mean, THEN dead diagonal := 1 (fp64)
    Hp = torch.from_numpy(H.astype(np.float64)[ph][:, ph])
    dg = torch.diagonal(Hp)
    dead_p = dg == 0
    dg += cfg.percdamp * dg.abs().mean()
    dg[dead_p] = 1.0
    Uref = torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(Hp)), upper=True).numpy()
    _, U32, p32 = S.process_hessian_and_weights(W, H, True, 1.0)          # the numpy fp32 route, for the error scale
    np.testing.assert_array_equal(np.diag(H)[p32], dp)                    # the same order but for ties among the dead
    e_ref = np.abs(U32 - Uref).max() / np.abs(Uref).max()
    e_ours = np.abs(Uh - Uref).max() / np.abs(Uref).max()
    report('spqr_stacked_factor_vs_fp64', e_ours=e_ours, e_ref=e_ref)
    assert np.array_equal(Uh, np.triu(Uh)) and e_ours <= max(4 * e_ref, 1e-5), (e_ours, e_ref)
