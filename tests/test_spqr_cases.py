"""The inputs of tests/test_spqr_widths_gpu.py (tests/spqr_cases.py) reach what they are there for: shown here on the oracle
(oracle/spqr_ref.py, pinned to the reference by tests/test_oracle_golden.py) and on the arrays themselves, never on the kernel's
output, so that no GPU test passes because its input had nothing to find."""
import math

import numpy as np
import pytest

import spqr_cases as C
from oracle import spqr_ref as S

KEYS = ('mask', 'scales', 'zeros', 'tmp', 'losses')


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS)


@pytest.mark.parametrize('R,K,g,rel', C.RAGGED)
def test_ragged_cases_find_outliers_and_the_oracle_takes_the_shape(R, K, g, rel):
    """A: K % 128 != 0 and K % g == 0; both finite modes mask at least one entry and at most half; the detection changes some
    group's qparams (the two modes are not one test run twice); the inf mode masks nothing."""
    assert K % 128 != 0 and K % g == 0 and K % 4 == 0
    Wp, U = C.general(R, K)
    assert Wp.shape == (R, K) and np.array_equal(U, np.triu(U)) and np.count_nonzero(np.triu(U, 1)) > 0
    out = {}
    for mode in C.MODES:
        thr, simp = C.mode_args(mode, Wp, U, rel)
        out[mode] = o = S.weight_transform(Wp, U, 4, g, thr, simp)
        assert np.isfinite(o['tmp']).all() and np.isfinite(o['losses']).all()
        assert C.mask_share_ok(o['mask']) if mode != 'inf' else o['mask'].sum() == 0, (mode, int(o['mask'].sum()))
    assert (out['detect']['scales'] != out['simplified']['scales']).any()
    assert not same(out['detect'], out['inf'])


@pytest.mark.parametrize('R,K,g', C.GRID)
def test_grid_weights_hold_duplicated_extremes_at_detection_time(R, K, g):
    """B1: with the diagonal U every group is detected on exactly the values written, and at least 20 % of the groups hold
    their min in more than one column, likewise their max; the detection flags columns in some groups and changes qparams.
    With the general U only the first group of every row is still untouched, and some of those are tied."""
    Wp, U = C.grid(R, K, g, 'diag')
    assert np.count_nonzero(U - np.diag(np.diag(U))) == 0 and (np.diag(U) > 0).all()
    lo, hi = C.tie_share(Wp, g)
    assert lo >= 0.2 and hi >= 0.2, (lo, hi)
    for kind in C.GRID_U:
        Wp, U = C.grid(R, K, g, kind)
        thr = C.threshold(Wp, U, C.GRID_THR)
        o = S.weight_transform(Wp, U, 4, g, thr, False)
        assert C.mask_share_ok(o['mask']), (kind, int(o['mask'].sum()))
        assert (o['scales'] != S.weight_transform(Wp, U, 4, g, thr, True)['scales']).any(), kind
    lo, hi = C.tie_share(Wp[:, :g], g)                # general U: the untouched first groups, R of them, a few of them tied
    assert lo * R >= 3 and hi * R >= 3, (lo, hi)
    # the ties decide something: a detection that takes every holder of an extreme for its only holder flags other columns in
    # several groups (at a relative threshold of 0.1 it would flag the same ones in all 960 groups of g = 16: a tied column has
    # no error of its own, and the wrong leave-one-out grid only moves its Loo by the rounding errors of the others)
    Wp, U = C.grid(R, K, g, 'diag')
    G, d = Wp.reshape(-1, g), np.tile(np.diag(U).reshape(-1, g), (R, 1))
    thr = C.threshold(Wp, U, C.GRID_THR)
    fl = C.detection_flags(G, d, 4, thr)
    assert fl.any(1).sum() >= 10 and (fl != C.detection_flags(G, d, 4, thr, assume_unique=True)).any(1).sum() >= 5


@pytest.mark.parametrize('g', [16, 32])
def test_planted_groups_are_what_their_names_say(g):
    """B2: on the diagonal U the planted groups are what the detection sees. The unique extremes are flagged by the numpy
    restatement of the detection, the doubled ones are not (leaving one copy out leaves the grid alone); in the *_far plants a
    detection with a wrong count of copies would flag both copies and so change the group's stored scale."""
    Wp, U, where = C.planted(g)
    thr = C.threshold(Wp, U, C.PLANT_THR)
    assert C.mask_share_ok(S.weight_transform(Wp, U, 4, g, thr, False)['mask'])
    assert np.count_nonzero(U - np.diag(np.diag(U))) == 0
    d = np.diag(U)
    for r, groups in where.items():
        name = C.PLANTS[r % len(C.PLANTS)]
        for q in groups:
            v = Wp[r, q * g:(q + 1) * g]
            n_lo, n_hi = int((v == v.min()).sum()), int((v == v.max()).sum())
            fl = C.detection_flags(v[None], d[None, q * g:(q + 1) * g], 4, thr)[0]
            if name == 'constant':
                assert n_lo == n_hi == g and not fl.any()
            elif name == 'two_values':
                assert len(np.unique(v)) == 2 and n_lo > 1 and n_hi > 1
            elif name in ('min_col0', 'min_col15', 'min_reg1'):
                at = {'min_col0': 0, 'min_col15': 15, 'min_reg1': 21 % g}[name]
                assert n_lo == 1 and v.argmin() == at and fl[at]
            elif name in ('max_col0', 'max_col15', 'max_reg1'):
                at = {'max_col0': 0, 'max_col15': 15, 'max_reg1': 21 % g}[name]
                assert n_hi == 1 and v.argmax() == at and fl[at]
            elif name in ('min_twice', 'min_twice_far'):
                assert n_lo == 2 and v[3] == v.min() and not fl[v == v.min()].any()
            elif name in ('max_twice', 'max_twice_far'):
                assert n_hi == 2 and v[3] == v.max() and not fl[v == v.max()].any()
            elif name == 'signed_zeros':
                assert (v == 0).all() and 0 < np.signbit(v).sum() < g
            elif name == 'zeros_and_values':
                z = v == 0
                assert v.min() == 0 and np.signbit(v[z]).any() and not np.signbit(v[z]).all() and (v > 0).any()
            if name.endswith('_far'):          # only the count of copies keeps the two unflagged (and the group's range wide)
                assert d[q * g + 3] == d[(q + 1) * g - 2] == C.FAR_D
                assert C.detection_flags(v[None], d[None, q * g:(q + 1) * g], 4, thr, assume_unique=True)[0, [3, g - 2]].all()
    assert g == 16 or 21 % g >= 16                       # the second register of a lane


@pytest.mark.parametrize('actorder', [True, False])
def test_dead_channel_inputs_through_the_numpy_route(actorder):
    """B3 (the GPU test takes (Wp, U) from spqr_factor; the same H and W through the oracle's factor here): 40 exactly-zero
    Hessian diagonals, their weight columns zeroed, d = 1 there, outliers found."""
    R, K, g = C.DEAD_SHAPE
    W, H, dead = C.dead_inputs(R, K, C.DEAD_N)
    assert (np.diag(H)[dead] == 0).all() and (np.diag(H) == 0).sum() == C.DEAD_N and not H[dead].any()
    Wp, U, perm = S.process_hessian_and_weights(W, H, actorder, 1.0)
    at = np.flatnonzero((Wp == 0).all(0))
    assert len(at) == C.DEAD_N and np.allclose(np.diag(U)[at], 1.0, rtol=0, atol=1e-6)
    assert not actorder or np.array_equal(at, np.arange(K - C.DEAD_N, K))
    assert C.mask_share_ok(S.weight_transform(Wp, U, 4, g, C.threshold(Wp, U, C.DEAD_REL), False)['mask'])


def test_threshold_edges_and_the_group_with_every_column_flagged():
    """C: thr = 0 and the tiny threshold mask almost everything; the numpy restatement of the detection finds first groups
    (untouched by any feedback) with ALL columns flagged, the `n_keep < 1` branch; a huge finite threshold and both sides of
    the kernel's cut give the oracle's inf result."""
    R, K, g = C.EDGE_SHAPE
    Wp, U = C.general(R, K)
    d = np.tile(np.diag(U)[:g], (R, 1))
    tiny = C.threshold(Wp, U, C.TINY_REL)
    assert 0 < np.float32(tiny) < 1e-4
    for thr in (0.0, tiny):
        o = S.weight_transform(Wp, U, 4, g, thr, False)
        assert o['mask'].mean() > 0.9 and np.isfinite(o['tmp']).all()
        assert C.detection_flags(Wp[:, :g], d, 4, thr).all(1).sum() >= 5
    inf = S.weight_transform(Wp, U, 4, g, math.inf, False)
    for thr in (1e30, C.CUT_BELOW, C.CUT_ABOVE):
        assert np.isfinite(np.float32(thr)) and same(S.weight_transform(Wp, U, 4, g, thr, False), inf)
    assert np.float32(C.CUT_BELOW) <= np.float32(3.0e38) < np.float32(C.CUT_ABOVE)


def test_bit_width_cases_find_outliers():
    """D: every weight width with its scaled threshold, every second-level pair; the second-level widths change stored values."""
    R, K, g = C.EDGE_SHAPE
    Wp, U = C.general(R, K)
    for bit in C.BITS:
        assert C.mask_share_ok(S.weight_transform(Wp, U, bit, g, C.threshold(Wp, U, C.bit_rel(bit)), False)['mask']), bit
    thr = C.threshold(Wp, U, C.EDGE_REL)
    outs = [S.weight_transform(Wp, U, 4, g, thr, False, sb, zb) for sb, zb in C.SECOND_LEVEL_BITS]
    assert all(C.mask_share_ok(o['mask']) for o in outs)
    assert (outs[0]['zeros'] != outs[1]['zeros']).any() and (outs[1]['zeros'] != outs[2]['zeros']).any()


def test_row_cases_find_outliers_from_the_first_row_on():
    """E: one input, its first R rows per case: the oracle of R rows is the first R rows of the oracle of all (independence of
    rows, which the sampled-row checks at model widths rely on too), and row 0 alone already holds an outlier."""
    Wp, U, thr = C.rows_input()
    full = S.weight_transform(Wp, U, 4, 16, thr, False)
    for R in C.ROWS:
        assert C.mask_share_ok(full['mask'][:R]), R
    part = S.weight_transform(Wp[:17], U, 4, 16, thr, False)
    assert all(np.array_equal(part[k], full[k][:17]) for k in KEYS)


def test_stacked_inputs_through_the_numpy_route():
    """G (the GPU test re-asserts this on the product's own factor): every layer of the stack finds outliers at its threshold;
    the dead channels are exact zeros of diag(H)."""
    K = C.STACK_K
    W, H, dead = C.dead_inputs(sum(C.STACK_ROWS), K, C.STACK_DEAD)
    assert (np.diag(H) == 0).sum() == C.STACK_DEAD and K % 128 != 0
    Wp, U, perm = S.process_hessian_and_weights(W, H, True, 1.0)
    assert sorted(perm[-C.STACK_DEAD:]) == sorted(dead)
    r0 = 0
    for R in C.STACK_ROWS:
        Wl = Wp[r0:r0 + R]
        r0 += R
        assert C.mask_share_ok(S.weight_transform(Wl, U, 4, 16, C.threshold(Wl, U, C.STACK_REL), False)['mask']), R


def test_sample_rows_cover_both_ends():
    for R, K, g in C.MODEL:
        rows = C.sample_rows(R, 16, K)
        assert 48 <= len(rows) <= 64 and set(range(16)) <= set(rows) and set(range(R - 16, R)) <= set(rows)
        assert len(set(rows)) == len(rows) and rows.min() >= 0 and rows.max() < R
