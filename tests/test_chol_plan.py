"""K3's host schedule (llmc_test_chol_plan, a pure host call) checked without a device: the helper-stream plan replayed as a
happens-before check with the replay of test_gptq_pipe_plan.py (two in-order lanes, events between them), the pieces of every
factor step and far update compared with the one-stream plan's, and every plan of the option matrix checked for rectangles
inside their buffers. Every rectangle in a plan is read back from the arguments the launch would get. No GPU needed."""
import numpy as np
import pytest

from llmc_amd import _ffi
from test_gptq_pipe_plan import RECORD, WAIT, CHAIN, BULK, replay, unordered_conflicts

TRANSPOSE, POTRF, SOLVE, UPDATE, SPLIT, FAR, PLACE, ZERO, INV_X, INV_C = 0, 1, 2, 3, 4, 7, 8, 9, 10, 11
SGEMM, GEMM3, GEMM6 = 1, 2, 3
WORK, VBLK, XBUF, G6WS, OTHER = range(5)
W, RA, RB, W2, LANE = 2, 7, 12, 17, 22          # where a row's four rectangles (buffer, r0, r1, c0, c1) and its lane start
NB, NBO = 128, 512

# 640: one outer block and a ragged second one; the bulk lane carries the steps' far columns only, no far update. 1536: the
# smallest K with a far update on the bulk lane. 2176: 17 ragged blocks, a bulk update still in flight while the next block's steps
# fork. 5000: no multiple of 128.
SHAPES = [640, 1536, 2176, 5000, 14336, 28672]
PLANES = dict(gemm3s_min_tiles=1)               # the planes path at every size
OPTIONS = [{}, dict(k3_fp32=1), dict(k3_no_planes=1), dict(k3_split_far=1), dict(k3_no_gemm6=1), PLANES]


def chol_plan(K, lanes=1, rev=0, **options):
    cap = 64 + 16 * (K // NB + 1)
    out = np.zeros((cap, 22 + lanes), np.int32)
    with _ffi.option(**options):
        n = _ffi.lib().llmc_test_chol_plan(K, rev, lanes, out.ctypes.data, cap)
    assert 0 <= n <= cap, (n, _ffi.last_error())
    return out[:n]


def launches_of(recs):
    return recs[(recs[:, 0] != RECORD) & (recs[:, 0] != WAIT)]


def footprint(row):
    """[(buffer, r0, r1, c0, c1, written)] of a launch. k_potrf_inv also sets the failure flag, with atomics: no conflict."""
    return [tuple(row[o:o + 5]) + (o in (W, W2),) for o in (W, RA, RB, W2) if row[o] >= 0]


def conflict(a, b):
    """The buffers in which two launches must not run at the same time (empty: none)."""
    return tuple(sorted({x[0] for x in a for y in b
                         if x[0] == y[0] and (x[5] or y[5]) and x[1] < y[2] and y[1] < x[2] and x[3] < y[4] and y[3] < x[4]}))


@pytest.mark.parametrize('options', [PLANES, {}], ids=['planes', 'default'])
@pytest.mark.parametrize('K', SHAPES)
def test_conflicting_launches_on_different_lanes_are_ordered(K, options):
    recs = chol_plan(K, **options)
    launches, issued, clock = replay(recs, footprint, LANE)
    assert unordered_conflicts(launches, conflict) == []
    # entry: the bulk lane starts behind the caller's stream; exit: the caller's stream (the chain) is behind all of the bulk lane
    assert recs[0, 0] == RECORD and recs[0, LANE] == CHAIN and recs[1, 0] == WAIT and recs[1, LANE] == BULK and recs[1, 1] == recs[0, 1]
    assert recs[-2, 0] == RECORD and recs[-2, LANE] == BULK and recs[-1, 0] == WAIT and recs[-1, LANE] == CHAIN and recs[-1, 1] == recs[-2, 1]
    assert clock[CHAIN][BULK] == issued[BULK]
    # the bulk lane carries the far columns of factor steps and far updates beyond the next block, where there are such
    bulk = launches_of(recs)
    bulk = bulk[bulk[:, LANE] == BULK]
    assert np.isin(bulk[:, 0], (SOLVE, UPDATE, FAR)).all()
    assert (len(bulk) > 0) == (K > NBO) and (bulk[:, 0] == FAR).any() == (K > 2 * NBO)
    if options:
        assert (launches_of(recs)[:, 0] == SPLIT).sum() == (K - 1) // NBO, 'the planes path at every far update'


def test_the_three_dependencies_the_replay_is_there_for():
    """With the chain's waits taken out of the plan (the exit join stays) the replay reports: (a) the block's far update on the
    chain reads panel rows that a step's panel solve on the bulk lane writes; (b) a factor step on the chain touches rows that a
    previous block's far update on the bulk lane writes; (c) the plane split on the chain rewrites X while the previous block's far
    update on the bulk lane reads it. In the plan, (a) is the wait 'the block's far panels are complete' and (c) 'the planes the
    previous block's update reads are free'; (b) and today also (c) are implied by (a)'s wait, which is behind the previous
    block's update on the in-order bulk lane — (c)'s wait is stated all the same, it is the dependency."""
    recs = chol_plan(2176, **PLANES)
    for options, reader, want in ((PLANES, SPLIT, {'a', 'b', 'c'}), ({}, FAR, {'a', 'b'})):
        # (a): with planes the far update reads the panel through its plane split; without (this size, default options) itself
        rows = chol_plan(2176, **options)
        keep = ~((rows[:, 0] == WAIT) & (rows[:, LANE] == CHAIN))
        keep[-1] = True
        rows = rows[keep]
        lr = launches_of(rows)
        found = set()
        for i, j, bufs in unordered_conflicts(replay(rows, footprint, LANE)[0], conflict):
            a, b = lr[i], lr[j]
            if a[LANE] != BULK or b[LANE] != CHAIN:
                continue
            if a[0] == SOLVE and b[0] == reader and WORK in bufs:
                found.add('a')
            if a[0] == FAR and b[0] in (POTRF, SOLVE, UPDATE) and WORK in bufs:
                found.add('b')
            if a[0] == FAR and b[0] == SPLIT and XBUF in bufs:
                found.add('c')
        assert found == want, options
    # and each of the chain's waits that is not implied by another is needed: without the first 'far panels' wait alone, (a)
    first = np.nonzero((recs[:, 0] == WAIT) & (recs[:, LANE] == CHAIN))[0][0]
    assert unordered_conflicts(replay(np.delete(recs, first, 0), footprint, LANE)[0], conflict) != []


def pieces(recs):
    """{(factor step or outer block, kind): [written rectangle of every piece, in issue order]} of the factorisation."""
    out, c0 = {}, None
    for row in launches_of(recs).tolist():
        if row[0] == POTRF:
            c0 = row[W + 1]
        if row[0] in (SOLVE, UPDATE):
            out.setdefault((c0, row[0]), []).append(tuple(row[W + 1:W + 5]))
        if row[0] == FAR:
            out.setdefault((c0 // NBO * NBO, FAR), []).append(tuple(row[W + 1:W + 5]))
    return out


def check_update_order(K, recs):
    """Per element of the trailing matrix the updates arrive in step order: on the grid of 128-blocks, done[i, j] = the factor
    steps whose update block (i, j), j >= i, has received."""
    n = -(-K // NB)
    done = np.zeros((n, n), np.int64)
    upper = np.triu(np.ones((n, n), bool))

    def cells(rect):
        r0, r1, c0, c1 = rect
        assert r0 % NB == 0 and c0 % NB == 0 and (r1 % NB == 0 or r1 == K) and (c1 % NB == 0 or c1 == K)
        m = np.zeros((n, n), bool)
        m[r0 // NB:-(-r1 // NB), c0 // NB:-(-c1 // NB)] = True
        return m & upper

    for row in launches_of(recs).tolist():
        kind, rect = row[0], tuple(row[W + 1:W + 5])
        if kind in (POTRF, SOLVE):          # step s reads and rewrites row s, which has received every earlier step's update
            step = rect[0] // NB
            assert (done[cells(rect)] == rect[0] // NB).all(), row
        elif kind == UPDATE:                # of step s = the panel rows it reads
            s = row[RA + 1] // NB
            assert (done[cells(rect)] == s).all(), row
            done[cells(rect)] = s + 1
        elif kind == FAR:                   # all the steps of the outer block before its rows, at once
            k = step // 4 * 4
            assert (done[cells(rect)] == k).all() and step == k + 3, row
            done[cells(rect)] = k + 4
    want = np.minimum.outer(np.arange(n), np.arange(n))
    assert (done[upper] == want[upper]).all()


@pytest.mark.parametrize('K', SHAPES[:-1])
def test_pieces_cover_what_the_one_stream_plan_covers_in_step_order(K):
    laned = chol_plan(K, **PLANES)
    one = chol_plan(K, lanes=0, **PLANES)
    split = chol_plan(K, lanes=0, k3_split_far=1, **PLANES)
    assert np.array_equal(launches_of(laned)[:, :LANE][launches_of(laned)[:, 0] >= PLACE], one[one[:, 0] >= PLACE]), 'the inverse'
    pl, po, ps = pieces(laned), pieces(one), pieces(split)
    assert pl.keys() == po.keys() == ps.keys() and len(po) > 0
    for key, whole in po.items():
        assert len(whole) == 1
        r0, r1, c0, c1 = whole[0]
        for cut in (pl[key], ps[key]):
            if key[1] == FAR:       # rows [r0, K) of the upper triangle, each piece from its own diagonal to the last column
                assert (r0, c0, r1, c1) == (r0, r0, K, K)
                assert [p[0] for p in cut] == [p[2] for p in cut] and all(p[3] == K for p in cut)
                edges = [p[0] for p in cut] + [cut[-1][1]]
                assert edges[0] == r0 and edges[-1] == K and [p[1] for p in cut] == edges[1:], (key, cut)
                assert len(cut) == (2 if r0 + NBO < K else 1)
            else:                   # columns [c0, K) of the step's rows: the chain's piece first in the plan, the bulk piece right of it
                cut = sorted(cut, key=lambda p: p[2])
                assert all(p[:2] == (r0, r1) for p in cut)
                edges = [p[2] for p in cut] + [cut[-1][3]]
                assert edges[0] == c0 and edges[-1] == c1 and [p[3] for p in cut] == edges[1:], (key, cut)
    # one stream: a step is one piece, whatever k3_split_far says
    assert all(len(v) == 1 for k, v in ps.items() if k[1] != FAR)
    for recs in (laned, one, split):
        check_update_order(K, recs)


def buffer_sizes(K):
    """(rows, columns) of every buffer, from the workspace size alone for the last."""
    a256 = lambda x: (x + 255) // 256 * 256
    vrows = -(-K // NB) * NB
    xfloats = (K // 2 + NB) ** 2
    g6 = _ffi.lib().llmc_chol_inv_upper_ws_bytes(K) - a256(K * K * 4) - a256(vrows * NB * 4) - a256(xfloats * 4)
    assert g6 >= 0
    return {WORK: (K, K), VBLK: (vrows, NB), XBUF: (1, xfloats), G6WS: (1, g6 // 4), OTHER: (K, K)}


@pytest.mark.parametrize('options', OPTIONS, ids=lambda o: '-'.join(o) or 'default')
@pytest.mark.parametrize('K', SHAPES[:-1])
def test_option_matrix_rectangles_lie_inside_their_buffers(K, options):
    size = buffer_sizes(K)
    for rev in (0, 1):
        for lanes in (0, 1):
            recs = chol_plan(K, lanes, rev, **options)
            rows = launches_of(recs)
            assert len(rows) > 0 and np.isin(rows[:, 0], (TRANSPOSE, POTRF, SOLVE, UPDATE, SPLIT, FAR, PLACE, ZERO, INV_X, INV_C)).all()
            for o in (W, RA, RB, W2):
                buf, r0, r1, c0, c1 = (rows[:, o + i] for i in range(5))
                assert np.isin(buf, (-1, WORK, VBLK, XBUF, G6WS, OTHER)).all(), 'a leading dimension that is not its buffer\'s'
                for b, (nr, nc) in size.items():
                    m = buf == b
                    assert (0 <= r0[m]).all() and (r0[m] < r1[m]).all() and (r1[m] <= nr).all()
                    assert (0 <= c0[m]).all() and (c0[m] < c1[m]).all() and (c1[m] <= nc).all(), (b, o)
            assert (rows[:, W] >= 0).all()
            # the caller's other matrix: read by the transposing pass in front (not with rev), written by the one at the end
            t = rows[rows[:, 0] == TRANSPOSE]
            assert len(t) == 2 - rev and t[-1, W] == OTHER and (rows[rows[:, 0] != TRANSPOSE][:, [W, RA, RB, W2]] != OTHER).all()
            assert (rows[0, 0] == TRANSPOSE) == (not rev) and rows[-1, 0] == TRANSPOSE
            if lanes:
                ev = recs[(recs[:, 0] == RECORD) | (recs[:, 0] == WAIT)]
                assert (ev[:, [W, RA, RB, W2]] == -1).all() and (ev[:, 1] > 0).all()
            else:
                assert len(rows) == len(recs)
            forms = set(rows[:, 1].tolist())
            assert (GEMM3 in forms) == ('k3_fp32' not in options)
            assert (GEMM6 in forms) == (K > 8192 and not ({'k3_fp32', 'k3_no_gemm6'} & set(options)))
            assert (ZERO in rows[:, 0]) == (K > 4096 and not ({'k3_fp32', 'k3_no_gemm6'} & set(options)))
            if 'k3_no_planes' in options or 'k3_fp32' in options:
                assert SPLIT not in rows[:, 0]
