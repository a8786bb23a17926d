"""The helper-stream schedule of the column loop (llmc_test_gptq_pipe_plan, a pure host call) replayed as a happens-before check:
two in-order lanes, events between them. Every pair of launches on different lanes that touch the same memory, one of them
writing, is ordered by the events; the exit join puts the caller's stream behind both lanes; and without lanes and events the
plan is the one-stream k4_split_far plan row for row. GPU bit-compares of the two schedules cannot see a race that happens not to
fire; this can. No GPU needed."""
import numpy as np
import pytest

from llmc_amd import _ffi
from test_chain_riders_plan import BLOCK, NEAR, NEAR_FAR, FAR, FLUSH, GROUP, SHAPES, check, plan

RECORD, WAIT = 5, 6
CHAIN, BULK = 0, 1

# (256, 2048, None): four groups, so group 3 rewrites err buffer 0, which group 0's bulk pieces read. (256, 2048, 1002): OWQ, the
# last group's per-block updates reach [1002, 2048), which group 0's bulk pieces also write.
PIPE_SHAPES = SHAPES + [(256, 2048, None), (256, 2048, 1002)]


def pipe_plan(R, K, n_quant=None, group_size=128, static_groups=0):
    cap = 64 + 24 * (K // 128 + 1)
    out = np.zeros((cap, 13), np.int32)
    n = _ffi.lib().llmc_test_gptq_pipe_plan(R, K, n_quant or K, group_size, static_groups, out.ctypes.data, cap)
    assert 0 <= n <= cap, (n, _ffi.last_error())
    return out[:n]


def footprint(row):
    """(columns of W read and written, err buffer, err k range or None for all of it, writes the err buffer)."""
    kind, g, w0, w1, err_rd, err_wr = row[:6]
    if kind == BLOCK:
        assert row[6] == -1, 'riders in the helper-stream schedule'
        k0 = w0 - g * GROUP
        return (w0, w1), err_wr, (k0, k0 + (w1 - w0)), True
    assert kind in (NEAR, NEAR_FAR, FAR)
    # a near product reads its block's slice only; taken as the whole buffer here (more conflicts to order, never fewer)
    return (w0, w1), err_rd, None, False


def conflict(a, b):
    """What two launches must not do at the same time: 'W', 'err' or None."""
    (a0, a1), ae, ak, aw = a
    (b0, b1), be, bk, bw = b
    if a0 < b1 and b0 < a1:
        return 'W'          # every launch writes its columns of W
    if ae == be and (aw or bw) and (ak is None or bk is None or (ak[0] < bk[1] and bk[0] < ak[1])):
        return 'err'
    return None


def replay(recs, footprint=footprint, lane_col=12):
    """Vector clocks: clock[l][m] = how many of lane m's launches are ordered before the next launch of lane l. (The footprint
    function and the lane's column are parameters for tests/test_chol_plan.py, which replays K3's plans the same way.)"""
    issued = [0, 0]
    clock = [[0, 0], [0, 0]]
    events = {}
    launches = []            # (lane, index on its lane, clock at issue, footprint)
    for row in recs.tolist():
        kind, lane = row[0], row[lane_col]
        assert lane in (CHAIN, BULK)
        if kind == RECORD:
            assert row[1] not in events and row[1] > 0, 'an event id recorded twice'
            snap = list(clock[lane])
            snap[lane] = issued[lane]
            events[row[1]] = snap
        elif kind == WAIT:
            assert row[1] in events, 'wait for an event that was not recorded before'
            clock[lane] = [max(x, y) for x, y in zip(clock[lane], events[row[1]])]
        else:
            launches.append((lane, issued[lane], list(clock[lane]), footprint(row)))
            issued[lane] += 1
    return launches, issued, clock


def unordered_conflicts(launches, conflict=conflict):
    bad = []
    for j, (lj, _, cj, fj) in enumerate(launches):
        for i in range(j):
            li, ni, _, fi = launches[i]
            # issued earlier on the other lane: ordered only if the later launch's lane has waited past it
            if li != lj and cj[li] <= ni and conflict(fi, fj):
                bad.append((i, j, conflict(fi, fj)))
    return bad


@pytest.mark.parametrize('R,K,n_quant', PIPE_SHAPES)
def test_conflicting_launches_on_different_lanes_are_ordered(R, K, n_quant):
    recs = pipe_plan(R, K, n_quant)
    launches, issued, clock = replay(recs)
    assert unordered_conflicts(launches) == []
    # entry: the bulk lane starts behind the caller's stream; exit: the caller's stream (the chain) is behind all of the bulk lane
    assert recs[0, 0] == RECORD and recs[0, 12] == CHAIN and recs[1, 0] == WAIT and recs[1, 12] == BULK and recs[1, 1] == recs[0, 1]
    assert recs[-2, 0] == RECORD and recs[-2, 12] == BULK and recs[-1, 0] == WAIT and recs[-1, 12] == CHAIN and recs[-1, 1] == recs[-2, 1]
    assert clock[CHAIN][BULK] == issued[BULK]
    # the bulk lane carries far pieces beyond the next group only, and only where there are such columns
    bulk = recs[(recs[:, 12] == BULK) & (recs[:, 0] < RECORD)]
    assert (bulk[:, 0] == FAR).all() and (bulk[:, 2] >= GROUP * (bulk[:, 1] + 2)).all()
    assert (len(bulk) > 0) == (min(n_quant or K, K - 1) > GROUP and K > 2 * GROUP)


@pytest.mark.parametrize('R,K,n_quant', PIPE_SHAPES)
def test_without_lanes_it_is_the_one_stream_split_plan(R, K, n_quant):
    recs = pipe_plan(R, K, n_quant)
    with _ffi.option(k4_split_far=1):
        one = plan(R, K, n_quant)
    assert np.array_equal(recs[recs[:, 0] < RECORD][:, :12], one)
    check(R, K, n_quant, one)
    assert not np.isin(one[:, 0], (FLUSH,)).any() and (one[:, 6] == -1).all()


def test_the_two_dependencies_the_small_shapes_are_there_for():
    """The replay sees them. With the chain lane's waits taken out of the plan, (256, 2048): group 3's in-block launches rewrite err
    buffer 0 unordered against group 0's pieces on the bulk lane, which read it; (256, 2048, n_quant 1002): the last group's near
    products write [1002, 2048) unordered against group 0's bulk pieces, which write [1024, 2048)."""
    for shape, cause, late_kind, late_group in (((256, 2048, None), 'err', BLOCK, 3), ((256, 2048, 1002), 'W', NEAR, 1)):
        recs = pipe_plan(*shape)
        keep = ~((recs[:, 0] == WAIT) & (recs[:, 12] == CHAIN))
        keep[-1] = True                # the exit join stays
        rows = recs[keep]
        launch_rows = rows[rows[:, 0] < RECORD]
        found = False
        for i, j, why in unordered_conflicts(replay(rows)[0]):
            a, b = launch_rows[i], launch_rows[j]
            found |= (why == cause and a[0] == FAR and a[1] == 0 and a[12] == BULK and b[0] == late_kind and b[1] == late_group)
        assert found, shape
