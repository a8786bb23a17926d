"""The launch plan of the one-stream column loop with rider tiles (llmc_test_gptq_rider_plan, a pure host call): every tile of
every group's far update is issued exactly once, in the reference's order (block 0, 1, 2, ... per element), before the first
later launch that touches its columns or rewrites its err buffer. No GPU needed."""
import numpy as np
import pytest

from llmc_amd import _ffi

BLOCK, NEAR, NEAR_FAR, FAR, FLUSH = range(5)
GROUP = 512


def cu_count():
    """What the library sizes the rider quota with: the current device's CU count, 256 (MI355X) where there is no device."""
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count if torch.cuda.is_available() else 256

# (R, K, n_quant): the shapes tests/test_chain_riders_gpu.py runs
SHAPES = [(4096, 14336, None), (6144, 4096, None), (4096, 4096, None), (28672, 4096, None), (8192, 28672, None),
          (4096, 1024, None), (4096, 4096 + 128, None), (4096, 4096, 3002), (4096, 14336, 9001), (1024, 2304, None),
          (384, 1536, None), (4096, 4100, None)]


def plan(R, K, n_quant=None, group_size=128, static_groups=0):
    L = _ffi.lib()
    cap = 64 + 16 * (K // 128 + 1)
    out = np.zeros((cap, 12), np.int32)
    with _ffi.helper_streams(False):
        n = L.llmc_test_gptq_rider_plan(R, K, n_quant or K, group_size, static_groups, out.ctypes.data, cap)
    assert 0 <= n <= cap, (n, _ffi.last_error())
    return out[:n]


def check(R, K, n_quant, recs):
    """Replays the plan on a per-column count of far updates received."""
    NQ = n_quant or K
    starts = list(range(0, NQ, GROUP))
    gend = [min(g0 + GROUP, NQ) for g0 in starts]
    near_end = [K if e == NQ else e for e in gend]
    nblocks = [-(-(e - g0) // 128) for g0, e in zip(starts, gend)]
    has_far = [ne < K for ne in near_end]
    applied = np.zeros(K, np.int64)           # far updates (one per earlier group) a column has received
    blocks_done = [0] * len(starts)
    far_left = [K - e if f else 0 for e, f in zip(gend, has_far)]      # columns of the group's far update not yet issued
    err_owner = {}

    kdone = np.zeros(K, np.int64)             # how many of the current far update's 512 err columns a column has received

    def far(g, c0, c1, err, k0=0, k1=0):
        k0, k1 = (0, 512) if k1 == 0 else (k0, k1)
        assert has_far[g] and gend[g] <= c0 < c1 <= K and 0 <= k0 < k1 <= 512 and k0 % 128 == 0 and k1 % 128 == 0
        assert blocks_done[g] == nblocks[g], 'far update before the group\'s err columns are complete'
        assert err_owner.get(err) == g, 'err buffer rewritten before the far update read it'
        assert (applied[c0:c1] == g).all(), 'far updates out of order (or issued twice)'
        assert (kdone[c0:c1] == k0).all(), 'a tile\'s k ranges out of order (or issued twice)'
        kdone[c0:c1] = k1
        if k1 == 512:
            kdone[c0:c1] = 0
            applied[c0:c1] += 1
            far_left[g] -= c1 - c0

    for kind, g, w0, w1, err_rd, err_wr, rg, r0, r1, rerr, k0, k1 in recs.tolist():
        if kind == BLOCK:
            assert (applied[w0:w1] == g).all() and (kdone[w0:w1] == 0).all(), 'in-block kernel before every earlier group\'s update of its columns'
            assert starts[g] + 128 * blocks_done[g] == w0
            if blocks_done[g] == 0 and err_wr in err_owner:
                assert far_left[err_owner[err_wr]] == 0, 'err buffer rewritten while far tiles that read it are pending'
            err_owner[err_wr] = g
            blocks_done[g] += 1
            if rg >= 0:
                # the two roles of one launch share nothing: riders beyond everything this group's launches write, other err buffer
                assert rg == g - 1 and r0 >= near_end[g] and rerr != err_wr
                assert (r0 - gend[rg]) % 128 == 0 and (r1 - r0) % 128 == 0
                ntiles = (r1 - r0) // 128 * (R // 128)
                assert 0 < ntiles <= cu_count() - -(-R // 32), 'more rider tiles than CUs the chain leaves free'
                far(rg, r0, r1, rerr, k0, k1)
        elif kind == NEAR:
            assert err_rd == g % 3 and w1 == near_end[g]
            lo = max(w0, gend[g])
            assert (applied[lo:w1] == g).all() and (kdone[lo:w1] == 0).all(), 'last group\'s near update before earlier far updates landed'
        else:
            assert kind in (NEAR_FAR, FAR, FLUSH) and err_rd == g % 3
            far(g, w0, w1, err_rd, k0, k1)
    assert blocks_done == nblocks
    assert far_left == [0] * len(starts)
    expect = np.zeros(K, np.int64)
    for g, e in enumerate(gend):
        if has_far[g]:
            expect[e:] += 1
    assert (applied == expect).all(), 'a far tile was dropped or issued twice'


@pytest.mark.parametrize('R,K,n_quant', SHAPES)
def test_every_far_tile_once_and_in_order(R, K, n_quant):
    recs = plan(R, K, n_quant)
    check(R, K, n_quant, recs)
    with _ffi.option(no_riders=1):
        off = plan(R, K, n_quant)
    check(R, K, n_quant, off)
    # the switch restores the one-launch far update over [gend, K): no riders, no flush
    assert (off[:, 6] == -1).all() and not np.isin(off[:, 0], (NEAR_FAR, FLUSH)).any()
    far = off[off[:, 0] == FAR]
    assert (far[:, 3] == K).all()
    with _ffi.option(k4_split_far=1):
        check(R, K, n_quant, plan(R, K, n_quant))


@pytest.mark.parametrize('R,K', [(4096, 14336), (6144, 4096), (4096, 4096), (4096, 4096 + 128)])
def test_riders_are_planned_where_the_chain_leaves_cus_free(R, K):
    recs = plan(R, K)
    riders = recs[recs[:, 6] >= 0]
    assert len(riders) > 0
    per_launch = (cu_count() - R // 32) // (R // 128)          # whole tile columns, one tile per free CU, half its k per launch
    width = (riders[:, 8] - riders[:, 7]) // 128
    assert (width <= per_launch).all() and width.max() == per_launch
    # what rides is the tail of a group's far update, sized to the next group's four launches: nothing is ever left to flush
    assert not (recs[:, 0] == FLUSH).any()
    far = recs[recs[:, 0] == FAR]
    assert (far[:, 2] == 512 * (far[:, 1] + 1)).all()          # the launch behind a group starts at the next group's columns
    g0 = far[0]
    assert g0[3] == max(1024, K - 2 * per_launch * 128)
    assert set(map(tuple, riders[:, 10:12].tolist())) == {(0, 256), (256, 512)}


@pytest.mark.parametrize('R,K,n_quant', [(28672, 4096, None), (8192, 28672, None), (4096, 1024, None), (4096, 4100, None),
                                         (4000, 4096, None), (1024, 2304, None), (384, 1536, None)])
def test_no_riders_where_the_chain_fills_the_chip_or_the_shape_is_not_tiled(R, K, n_quant):
    """R >= 8192: the in-block kernel's workgroups cover the CUs; K <= 1024: no far-far columns; K % 128 != 0 or R % 128 != 0: the far
    update is not on whole 128 x 128 tiles; R <= 2048: the chain role takes less than half the CUs, a regime that was not measured.
    The plan is the one the switch gives."""
    recs = plan(R, K, n_quant)
    with _ffi.option(no_riders=1):
        off = plan(R, K, n_quant)
    assert np.array_equal(recs, off)
