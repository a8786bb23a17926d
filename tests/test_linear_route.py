"""What llmc_linear_eval / llmc_linear_eval_kt launch is data (lin_route through llmc_test_linear_route, a pure host call): kernel, grid,
tile order, k-slices, store form and STAGE_Y of the calls the product makes, and the refusals, checked without a device on a
256-CU grid. The expected numbers are worked out from the rules in csrc/linear_eval.hip's comments, not read back from it."""
import pytest

from linear_routes import (EINVAL, ENOTSUP, KTILED, ROW_MAJOR, STORE_BLOCKED, STORE_NONE, STORE_ROWS, STORE_SCALAR, STORE_SPLITK,
                           route)
from llmc_amd import _ffi

CU = 256


def test_row_major_entry_is_one_fixed_geometry():
    for dt in ('bf16', 'f16'):
        r = route(False, dt, 2048, 4096, 4096, cus=CU)
        assert (r.status, r.kernel, r.grid, r.threads, r.ksplit, r.store, r.stage_y) == (0, ROW_MAJOR, 256, 512, 1, STORE_SCALAR, -1)
        assert (r.ntm, r.ntn, r.nrounds) == (8, 16, 1)
        r = route(False, dt, 2048, 4096, 4096, mode=1, cus=CU)
        assert (r.status, r.kernel, r.store, r.stage_y) == (0, ROW_MAJOR, STORE_NONE, 0)
    assert route(False, 'bf16', 1, 64, 8, cus=CU).nrounds == 1
    # the grid does not follow the device: 256 workgroups whatever it has
    assert route(False, 'bf16', 2048, 4096, 4096, cus=64).grid == 256


def test_tile_order_of_a_ragged_17_x_17_product():
    """289 tiles on 256 workgroups: 32 tiles per XCD and round as 8 x 4 blocks (480 padded tiles, the fewest; 4 x 8 pads as many
    and comes later), 3 x 5 blocks over 8 XCDs = 2 rounds."""
    for tiled in (False, True):
        r = route(tiled, 'bf16', 256 * 17 - 37, 256 if tiled else 192, 256 * 17 - 56, cus=CU)
        assert (r.status, r.kernel, r.grid) == (0, int(tiled), 256)
        assert (r.ntm, r.ntn, r.sbm, r.sbn, r.nrounds) == (17, 17, 8, 4, 2)
    # 16 x 16 tiles fill the grid exactly: one round, no padding
    r = route(True, 'bf16', 4096, 256, 4096, cus=CU)
    assert (r.sbm * r.sbn, r.nrounds) == (32, 1)
    # a smaller device: 64 workgroups, 8 tiles per XCD and round
    r = route(True, 'bf16', 4096, 256, 4096, cus=70)
    assert (r.grid, r.sbm * r.sbn, r.nrounds) == (64, 8, 4)


@pytest.mark.parametrize('shape,sk', [((300, 1152, 200), 2), ((300, 1664, 200), 3), ((300, 4224, 200), 8), ((700, 1152, 520), 2),
                                      ((2048, 4096, 4096), 2), ((300, 512, 200), 1), ((4096, 4096, 12288), 1)])
def test_k_slices(shape, sk):
    """tiles * slices fills the grid, at least 512 k per slice, at most 8 slices, none once 3/4 of the CUs have a tile."""
    N, K, R = shape
    r = route(True, 'bf16', N, K, R, ws=True, cus=CU)
    tiles = -(-N // 256) * -(-R // 256)
    assert (r.status, r.ksplit, r.ntm * r.ntn) == (0, sk, tiles * sk)
    assert r.store == (STORE_SPLITK if sk > 1 else STORE_ROWS)
    # without a workspace, with a misaligned one or output, with the option, blocked or in loss mode: a single pass
    assert route(True, 'bf16', N, K, R, ws=False, cus=CU).ksplit == 1
    assert route(True, 'bf16', N, K, R, ws=True, mis=(0, 0, 0, 0, 4), cus=CU).ksplit == 1
    assert route(True, 'bf16', N, K, R, ws=True, mis=(0, 0, 2, 0, 0), cus=CU).ksplit == 1
    assert route(True, 'bf16', N, K, R, ws=True, blocked=True, cus=CU).ksplit == 1
    assert route(True, 'bf16', N, K, R, mode=1, cus=CU).ksplit == 1
    with _ffi.option(linear_nosplit=1):
        assert route(True, 'bf16', N, K, R, ws=True, cus=CU).ksplit == 1
    assert route(True, 'bf16', N, K, R - 3, ws=True, cus=CU).ksplit == 1       # R % 8 != 0: the reduction kernel stores 8 per thread


def test_store_forms_and_stage_y():
    k = dict(cus=CU)
    assert route(True, 'f16', 300, 128, 200, **k).store == STORE_ROWS
    assert route(True, 'f16', 300, 128, 201, **k).store == STORE_SCALAR                       # R % 8 != 0
    assert route(True, 'f16', 300, 128, 200, mis=(0, 0, 2, 0, 0), **k).store == STORE_SCALAR   # Y not 16-B aligned
    assert route(True, 'f16', 300, 128, 201, blocked=True, **k).store == STORE_BLOCKED
    for r in (route(True, 'f16', 300, 128, 200, y0=True, **k), route(True, 'f16', 300, 128, 200, **k)):
        assert r.stage_y == -1
    assert route(True, 'f16', 300, 128, 200, mode=1, **k).stage_y == 1
    assert route(True, 'f16', 300, 128, 201, mode=1, **k).stage_y == 0
    assert route(True, 'f16', 300, 128, 200, mode=1, mis=(0, 0, 0, 2, 0), **k).stage_y == 0
    assert route(True, 'f16', 300, 128, 201, mode=1, blocked=True, **k).stage_y == 2
    assert route(True, 'f16', 300, 128, 200, mode=1, **k).store == STORE_NONE
    assert route(True, 'f16', 65536, 128, 32768, mode=1, **k).stage_y == 0                    # Y0 of 4 GiB: not through a buffer descriptor


def test_refusals():
    k = dict(cus=CU)
    for tiled in (False, True):
        r = route(tiled, 'bf16', 300, 100, 200, **k)
        assert r.status == ENOTSUP and ('K % 128' if tiled else 'K % 64') in r.error
        assert route(tiled, 'bf16', 300, 128, 200, mis=(2, 0, 0, 0, 0), **k).status == EINVAL
        assert route(tiled, 'bf16', 300, 128, 200, mis=(0, 8, 0, 0, 0), **k).status == EINVAL
        assert route(tiled, 2, 300, 128, 200, **k).status == EINVAL                           # fp32
        assert route(tiled, 'bf16', 0, 128, 200, **k).status == EINVAL
        assert route(tiled, 'bf16', 300, 128, 200, y=False, **k).status == EINVAL
        assert route(tiled, 'bf16', 300, 128, 200, mode=1, ws=False, **k).status == EINVAL
        assert route(tiled, 'bf16', 300, 128, 200, mode=1, loss=False, **k).status == EINVAL
        assert route(tiled, 'bf16', 300, 128, 200, flags=2, y=True, **k).status == EINVAL
        assert route(tiled, 'bf16', 1 << 20, 2048, 256, **k).status == ENOTSUP                 # X of 4 GiB
    assert route(False, 'bf16', 300, 192, 200, **k).status == 0
    assert route(True, 'bf16', 300, 192, 200, **k).status == ENOTSUP
    r = route(True, 'bf16', 300, 128, 200, flags=8, y=True, **k)
    assert r.status == EINVAL and 'unknown mode bits' in r.error
    assert route(False, 'bf16', 300, 128, 200, flags=_ffi.LINEAR_YBLOCKED, y=True, **k).status == EINVAL     # no blocked form there
    assert route(True, 'bf16', 300, 128, 200, blocked=True, mis=(0, 0, 8, 0, 0), **k).status == EINVAL
    assert route(True, 'bf16', 300, 128, 200, mode=1, blocked=True, mis=(0, 0, 0, 8, 0), **k).status == EINVAL
    assert route(True, 'bf16', 65536, 128, 32768, blocked=True, **k).status == ENOTSUP         # blocked image of 4 GiB
    assert route(True, 'bf16', 300, 128, 200, cus=7).status == EINVAL
    L = _ffi.lib()
    assert L.llmc_test_linear_route(None, None) == EINVAL


def test_workspace_query_agrees_with_the_route():
    """llmc_linear_eval_ws_bytes covers the fp32 slices the route asks for (this process has no device: 256 CUs)."""
    L = _ffi.lib()
    for N, K, R in [(300, 1152, 200), (300, 4224, 200), (700, 1152, 520), (2048, 4096, 4096), (4096, 4096, 12288), (300, 192, 200)]:
        r = route(K % 128 == 0, 'bf16', N, K, R, ws=True)
        tiles = -(-N // 256) * -(-R // 256)
        assert L.llmc_linear_eval_ws_bytes(N, K, R) == max(4 * tiles, r.ksplit * N * R * 4 if r.ksplit > 1 else 0)
