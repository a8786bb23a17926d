"""csrc/linear_eval.hip (k_linear_eval behind llmc_linear_eval, k_linear_eval4 behind llmc_linear_eval_kt) against an fp64 reference,
bit for bit, on inputs whose arithmetic is exact: X in {-1, 0, 1}, W in {-c, 0, c}, small odd integer biases. Every product and
every partial sum is a small integer, so every fp32 sum is exact in any order (k-slices included) and the only rounding left is the
single one to the model dtype, which the reference performs too. A wrong index, mask, staging address or a race between an epilogue and
the next tile's prologue shows as a bit difference; nothing here is compared with a tolerance. Each case asks the route hook
(llmc_test_linear_route, tests/linear_routes.py) which kernel, round count, k-slices, store form and STAGE_Y the call takes, and
asserts that it is the path the case is there for. Preconditions (magnitudes, exact tile sums) are asserted on the reference."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from linear_routes import (EINVAL, ENOTSUP, KTILED, ROW_MAJOR, STORE_BLOCKED, STORE_ROWS, STORE_SCALAR, STORE_SPLITK, route, route_of_loss,
                           route_of_out)
from llmc_amd import _ffi
from llmc_amd.compression.quantization import awq_ops

pytestmark = pytest.mark.gpu
TD = {'f16': torch.float16, 'bf16': torch.bfloat16}
DTS = ['bf16', 'f16']
EXACT = {'bf16': 256, 'f16': 2048}      # every integer up to here is a value of the dtype (8 / 11 significant bits)
POISON = 0x7FC1                         # a NaN in both dtypes


@functools.lru_cache(maxsize=None)
def case(N, K, R, pinv, c=1):
    """Operands, bias, Y0 offsets and the product as fp64 tensors on the device. W is non-zero with probability 1 / pinv; the pattern
    does not depend on c. The fp64 product of integers is exact, whatever the order torch sums in."""
    gen = torch.Generator().manual_seed(1000003 * N + 1009 * K + R)
    x = torch.randint(-1, 2, (N, K), generator=gen)
    w = c * (torch.randint(0, 2, (R, K), generator=gen) * 2 - 1) * (torch.randint(0, pinv, (R, K), generator=gen) == 0)
    b = torch.randint(-4, 4, (R,), generator=gen) * 2 + 1              # odd, -7 .. 7
    e = torch.randint(-2, 3, (N, R), generator=gen)
    x, w, b, e = (t.double().cuda() for t in (x, w, b, e))
    return SimpleNamespace(N=N, K=K, R=R, x=x, w=w, b=b, e=e, ref=x @ w.T)


def narrow(cs, R):
    """The same product with the first R rows of W only."""
    return SimpleNamespace(N=cs.N, K=cs.K, R=R, x=cs.x, w=cs.w[:R].contiguous(), b=cs.b[:R].contiguous(), e=cs.e[:, :R].contiguous(),
                           ref=cs.ref[:, :R].contiguous())


def bits(t):
    return t.contiguous().view(torch.int16)


def operands(cs, dt, tiled):
    x, w = cs.x.to(TD[dt]), cs.w.to(TD[dt])
    assert torch.equal(x.double(), cs.x) and torch.equal(w.double(), cs.w)
    return (awq_ops.ktile_pack(x), awq_ops.ktile_pack(w)) if tiled else (x, w)


def y_ref(cs, dt, bias=False, limit=None):
    """The reference output: the fp64 product (+ bias) rounded to the model dtype. limit: the precondition on its magnitude; by
    default every value is an integer the dtype holds, so the rounding changes nothing."""
    ref = cs.ref + cs.b if bias else cs.ref
    assert float(ref.abs().max()) <= (EXACT[dt] if limit is None else limit)
    assert cs.K * float(cs.w.abs().max()) < 2 ** 24          # every fp32 partial sum is an exact integer
    return ref.to(TD[dt])


def differences(got, want):
    bad = (bits(got) != bits(want)).nonzero()
    return f'{bad.shape[0]} of {want.numel()} elements differ, first at {bad[0].tolist()}: {got[tuple(bad[0])].item()} != {want[tuple(bad[0])].item()}'


def check_out(cs, dt, tiled, bias=False, blocked=False, limit=None):
    """linear_out against the reference; returns the route the call took and the output's bits."""
    x, w = operands(cs, dt, tiled)
    b = cs.b.to(TD[dt]) if bias else None
    want = y_ref(cs, dt, bias, limit)
    r = route_of_out(x, w, dt, b, tiled, blocked)
    assert r.status == 0 and r.kernel == (KTILED if tiled else ROW_MAJOR)
    y = awq_ops.linear_out(x, w, b, tiled=tiled, blocked=blocked)
    got = awq_ops.unblock_y(y, cs.N, cs.R) if blocked else y.clone()
    # the allocator hands this block to the next output of the same size: an element a later call leaves out is no stale right answer
    y.view(torch.int16).fill_(POISON)
    assert torch.equal(bits(got), bits(want)), differences(got, want)
    return r, bits(got)


def block_y(y, fill=64.0):
    """Row-major [N, R] -> the tile-blocked image (the inverse of awq_ops.unblock_y, which the blocked-output cases check against the
    kernel's own stores). The padding of edge tiles holds `fill`: the kernel must mask it."""
    N, R = y.shape
    n = ((N + 255) // 256) * ((R + 255) // 256) * 65536
    idx = awq_ops.unblock_y(torch.arange(n, device=y.device), N, R)
    yb = torch.full((n,), fill, dtype=y.dtype, device=y.device)
    yb[idx.reshape(-1)] = y.reshape(-1)
    return yb


def shifted(y):
    """The same matrix at an address that is 2 bytes past a 16-byte boundary."""
    buf = torch.empty(y.numel() + 8, dtype=y.dtype, device=y.device)
    v = buf[1:1 + y.numel()].view(y.shape)
    v.copy_(y)
    assert v.data_ptr() % 16 == 2 and v.is_contiguous()
    return v


def y0_of(cs, dt):
    """Y0 = reference output + e, e an integer in -2 .. 2: representable, so d = Y0 - Y is e exactly."""
    y0 = (cs.ref + cs.e).to(TD[dt])
    assert torch.equal(y0.double(), cs.ref + cs.e)
    return y0


def expected_loss(cs, dt, y0, acc0=0.0, times=1):
    """loss_acc after `times` calls: d formed and rounded in the model dtype, its squares summed exactly, added to the accumulator
    in float32 as k_loss_reduce does. Precondition: every 256 x 256 tile's sum is an integer below 2^24, so the kernel's fp32
    partials (lane, wave, tile) are exact in any order."""
    want = y_ref(cs, dt)
    d = (y0.double() - want.double()).to(TD[dt]).double()
    sq = d * d
    ntm, ntn = (cs.N + 255) // 256, (cs.R + 255) // 256
    pad = torch.zeros(ntm * 256, ntn * 256, dtype=torch.float64, device=sq.device)
    pad[:cs.N, :cs.R] = sq
    tiles = pad.reshape(ntm, 256, ntn, 256).sum((1, 3))
    assert torch.equal(tiles, tiles.round()) and float(tiles.max()) < 2 ** 24 and float(tiles.min()) > 0
    total = float(sq.sum())
    assert total < 2 ** 53
    acc = np.float32(acc0)
    for _ in range(times):
        acc = np.float32(acc + np.float32(total))
    return acc


def check_loss(cs, dt, tiled, form='rows', y0=None, acc0=0.0, times=1):
    """linear_loss_sum against the reference. form: 'rows' row-major Y0 as allocated, 'shifted' the same at a misaligned address,
    'blocked' the tile-blocked image. Returns the route."""
    x, w = operands(cs, dt, tiled)
    y0 = y0_of(cs, dt) if y0 is None else y0
    want = expected_loss(cs, dt, y0, acc0, times)
    arg = block_y(y0) if form == 'blocked' else shifted(y0) if form == 'shifted' else y0
    r = route_of_loss(x, w, dt, arg, tiled, form == 'blocked')
    assert r.status == 0 and r.kernel == (KTILED if tiled else ROW_MAJOR)
    acc = torch.full((1,), acc0, dtype=torch.float32, device='cuda')
    for _ in range(times):
        awq_ops.linear_loss_sum(x, w, arg, acc, tiled=tiled, y0_blocked=form == 'blocked')
    got = acc.cpu().numpy()[0]
    assert got == want, (float(got), float(want))
    return r


# ---- a. the second round: a workgroup refills its LDS ring behind every kind of epilogue -----------------------------------------------

def second_round_dims():
    G = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count & ~7
    T = math.isqrt(G) + 1                     # the smallest T with T * T > G
    assert T * T > G >= (T - 1) * (T - 1)
    return G, T, 256 * T - 37, 256 * T - 56, 256 * T - 61


def second_round_case(K, odd):
    G, T, N, R, R_odd = second_round_dims()
    assert R % 8 == 0 and R_odd % 2 == 1
    cs = case(N, K, R, 2)
    return G, T, narrow(cs, R_odd) if odd else cs


def in_second_round(r, G, T, tiled):
    assert r.grid == (G if tiled else 256) and r.tiles == T * T > r.grid and r.nrounds >= 2 and r.ksplit == 1
    assert r.sbm * r.sbn * 8 == r.grid


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('odd', [False, True])
@pytest.mark.parametrize('bias', [False, True])
def test_second_round_ktiled_store(dt, odd, bias):
    """K = 256: two ring turns per tile. R % 8 == 0: rows staged through the idle ring; odd R: two-byte stores."""
    G, T, cs = second_round_case(256, odd)
    r, _ = check_out(cs, dt, True, bias)
    in_second_round(r, G, T, True)
    assert r.store == (STORE_SCALAR if odd else STORE_ROWS)


@pytest.mark.parametrize('dt', DTS)
def test_second_round_ktiled_blocked_store(dt):
    G, T, cs = second_round_case(256, False)
    r, _ = check_out(cs, dt, True, True, blocked=True)
    in_second_round(r, G, T, True)
    assert r.store == STORE_BLOCKED


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('form,odd,stage', [('rows', False, 1), ('rows', True, 0), ('shifted', False, 0), ('blocked', False, 2)])
def test_second_round_ktiled_loss(dt, form, odd, stage):
    """STAGE_Y 1 (Y0 rows through LDS), 0 by an odd R, 0 by a misaligned Y0, 2 (tile-blocked Y0)."""
    G, T, cs = second_round_case(256, odd)
    r = check_loss(cs, dt, True, form)
    in_second_round(r, G, T, True)
    assert r.stage_y == stage


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('what', ['plain', 'bias', 'loss'])
def test_second_round_row_major(dt, what):
    """K = 192: three k-steps, an odd count for the double buffer, so a tile ends on the stage the next one starts with."""
    G, T, cs = second_round_case(192, False)
    r = check_loss(cs, dt, False) if what == 'loss' else check_out(cs, dt, False, what == 'bias')[0]
    in_second_round(r, G, T, False)
    assert (r.store, r.stage_y) == ((-1, 0) if what == 'loss' else (STORE_SCALAR, -1))


# ---- b. k-slices with a remainder ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('shape,pinv,sk', [((300, 1152, 200), 4, 2), ((300, 1664, 200), 8, 3), ((300, 4224, 200), 16, 8),
                                           ((700, 1152, 520), 4, 2)])
def test_split_k_with_a_remainder_slice(dt, bias, shape, pinv, sk):
    """The slices are whole ring turns of 4 stages of 32 k; K / 32 is no multiple of 4 * ksplit here, so the last slice is longer
    than the others. The sliced and the single-pass form both give the reference's bits."""
    N, K, R = shape
    assert (K // 32) % (4 * sk) != 0 and K % 128 == 0
    cs = case(N, K, R, pinv)
    r, sliced = check_out(cs, dt, True, bias)
    assert (r.ksplit, r.store, r.tiles) == (sk, STORE_SPLITK, sk * -(-N // 256) * -(-R // 256))
    with _ffi.option(linear_nosplit=1):
        r, single = check_out(cs, dt, True, bias)
    assert (r.ksplit, r.store) == (1, STORE_ROWS)
    assert torch.equal(sliced, single)
    assert _ffi.get_option('linear_nosplit') == 0


# ---- c. tile edges and tiny shapes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('shape,store,stage', [((255, 128, 257), STORE_SCALAR, 0), ((256, 128, 256), STORE_ROWS, 1),
                                               ((257, 384, 255), STORE_SCALAR, 0)])
def test_ktiled_tile_edges(dt, shape, store, stage):
    cs = case(*shape, 2)
    for bias in (False, True):
        r, _ = check_out(cs, dt, True, bias)
        assert (r.store, r.ksplit, r.nrounds) == (store, 1, 1)
    assert check_out(cs, dt, True, True, blocked=True)[0].store == STORE_BLOCKED
    assert check_loss(cs, dt, True).stage_y == stage
    assert check_loss(cs, dt, True, 'shifted').stage_y == 0
    assert check_loss(cs, dt, True, 'blocked').stage_y == 2


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('shape', [(1, 64, 8), (7, 64, 13), (257, 192, 255)])
def test_row_major_tile_edges(dt, shape):
    """K = 64 is a single k-step (nothing is ever staged ahead), K = 192 an odd count."""
    cs = case(*shape, 2)
    for bias in (False, True):
        r, _ = check_out(cs, dt, False, bias)
        assert (r.store, r.nrounds) == (STORE_SCALAR, 1)
    assert check_loss(cs, dt, False).stage_y == 0
    assert check_loss(cs, dt, False, 'shifted').stage_y == 0


# ---- d. the single rounding, on ties --------------------------------------------------------------------------------------------------------

def rounding_case(dt):
    """An odd c that puts max |ref| into the binade above the exact integers (spacing 2): every odd sum is a tie."""
    N, K, R, pinv = 300, 1152, 200, 4
    lo = EXACT[dt]
    m1 = float(case(N, K, R, pinv).ref.abs().max())
    c = int((2 * lo - 8) // m1)
    c -= 1 - c % 2
    cs = case(N, K, R, pinv, c)
    for ref in (cs.ref, cs.ref + cs.b):
        assert lo < float(ref.abs().max()) < 2 * lo
    return cs, 2 * lo


@pytest.mark.parametrize('dt', DTS)
def test_rounding_happens_once_and_to_nearest_even(dt):
    cs, limit = rounding_case(dt)
    t = TD[dt]
    refb = cs.ref + cs.b
    ties = (cs.ref.to(t).double() != cs.ref) & (cs.ref.abs() % 2 == 1)
    assert int(ties.sum()) >= 16                                            # sums the dtype does not hold: halfway between two values
    twice = cs.ref.to(t) + cs.b.to(t)                                       # rounded before the bias is added, and again after
    assert int((bits(twice) != bits(refb.to(t))).sum()) >= 16
    for tiled in (False, True):
        for bias in (False, True):
            r, y = check_out(cs, dt, tiled, bias, limit=limit)
            if tiled:
                assert (r.ksplit, r.store) == (2, STORE_SPLITK)
                with _ffi.option(linear_nosplit=1):
                    r, y1 = check_out(cs, dt, True, bias, limit=limit)
                assert (r.ksplit, r.store) == (1, STORE_ROWS) and torch.equal(y, y1)


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('tiled,form', [(False, 'rows'), (True, 'rows'), (True, 'shifted'), (True, 'blocked')])
def test_loss_difference_is_rounded_to_the_model_dtype(dt, tiled, form):
    """One tile; three planted Y0 values make d = Y0 - Y = 2^p + 1 or 2^p + 3, which the dtype does not hold (bf16: 257 -> 256,
    259 -> 260; f16: 2049 -> 2048, 2051 -> 2052); d = 0 elsewhere. The loss is that of the rounded d."""
    cs = case(256, 128, 256, 2)
    want = y_ref(cs, dt)
    big = float(EXACT[dt])
    y0 = want.clone()
    planted = []
    for v, take in ((-1.0, (0, -1)), (-3.0, (0,))):
        at = (want == v).nonzero()
        assert at.shape[0] >= 2
        planted += [tuple(at[i].tolist()) for i in take]
    for i, j in planted:
        y0[i, j] = big
    exact = y0.double() - want.double()
    rounded = exact.to(TD[dt]).double()
    assert sorted(exact[i, j].item() for i, j in planted) == [big + 1, big + 1, big + 3]
    assert sorted(rounded[i, j].item() for i, j in planted) == [big, big, big + 4]
    assert int((exact != 0).sum()) == 3 and float((rounded * rounded).sum()) != float((exact * exact).sum())
    r = check_loss(cs, dt, tiled, form, y0=y0)
    assert r.stage_y == ({'rows': 1, 'shifted': 0, 'blocked': 2}[form] if tiled else 0)
    assert expected_loss(cs, dt, y0) == np.float32(2 * big * big + (big + 4) ** 2)


# ---- e. accumulation into a loss that is not zero -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('tiled,form', [(False, 'rows'), (True, 'rows'), (True, 'blocked')])
def test_loss_accumulates_into_a_nonzero_sum(dt, tiled, form):
    cs = case(257, 384, 255, 2)
    check_loss(cs, dt, tiled, form, acc0=12345.0, times=2)


# ---- f. the k-tiled layout ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('rows', [1, 63, 65, 300])
@pytest.mark.parametrize('K', [32, 96, 160])
def test_ktile_pack_layout(dt, rows, K):
    """T[K / 32][rows][32]; rows that do not fill a 64-row block, and an odd number of 32-k slices (a block packs two)."""
    gen = torch.Generator().manual_seed(rows * 1000 + K)
    x = torch.randint(-32768, 32768, (rows, K), generator=gen).to(torch.int16).cuda().view(TD[dt])      # any bit pattern
    xt = awq_ops.ktile_pack(x)
    assert xt.shape == x.shape and xt.dtype == x.dtype
    assert torch.equal(bits(xt).reshape(K // 32, rows, 32), bits(x).reshape(rows, K // 32, 32).transpose(0, 1))


# ---- g. refusals, and linear_auto's routes --------------------------------------------------------------------------------------------------

def raw_call(tiled, x, w, N, K, R, flags, y=None, y0=None, loss=None, ws=None, x_off=0):
    L = _ffi.lib()
    fn = L.llmc_linear_eval_kt if tiled else L.llmc_linear_eval
    rc = fn(_ffi.ptr(x) + x_off, _ffi.ptr(w), _ffi.dt(x), N, K, R, flags, _ffi.ptr(y), _ffi.ptr(y0), _ffi.ptr(loss), _ffi.ptr(ws),
            _ffi.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('dt', DTS)
def test_refused_calls_write_nothing(dt):
    t = TD[dt]
    N, R = 300, 200

    def buffers(K):
        x = torch.ones(N * K + 8, dtype=t, device='cuda')
        w = torch.ones(R, K, dtype=t, device='cuda')
        return x, w, torch.full((N, R), 3.0, dtype=t, device='cuda'), torch.full((1,), 7.0, dtype=torch.float32, device='cuda'), \
            torch.full((64,), 5.0, dtype=torch.float32, device='cuda')

    def untouched(y, loss, ws):
        return bool((y == 3.0).all()) and loss.item() == 7.0 and bool((ws == 5.0).all())

    cases = [(False, 100, 0, 0, ENOTSUP), (True, 100, 0, 0, ENOTSUP), (True, 192, 0, 0, ENOTSUP),       # K % 64, K % 128
             (False, 128, 0, 2, EINVAL), (True, 128, 0, 2, EINVAL),                                        # X two bytes off
             (False, 128, 2, 0, EINVAL), (True, 128, 2, 0, EINVAL), (True, 128, 8, 0, EINVAL),             # no such mode
             (False, 128, _ffi.LINEAR_YBLOCKED, 0, EINVAL)]                                                # blocked: k-tiled only
    for tiled, K, flags, x_off, status in cases:
        x, w, y, loss, ws = buffers(K)
        for mode in (0, 1):
            if mode == 0:
                rc = raw_call(tiled, x, w, N, K, R, flags, y=y, ws=ws, x_off=x_off)
            else:
                rc = raw_call(tiled, x, w, N, K, R, flags | 1, y0=y, loss=loss, ws=ws, x_off=x_off)
            assert rc == status, (tiled, K, flags, x_off, mode, rc, _ffi.last_error())
            assert untouched(y, loss, ws), (tiled, K, flags, x_off, mode)
            hook = route(tiled, dt, N, K, R, mode=mode, flags=flags | mode, y=mode == 0, ws=True, mis=(x_off, 0, 0, 0, 0))
            assert hook.status == status
    # the same buffers are accepted once the argument is in order (the refusals above are about the argument, not the buffers)
    x, w, y, loss, ws = buffers(128)
    assert raw_call(True, x, w, N, 128, R, 0, y=y) == 0 and bool((y == 128.0).all())


@pytest.mark.parametrize('dt', DTS)
def test_linear_auto_gives_the_reference_bits_on_every_route(dt, monkeypatch, capfd):
    seen = []
    real_out, real_torch = awq_ops.linear_out, torch.nn.functional.linear

    def spy_out(x, wq, bias=None, tiled=False, blocked=False):
        seen.append('ktiled' if tiled else 'row-major')
        return real_out(x, wq, bias, tiled=tiled, blocked=blocked)

    def spy_torch(*a, **k):
        seen.append('torch')
        return real_torch(*a, **k)

    monkeypatch.setattr(awq_ops, 'linear_out', spy_out)
    monkeypatch.setattr(torch.nn.functional, 'linear', spy_torch)
    for shape, via in [((200, 128, 72), 'row-major'),        # fewer tokens than a tile: packing costs more than it saves
                       ((300, 128, 200), 'ktiled'),           # K % 128 == 0
                       ((300, 192, 200), 'row-major'),        # K % 64 == 0 only
                       ((300, 100, 200), 'torch')]:           # K % 64 != 0
        cs = case(*shape, 2)
        x, w, b = cs.x.to(TD[dt]), cs.w.to(TD[dt]), cs.b.to(TD[dt])
        for bias in (False, True):
            del seen[:]
            y = awq_ops.linear_auto(x, w, b if bias else None)
            assert seen == [via], (shape, seen)
            want = y_ref(cs, dt, bias)
            assert torch.equal(bits(y), bits(want)), (shape, bias, differences(y, want))
    assert 'outside the HIP GEMM' in capfd.readouterr().err
