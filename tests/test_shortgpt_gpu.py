"""llmc_block_influence (csrc/block_influence.hip) on the GPU against tests/shortgpt_oracle.py, bit for bit in the per-token values
and in the fp64 total, against the composition from torch ops within the derived bound, on every layout, on the special values
and on the reference's goldens. Shapes: the smallest at which each path of the kernel can go wrong."""
import numpy as np
import pytest
import torch

import shortgpt_oracle as O

pytestmark = pytest.mark.gpu

TDT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}

# (N, d, dtype): one vector in one lane; a partial wave; 65 vectors, ragged over the lanes; fp32 with a partial unrolled round;
# rows that are not whole vectors (scalar loads, a partial last slot); many workgroups at a model width; long rows (eight
# unrolled rounds); more rows than the default grid covers in one sweep
SHAPES = [(1, 8, 'bf16'), (3, 64, 'f16'), (5, 520, 'bf16'), (7, 100, 'f32'), (4, 36, 'bf16'), (300, 4096, 'bf16'),
          (2, 16384, 'bf16'), (70000, 8, 'bf16')]


def make(N, d, dt, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * N + d)
    x = torch.randn(N, d, generator=g) * torch.exp(0.5 * torch.randn(d, generator=g))
    y = x + torch.logspace(-2, 0, N).reshape(N, 1) * torch.randn(N, d, generator=g)
    return x.to(TDT[dt]), y.to(TDT[dt])


def f32(t):
    return t.float().cpu().numpy()


def composed_bound(d, dt):
    """torch sums a row's d products in an order of its own, a chain of at most d roundings per product (L = d), and its
    division and square roots may be HIP's fast forms, up to 2.5 ulp each: 8 more roundings cover the three."""
    return O.bound(64 * (d + 8), dt)


_CASES = {}


def case(N, d, dt):
    """inputs, the oracle's bits and the truth of a shape, computed once"""
    key = (N, d, dt)
    if key not in _CASES:
        x, y = make(N, d, dt)
        bi = O.block_influence(f32(x), f32(y), dt)
        _CASES[key] = (x, y, bi, O.total(bi), O.truth(f32(x), f32(y)))
    return _CASES[key]


def run(x, y, **kw):
    from llmc_amd.compression.sparsification import sparse_ops
    bi, total = sparse_ops.block_influence(x, y, **kw)
    assert bi.dtype == torch.float32 and bi.is_cuda and total.dtype == torch.float64 and total.is_cuda
    return bi.cpu().numpy(), np.float64(total.item())


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize('N,d,dt', SHAPES)
def test_kernel_equals_the_oracle_bit_for_bit_and_the_composition_within_the_bound(N, d, dt):
    from llmc_amd.compression.sparsification import sparse_ops
    x, y, want, want_total, truth = case(N, d, dt)
    xg, yg = x.cuda(), y.cuda()
    bi, total = run(xg, yg)
    assert same_bits(bi, want), np.abs(bi - want).max()
    assert total == want_total, (total, want_total)
    err = np.abs(bi.astype(np.float64) - truth).max()
    comp = sparse_ops.block_influence_composed(xg, yg).cpu().numpy()
    diff = np.abs(bi.astype(np.float64) - comp).max()
    print(f'{N} x {d} {dt}: |kernel - truth| {err:.3e} (bound {O.bound(d, dt):.3e}), |kernel - composed| {diff:.3e}')
    assert err <= O.bound(d, dt)
    assert diff <= O.bound(d, dt) + composed_bound(d, dt)


def test_a_forced_small_grid_gives_the_same_bits():
    x, y, want, want_total, _ = case(70000, 8, 'bf16')
    xg, yg = x.cuda(), y.cuda()
    for max_grid in (1, 3):
        bi, total = run(xg, yg, max_grid=max_grid)
        assert same_bits(bi, want) and total == want_total
    x, y, want, want_total, _ = case(300, 4096, 'bf16')
    bi, total = run(x.cuda(), y.cuda(), max_grid=2)
    assert same_bits(bi, want) and total == want_total


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
def test_layouts_give_the_bits_of_a_contiguous_copy(dt):
    from llmc_amd.compression.sparsification import sparse_ops
    N, d = 6, 136
    g = torch.Generator().manual_seed(11)
    bx = torch.randn(N, 2 * d, generator=g).to(TDT[dt]).cuda()
    by = (bx.float() + 0.1 * torch.randn(N, 3 * d, generator=g)[:, :2 * d].cuda()).to(TDT[dt])
    by3 = torch.zeros(N, 3 * d, dtype=TDT[dt], device='cuda')
    by3[:, :2 * d] = by

    def check(xv, yv, copies):
        want, want_total = run(xv.contiguous(), yv.contiguous())
        assert same_bits(want, O.block_influence(f32(xv), f32(yv), dt))
        ptr = []
        orig = sparse_ops._ffi.ptr
        sparse_ops._ffi.ptr = lambda t: ptr.append(orig(t)) or ptr[-1]
        try:
            bi, total = run(xv, yv)
        finally:
            sparse_ops._ffi.ptr = orig
        assert same_bits(bi, want) and total == want_total
        assert (ptr[0] == xv.data_ptr(), ptr[1] == yv.data_ptr()) == (not copies, not copies)      # read in place, not copied

    check(bx[:, :d], by[:, :d], False)                    # row stride 2 d
    check(bx[:, 1:d + 1], by[:, 1:d + 1], False)          # misaligned rows: the scalar loads
    check(bx[:, :d], by3[:, :d], False)                   # X and Y with different strides
    check(bx[:, :d], by3[:, 1:d + 1], False)              # one operand misaligned sends both to the scalar loads
    check(bx[:, :2 * d:2], by[:, :2 * d:2], True)         # a non-unit last stride is copied
    x3 = bx.reshape(2, 3, 2 * d)
    bi, _ = run(x3[..., :d], x3[..., d:])                 # [..., d] operands are read as rows
    assert same_bits(bi, O.block_influence(f32(bx[:, :d]), f32(bx[:, d:]), dt))


def test_special_values():
    d = 64
    g = torch.Generator().manual_seed(5)
    x = torch.randn(9, d, generator=g).to(torch.bfloat16)
    y = (x.float() + 0.2 * torch.randn(9, d, generator=g)).to(torch.bfloat16)
    x[0] = 0                                               # a zero row in X only
    x[1] = 0
    y[1] = 0                                               # a zero row in both
    y[2] = x[2]                                            # Y == X
    y[3] = -x[3]                                           # Y == -X
    x[4, 7] = float('nan')
    y[5, 63] = float('inf')
    x[6, 0] = float('-inf')
    y[6] = x[6]                                            # inf / inf
    bi, total = run(x.cuda(), y.cuda())
    b = O.bound(d, 'bf16')
    assert bi[0] == 0.5 and bi[1] == 0.5 and bi[4] == 0.5 and bi[5] == 0.5 and bi[6] == 0.5
    assert abs(bi[2]) <= b and abs(bi[3] - 2.0) <= b       # a few ulps negative is possible, as in the reference
    assert 0 < bi[7] < 1 and 0 < bi[8] < 1
    want = O.block_influence(f32(x), f32(y), 'bf16')
    assert same_bits(bi, want) and total == O.total(want)
    # fp16 rows of magnitude 60000: every square is 3.6e9, beyond fp16, and the fp32 sums hold them
    xh = (torch.randn(3, 4096, generator=g).sign() * 60000).to(torch.float16)
    yh = xh.clone()
    yh[:, ::3] *= -1
    assert torch.isfinite(xh).all() and float(xh.abs().max()) == 60000.0
    bi, total = run(xh.cuda(), yh.cuda())
    want = O.block_influence(f32(xh), f32(yh), 'f16')
    assert np.isfinite(bi).all() and same_bits(bi, want) and total == O.total(want)
    assert np.abs(bi - O.truth(f32(xh), f32(yh))).max() <= O.bound(4096, 'f16')


def test_two_calls_fold_into_the_oracle_two_batch_total():
    from llmc_amd.compression.sparsification import sparse_ops
    xa, ya, bia, _, _ = case(5, 520, 'bf16')
    xb, yb, bib, _, _ = case(300, 4096, 'bf16')
    run_total = torch.full((3,), -1.0, dtype=torch.float64, device='cuda')
    _, t = sparse_ops.block_influence(xa.cuda(), ya.cuda(), run_total[1], init=True)
    assert t.data_ptr() == run_total[1].data_ptr()
    sparse_ops.block_influence(xb.cuda(), yb.cuda(), run_total[1], init=False)
    got = run_total.cpu().numpy()
    assert got[0] == -1.0 and got[2] == -1.0                                   # the element alone is written
    assert got[1] == O.total(bib, running=O.total(bia))


def test_bad_arguments_are_refused_before_a_launch():
    from llmc_amd import _ffi
    from llmc_amd.compression.sparsification import sparse_ops
    x = torch.zeros(4, 16, dtype=torch.bfloat16, device='cuda')
    with pytest.raises(ValueError):
        sparse_ops.block_influence(x, x[:, :8])
    with pytest.raises(ValueError):
        sparse_ops.block_influence(x, x.float())
    with pytest.raises(ValueError, match='fp64'):
        sparse_ops.block_influence(x, x, torch.zeros(1, device='cuda'))
    L = _ffi.lib()
    assert L.llmc_block_influence_ws_bytes(0) == 0 and L.llmc_block_influence_ws_bytes(4097) == 16
    assert L.llmc_block_influence_ws_bytes(1 << 31) == (1 << 19) * 8 and L.llmc_block_influence_ws_bytes((1 << 31) + 1) == 0
    bi, tot, ws = torch.zeros(4, device='cuda'), torch.zeros(1, dtype=torch.float64, device='cuda'), torch.zeros(8, device='cuda')
    args = lambda **k: [k.get('x', x.data_ptr()), x.data_ptr(), k.get('dt', 1), k.get('N', 4), k.get('d', 16), k.get('ldx', 16), 16,   # noqa: E731
                        1, bi.data_ptr(), tot.data_ptr(), ws.data_ptr(), _ffi.stream()]
    for bad in (dict(dt=7), dict(N=0), dict(N=(1 << 31) + 1), dict(d=0), dict(ldx=15), dict(x=None)):
        assert L.llmc_block_influence(*args(**bad)) == -22, bad
    assert L.llmc_block_influence(*args(d=1 << 31, ldx=1 << 31)) == -22      # ldy = 16 < d comes first
    a = args(d=1 << 31, ldx=1 << 31)
    a[6] = 1 << 31
    assert L.llmc_block_influence(*a) == -95 and '2^31' in _ffi.last_error()


def test_the_gpu_result_on_the_goldens_is_nearer_the_truth_than_the_reference(golden):
    g = golden('shortgpt')
    for name in (str(n) for n in g['names']):
        dt, x, y, ref_bi, ref_total, ref_dist = O.golden_case(g, name)
        xt, yt = (torch.from_numpy(a).to(TDT[dt]).reshape(2, 24, 96).cuda() for a in (x, y))
        bi, total = run(xt, yt)
        truth = O.truth(x, y)
        assert same_bits(bi, O.block_influence(x, y, dt))
        if dt == 'f32':
            assert (np.abs(bi.astype(np.float64) - ref_bi) <= O.bound(96, dt) + ref_dist).all()          # (c)
        else:
            assert abs(total - truth.sum()) <= abs(ref_total - truth.sum())                                # (b)
