"""llmc_sparsegpt_prune (llmc_amd/csrc/sparsegpt_loop.hip) where tests/test_sparsegpt_gpu.py does not reach: the two-digit
select's edges (one first-digit bin, a threshold of +0, the last rank, subnormal and +inf scores), a single ragged block and
row counts around the 16-row workgroup and the 4-row wave, tall panels (k_sg_hist's capped grid, a trailing update of 4 columns
under 20000 rows), model widths (K = 4096, 11008) on a factor from chol_inv_upper, a NaN lower triangle under U, and calls of
different shape and mode back to back on the one cached workspace, also in turn with magnitude_prune, whose select is the same
code (csrc/radix_select.h). The inputs are tests/sparsegpt_cases.py's, whose
conditions tests/test_sparsegpt_cases.py proves on the CPU. Every comparison with tests/sparsegpt_oracle.py is bit for bit:
test_sparsegpt_gpu.py's assert_same on Wout, losses and the running W as uint32 views and on the mask as uint8."""
import numpy as np
import pytest
import torch

import sparsegpt_cases as C
import sparsegpt_oracle as O
from test_sparsegpt_gpu import assert_same, run_kernel

pytestmark = pytest.mark.gpu

_ref = {}


def oracle(key, W, U, mode):
    """the oracle's result, computed once per case and left unchanged"""
    if key not in _ref:
        _ref[key] = O.prune(W, U, **C.mode_kw(mode))
    return _ref[key]


def check(key, W, U, mode, U_device=None):
    """kernel == oracle on Wout, losses, mask and the running W. The kernel gets copies (the builders' arrays are read-only);
    U_device: what the device gets for U where that is not the oracle's."""
    want = oracle(key, W, U, mode)
    got = run_kernel(W.copy(), np.array(U if U_device is None else U_device), **C.mode_kw(mode))
    assert_same(got, want, key)
    return got, want


@pytest.mark.parametrize('name,mode', C.SELECT)
def test_select_edges_bit_exact(name, mode):
    """one_bin: k_sg_hist fills one bin and k_sg_hist_low ranks the whole panel. zero_floor: bin 0 and key 0, `s <= +0` prunes
    the zeros of either sign and nothing else. subnormal: the scores, the threshold and the losses are subnormal (the division
    and the key must keep them). overflow: keys of +inf in bin 0x7f80, kept at 0.5 and the threshold itself at 0.985.
    rank_last: rank numel - 1, the last bin the scan can stop in."""
    W, U = C.select_case(name)
    got, want = check((name, mode), W, U, mode)
    assert not any(np.isnan(got[k]).any() for k in ('Wout', 'losses', 'W'))


@pytest.mark.parametrize('R,K,mode', C.RAGGED)
def test_one_ragged_block_and_rows_around_the_workgroup_bit_exact(R, K, mode):
    """K < 128: a first block with count in {4, 20, 100, 124} (the guarded U tile load, d = 1 on the padding, a first stripe of
    fewer than 16 steps, no trailing update); K = 136 / 144 / 260: a last block of one group; R = 1, 3, 4, 5, 15, 16, 31, 33."""
    W, U = C.general(R, K)
    check(('ragged', R, K, mode), W, U, mode)


@pytest.mark.parametrize('mode', C.BIG_MODES)
@pytest.mark.parametrize('R,K', C.TALL)
def test_tall_panels_bit_exact(R, K, mode):
    """thousands of workgroups of the block kernel, one histogram from as many workgroups of k_sg_hist as its cap allows, and
    (K = 132) a trailing update of 4 columns under 20000 rows"""
    from conftest import report
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    report('sparsegpt_tall_panel', R=R, K=K, cus=cus, hist_grid_capped=bool(R * 128 > cus * 8192))
    W, U = C.general(R, K)
    check(('tall', R, K, mode), W, U, mode)


@pytest.fixture(scope='module')
def wide_factor():
    """U = chol_inv_upper(real_hessian(K)) on the device and its copy on the host (the oracle gets the same bits), made once per
    K and dropped when the next K comes"""
    from llmc_amd.compression.quantization import gptq_ops
    held = {}

    def get(K):
        if K not in held:
            held.clear()
            Ud = gptq_ops.chol_inv_upper(C.real_hessian(K, K).cuda().contiguous())
            held[K] = (Ud, Ud.cpu().numpy())
        return held[K]

    yield get
    held.clear()


@pytest.mark.parametrize('mode', C.BIG_MODES)
@pytest.mark.parametrize('R,K', C.WIDE)
def test_model_widths_on_a_real_factor_bit_exact(wide_factor, R, K, mode):
    """32 and 86 blocks: the row stride, the Hinv + i1 K + i2 offsets and the trailing update's N = K - i2 at K = 4096 and
    11008, on a factor whose diagonal decays"""
    Ud, Uh = wide_factor(K)
    d = np.diagonal(Uh)
    assert np.array_equal(Uh, np.triu(Uh)) and np.isfinite(Uh).all() and (d > 0).all() and d.max() > 2 * d.min()
    W = C.weights(R, K)
    want = oracle(('wide', R, K, mode), W, Uh, mode)
    Wg = torch.from_numpy(W).cuda()
    from llmc_amd.compression.sparsification import sparse_ops
    out, losses, mask = sparse_ops.sparsegpt_prune(Wg, Ud, want_losses=True, want_mask=True, **C.mode_kw(mode))
    got = dict(Wout=out.cpu().numpy(), losses=losses.cpu().numpy(), mask=mask.cpu().numpy(), W=Wg.cpu().numpy())
    assert_same(got, want, (R, K, mode))
    assert 0 < got['mask'].mean() < 1 and np.isfinite(got['Wout']).all() and np.isfinite(got['W']).all()


@pytest.mark.parametrize('mode', C.BIG_MODES)
@pytest.mark.parametrize('R,K', C.LOWER)
def test_the_lower_triangle_of_the_factor_is_never_used(R, K, mode):
    """the device's U holds NaN everywhere below the diagonal (a view of a workspace may hold anything there); the block
    kernel's float4 loads straddle the diagonal and the trailing GEMM reads Hinv[i1:i2, i2:]. The oracle gets the clean U."""
    W, U = C.general(R, K)
    got, want = check(('lower', R, K, mode), W, U, mode, U_device=C.nan_below(U))
    assert not any(np.isnan(got[k]).any() for k in ('Wout', 'losses', 'W'))


def test_calls_of_other_shapes_and_modes_on_the_one_workspace():
    """(300, 1024) at 0.5, (17, 256) at 0.9, (40, 320) at 4:8, zero_floor at 0.5 (which leaves the select's state at bin 0 and
    key 0), then the first again: a scan clears the histogram it read and a call zeroes the select's words at its start, so
    no call sees what another left behind"""
    got = []
    for name, R, K, mode in C.SEQUENCE:
        W, U = C.build(name, R, K)
        got.append(check(('sequence', name, R, K, mode), W, U, mode)[0])
    assert_same(got[-1], got[0], 'the first call again')


def test_magnitude_and_sparsegpt_calls_interleaved_on_the_shared_select():
    """csrc/radix_select.h serves both with two clearing conventions: magnitude_prune zeroes its workspace at the start of a call
    and leaves the histograms filled, sparsegpt_prune zeroes the select's words once and every scan clears what it read. What the
    two share is code, not memory (magnitude_prune gets a fresh workspace per call, sparsegpt_prune its cached one behind Err):
    this checks each convention on the one scan, not a histogram leaking from one call into another. In turn on one device: magnitude fp32 (64, 256) (both digits), sparsegpt 0.5 at (40, 260) (one full and one ragged block), magnitude
    bf16 (384, 256) (finished after the first digit), then the second and the first again. Every result bit for bit the oracle's
    (sparse_oracle.magnitude_prune at kth = numel / 2, sparsegpt_oracle.prune); a repeated call equals its first occurrence."""
    import sparse_oracle as SO
    from llmc_amd.compression.sparsification import sparse_ops
    g = torch.Generator().manual_seed(64 + 256)
    mag_w = {}
    for dt, (R, K) in ((torch.float32, (64, 256)), (torch.bfloat16, (384, 256))):
        w = (torch.randn(R, K, generator=g) * 0.05).to(dt)
        w[0, :7], w[1, :7] = 0.0, -0.0
        mag_w[dt] = (w, R * K // 2, SO.magnitude_prune(w, R * K // 2))

    def magnitude(dt):
        w, kth, (want, want_thresh, want_mask) = mag_w[dt]
        view = w.cuda()
        thresh, mask = sparse_ops.magnitude_prune(view, kth, want_mask=True)
        got = (SO.bits(view.cpu()), SO.bits(thresh.reshape(1).cpu()), mask.cpu())
        assert torch.equal(got[0], SO.bits(want)) and torch.equal(got[1], SO.bits(want_thresh.reshape(1))), dt
        assert torch.equal(got[2], want_mask), dt
        return got

    def sparsegpt():
        W, U = C.general(40, 260)
        return check(('interleaved', 40, 260), W, U, 's0.5')[0]

    m1, s1, _, s2, m2 = magnitude(torch.float32), sparsegpt(), magnitude(torch.bfloat16), sparsegpt(), magnitude(torch.float32)
    assert_same(s2, s1, 'sparsegpt again')
    assert all(torch.equal(a, b) for a, b in zip(m2, m1)), 'magnitude fp32 again'
