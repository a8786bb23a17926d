"""K4's column loop with far-update tiles riding on the in-block launches (k_gptq_block_riders, the default one-stream schedule)
against the one-launch far update (option no_riders): compensated weights, quantized weights, losses, scales and zeros identical
to the last bit, on the shapes of the models the benchmark runs and on the ragged ones."""
import pytest
import torch

from llmc_amd import _ffi
from llmc_amd.compression.quantization import gptq_ops

pytestmark = pytest.mark.gpu


def _inputs(R, K, seed):
    """W and the upper factor U of a damped random Hessian's inverse, generated on the device (K = 28672 is 3.3 GB a matrix)."""
    gen = torch.Generator(device='cuda').manual_seed(seed)
    n = max(K // 4, 512)
    X = torch.randn(n, K, generator=gen, device='cuda')
    X[:, ::5] *= 4
    H = (X.T @ X) / n
    del X
    H.diagonal().add_(0.05 * float(H.diagonal().mean()))
    U = gptq_ops.chol_inv_upper(H)
    W = torch.randn(R, K, generator=gen, device='cuda') * 0.02
    return W, U


def _both(W, U, run):
    """run(W) with riders and without; W is the running weight matrix the call overwrites (OWQ reads its tail afterwards)."""
    out = {}
    for name, opts in (('riders', {}), ('one_launch', dict(no_riders=1))):
        with _ffi.option(**opts), _ffi.helper_streams(False):
            Wc = W.clone()
            res = run(Wc)
            torch.cuda.synchronize()
            out[name] = (Wc,) + tuple(res)
    for i, (a, b) in enumerate(zip(out['riders'], out['one_launch'])):
        assert (a is None and b is None) or torch.equal(a, b), ('W', 'tmp', 'losses', 'scales', 'zeros')[i]


def _plan_has_riders(R, K, n_quant=None):
    import numpy as np
    cap = 64 + 16 * (K // 128 + 1)
    out = np.zeros((cap, 12), np.int32)
    with _ffi.helper_streams(False):
        n = _ffi.lib().llmc_test_gptq_rider_plan(R, K, n_quant or K, 128, 0, out.ctypes.data, cap)
    assert 0 <= n <= cap
    return bool((out[:n, 6] >= 0).any())


# (4096, 14336) down_proj, (6144, 4096) q/k/v stacked, (4096, 4096) o_proj, (28672, 4096) gate/up stacked: the chain fills the chip,
# no riders; K = 1024: fewer than three groups; K = 4096 + 128: the far update ends on a 128-column group
@pytest.mark.parametrize('R,K,riders', [(4096, 14336, True), (6144, 4096, True), (4096, 4096, True), (28672, 4096, False),
                                        (4096, 1024, False), (4096, 4096 + 128, True)])
def test_dynamic_g128_same_bits_with_and_without_riders(R, K, riders):
    assert _plan_has_riders(R, K) == riders
    W, U = _inputs(R, K, R + K)
    _both(W, U, lambda w: gptq_ops.gptq_quantize(w, U, False, 0.0, 15.0, 128))


def test_70b_down_proj_shape_has_no_riders_and_the_same_bits():
    """(8192, 28672): 256 chain workgroups on 256 CUs — nothing rides, the schedule is the one-launch one."""
    R, K = 8192, 28672
    need = (3 * K * K + 8 * R * K) * 4
    if torch.cuda.mem_get_info()[0] < need + (8 << 30):
        pytest.skip('not enough device memory for K = 28672')
    assert not _plan_has_riders(R, K)
    W, U = _inputs(R, K, 70)
    _both(W, U, lambda w: gptq_ops.gptq_quantize(w, U, False, 0.0, 15.0, 128))


@pytest.mark.parametrize('K,n_quant', [(4096, 3002), (14336, 9001)])
def test_owq_ragged_n_quant_same_bits(K, n_quant):
    """llmc_gptq_quantize_cols with n_quant that is no multiple of 4: the last group's per-block updates reach [n_quant, K), the
    queued tiles of the group before are flushed first."""
    R = 4096
    assert _plan_has_riders(R, K, n_quant)
    W, U = _inputs(R, K, K + n_quant)
    s0 = torch.ones(R, K // 128, device='cuda')
    z0 = torch.zeros(R, K // 128, device='cuda')
    _both(W, U, lambda w: gptq_ops.gptq_quantize(w, U, False, 0.0, 15.0, 128, n_quant=n_quant, init_scales=s0, init_zeros=z0))


def test_static_groups_same_bits():
    """The vllm variant: qparams given per static group (k_gptq_block<1> in the chain role)."""
    R, K = 4096, 4096
    W, U = _inputs(R, K, 11)
    Wg = W.view(R, K // 128, 128)
    mn, mx = Wg.amin(-1).clamp(max=0), Wg.amax(-1).clamp(min=0)
    scales = ((mx - mn) / 15.0).clamp(min=1e-5)
    zeros = (-mn / scales).round().clamp(0, 15)
    cg = torch.arange(K, device='cuda', dtype=torch.int32) // 128
    _both(W, U, lambda w: gptq_ops.gptq_quantize(w, U, False, 0.0, 15.0, 128, static_groups=True, col_group=cg, scales=scales,
                                                 zeros=zeros))
    _both(W, U, lambda w: gptq_ops.gptq_quantize(w, U, True, -8.0, 7.0, 0, scales=scales[:, :1].clone(), zeros=None))     # per channel, sym


def test_dynamic_g64_generic_path_same_bits():
    """Group size 64: qparams change inside a block, the chain role runs the generic path (k_gptq_block<0>)."""
    R, K = 4096, 4096
    W, U = _inputs(R, K, 64)
    _both(W, U, lambda w: gptq_ops.gptq_quantize(w, U, False, 0.0, 15.0, 64))


@pytest.mark.parametrize('R,K,n_quant', [(4096, 4096, None), (6144, 4096, 3002)])
def test_calib_algo_mse_same_bits(R, K, n_quant):
    """llmc_gptq_quantize_mse: the searched qparams of a block's groups are found right before its in-block launch, on the running
    panel — which the riders of the same launch never touch."""
    W, U = _inputs(R, K, R + 3)
    s0 = torch.ones(R, K // 128, device='cuda')
    z0 = torch.zeros(R, K // 128, device='cuda')
    _both(W, U, lambda w: gptq_ops.gptq_quantize(w, U, False, 0.0, 15.0, 128, n_quant=n_quant, init_scales=s0, init_zeros=z0,
                                                 mse=(1, 80, 100, 2.4)))


def test_riders_agree_with_the_helper_stream_schedule():
    """Three schedules, one result: riders (one stream), one launch per group (one stream), the helper-stream schedule."""
    R, K = 4096, 6144
    W, U = _inputs(R, K, 5)
    with _ffi.helper_streams(False):
        a = gptq_ops.gptq_quantize(W.clone(), U, False, 0.0, 15.0, 128)
    with _ffi.helper_streams(True):
        b = gptq_ops.gptq_quantize(W.clone(), U, False, 0.0, 15.0, 128)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
