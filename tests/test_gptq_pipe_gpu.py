"""K4's column loop with helper streams against one stream, bit for bit, on the smallest shapes on which the two event dependencies
of the pipelined schedule exist: (256, 2048) has four column groups, so group 3 rewrites the err buffer that group 0's pieces on
the bulk stream read; n_quant = 1002 makes the last group's per-block updates reach [1002, 2048), which group 0's bulk pieces
also write. tests/test_gptq_pipe_plan.py is the guard against a race (it replays the plan on a CPU); this run shows that what the
executor issues computes what the plan says."""
import pytest
import torch

from llmc_amd import _ffi
from llmc_amd.compression.quantization import gptq_ops
from test_chain_riders_gpu import _inputs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('R,K,n_quant,mse', [(256, 2048, None, None), (256, 2048, 1002, None), (256, 2048, 1002, (1, 80, 100, 2.4))])
def test_helper_streams_on_and_off_same_bits(R, K, n_quant, mse):
    W, U = _inputs(R, K, R + K + (n_quant or 0))
    s0 = torch.ones(R, K // 128, device='cuda')
    z0 = torch.zeros(R, K // 128, device='cuda')
    out = []
    for on in (False, True):
        with _ffi.helper_streams(on):
            Wc = W.clone()
            res = gptq_ops.gptq_quantize(Wc, U, False, 0.0, 15.0, 128, n_quant=n_quant, init_scales=s0, init_zeros=z0, mse=mse)
            torch.cuda.synchronize()
            out.append((Wc,) + tuple(res))
    for name, a, b in zip(('W', 'tmp', 'losses', 'scales', 'zeros'), *out):
        assert torch.equal(a, b), name
