"""SmoothQuant through the reference's own `main(config)` (tools/ref_pipeline.py, as tests/test_ref_pipeline_gpu.py does for the
other methods): configs/quantization/backend/vllm/smoothquant_w8a8.yml's quant section on the OPT architecture, once with the
reference's class and once after `llmc_amd.register_into(ALGO_REGISTRY, names=(..., 'SmoothQuant'))`. OPT because its norms are
nn.LayerNorm: the reference recognises a subset's norm through transformers' ALL_LAYERNORM_LAYERS, which no longer lists
LlamaRMSNorm, so on Llama the reference arm would transform nothing."""
import pytest

import test_ref_pipeline_gpu as P

pytestmark = pytest.mark.gpu


@P.needs_ref
def test_opt_smoothquant_w8a8_through_the_reference_main(tmp_path):
    res = P.run_arms(tmp_path, 'opt', ['smoothquant_w8a8'])
    w0 = P.original_weights(tmp_path, 'opt')
    stats, pa, pb = P.compare('opt_smoothquant_w8a8', *res['smoothquant_w8a8'])
    ref, ours = res['smoothquant_w8a8']
    moved = 0
    for n, st in stats.items():
        assert st['float_layer'] == 0.0, n
        # same inputs in both arms (the blocks stay in floating point until deploy), the same max / pow / div chain, the same
        # per_channel fake-quant at deploy: the deployed weights agree element for element up to isolated rounding ties
        assert st['w_close'] >= 0.999, (n, st)
        key = next(k for k in w0 if k.endswith(n.split('model.', 1)[-1]))
        if any(t in n for t in ('q_proj', 'k_proj', 'v_proj', 'fc1')):
            # the scale really was folded in: the deployed weight is not the fake-quantized original
            assert abs(ours[n + '/weight'] - w0[key]).max() > 0.05 * abs(w0[key]).max(), n
            moved += 1
    assert moved == 8                                      # q / k / v / fc1 of two blocks
    print('opt smoothquant_w8a8: w_equal', {n.rsplit('.', 2)[-2] + '.' + n.rsplit('.', 1)[-1]: round(st['w_equal'], 5) for n, st in stats.items()},
          'ppl', pa, pb)
    assert abs(pa - pb) <= 2e-3 * pa, (pa, pb)
