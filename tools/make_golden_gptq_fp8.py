"""Write tests/golden/gptq_fp8.npz: the reference's GPTQ with a FloatQuantizer weight quantizer (use_qtorch), on CPU.

Usage (where the reference tree exists; it needs no GPU):  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_gptq_fp8.py

The reference imports, CPU shims and helpers come from oracle/make_golden.py, read-only; float_quantize is bound to the
restated qtorch (_qtorch_stub) as suite_fp8_qtorch does. Every case stores what the GPTQ suites of that file store as far as
it applies to a symmetric float quantizer (W0, perm, Wp, tmp, losses, g_scales, final_w, buf_scales(_dtype) as the reference
leaves it, w_qdq(_dtype), the w_q weight bytes and scales, meta) plus W_after (the reference's running W after
weight_transform) and rtn_scales (the layer's buf_scales before the transform). To stay small the loop runs with the
synthetic upper factor of tools/make_golden_gptq_mse.py (synth_upper; U_seed holds its seed, a checksum of its bits and the
power of two its off-diagonal entries are multiplied by: the e5m2 outlier case runs with a strong factor, so that the in-block
feedback carries running weights more than 7 % past the maximum their group's scale was taken from — |w / s| >= 61440, where
e5m2 saturates; the tool asserts that it does) and
values of the model dtype are stored as 16-bit patterns (W0_bits, Wp_bits, w_qdq_bits, and the scales' own bits where they
are 16-bit tensors).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.make_golden import DT, _gptq_instance, _qtorch_stub, f32, rand_weight, save  # noqa: E402
from make_golden_gptq_mse import bits16, synth_upper  # noqa: E402

# (name, bit, group_size (0: per_channel), actorder, static_groups, dtype, R, K, dead columns, planted); U_AMP: the cases whose
# upper factor's off-diagonal entries are multiplied (by a power of two: exact)
U_AMP = {'e5m2_g128_noact_dyn_bf16_outliers': 32}
CASES = [
    ('e4m3_pc_act_bf16_dead', 'e4m3', 0, True, False, 'bf16', 16, 384, True, None),         # the shipped gptq_fp8.yml
    ('e5m2_pc_noact_f16', 'e5m2', 0, False, False, 'f16', 16, 256, False, None),
    ('e4m3_g128_act_dyn_bf16', 'e4m3', 128, True, False, 'bf16', 16, 256, False, None),
    ('e4m3_g64_act_static_f16', 'e4m3', 64, True, True, 'f16', 16, 256, False, None),
    ('e4m3_g32_noact_dyn_f16_k320', 'e4m3', 32, False, False, 'f16', 16, 320, False, None),  # 64-wide last block
    ('e4m3_pc_noact_f16_zero_row', 'e4m3', 0, False, False, 'f16', 16, 256, False, 'zero_row'),
    ('e5m2_g128_noact_dyn_bf16_outliers', 'e5m2', 128, False, False, 'bf16', 16, 256, False, 'outliers'),
]


def main():
    import torch.distributed as dist
    import llmc.compression.quantization.quant as qmod
    qmod.float_quantize = _qtorch_stub
    if not dist.is_initialized():
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:29598', rank=0, world_size=1)
    out = {}
    gen = torch.Generator().manual_seed(8448)
    for ci, (name, bit, gs, actorder, static_groups, dt, R, K, dead, planted) in enumerate(CASES):
        gran = 'per_group' if gs else 'per_channel'
        kw = dict(group_size=gs) if gs else {}
        wq = qmod.FloatQuantizer(bit, True, gran, use_qtorch=True, **kw)
        g = _gptq_instance(wq, actorder, static_groups, dtype=DT[dt])
        layer = torch.nn.Linear(K, R, bias=False).to(DT[dt])
        w = rand_weight(gen, R, K, dt)
        if planted == 'zero_row':
            w[3, :] = 0.0              # the RTN scale clamp(1e-5) / 448 underflows to 0 in fp16
        if planted == 'outliers':
            w[:, 100] *= 30            # late in its group: the running value leaves the range the group's scale was set from
            w[:, 250] *= 30
        layer.weight.data = w
        # collect_block_qparams (base_blockwise_quantization.py:338-365)
        _, s0, z0, qmax, qmin = wq.get_tensor_qparams(layer.weight.data)
        layer.register_buffer('buf_scales', s0.detach())
        layer.register_buffer('buf_zeros', z0.detach())
        layer.register_buffer('buf_qmax', torch.as_tensor(qmax))
        layer.register_buffer('buf_qmin', torch.as_tensor(qmin))
        g.layers_cache['fc'] = {}
        g.layer_init(layer, 'fc')
        for _ in range(2):
            x = torch.randn(1, 96, K, generator=gen) * torch.exp(0.5 * torch.randn(K, generator=gen))
            x[..., 5] *= 30
            if dead:
                x[..., 17] = 0
                x[..., 200] = 0
            g.add_batch(layer, 'fc', x.to(DT[dt]), None)
        rtn_s = layer.buf_scales.clone()
        g.initialize_qparams_and_prepare_weights(layer, 'fc')
        perm = g.perm.clone() if actorder else None
        W0 = layer.weight.data.clone()
        Wp, _ = g.process_hessian_and_weights(layer, 'fc')
        amp = U_AMP.get(name, 1)
        Un = synth_upper(K, 100 + ci)
        Un = np.where(np.eye(K, dtype=bool), Un, Un * np.float32(amp)).astype(np.float32)
        U = torch.from_numpy(Un)
        Wp_in = Wp.clone()
        Losses, tmp, Wrun = torch.zeros_like(Wp), torch.zeros_like(Wp), Wp.clone()
        g.weight_transform(Wrun, U, Losses, tmp)
        p = name + '/'
        out[p + 'W0_bits'] = bits16(W0, dt)
        out[p + 'perm'] = perm.numpy().astype(np.int64) if perm is not None else np.zeros(0, np.int64)
        out[p + 'Wp_bits'] = bits16(Wp_in, dt)
        out[p + 'U_seed'] = np.array([100 + ci, int(U.numpy().view(np.uint32).astype(np.uint64).sum()), amp], np.int64)
        out[p + 'tmp'], out[p + 'losses'], out[p + 'W_after'] = f32(tmp), f32(Losses), f32(Wrun)
        if gs:
            out[p + 'g_scales'] = np.stack([f32(q['scale']).reshape(-1) for q in g.groups], axis=1)
            assert all(float(q['zero']) == 0.0 and q['zero'].dim() == 0 for q in g.groups)
        else:
            out[p + 'g_scales'] = f32(g.qparams['scale']).reshape(-1, 1)
            assert float(g.qparams['zero']) == 0.0
        out[p + 'rtn_scales'] = f32(rtn_s).reshape(-1)
        out[p + 'rtn_scales_dtype'] = np.array(str(rtn_s.dtype))
        # finish the layer like update_layer_with_transformed_weights (gptq.py:186-196)
        t2 = tmp.clone()
        if perm is not None:
            t2 = t2[:, torch.argsort(g.perm)]
        layer.weight.data = t2.reshape(layer.weight.shape)
        if gs and not static_groups:
            g.update_model_qparams(layer)
        out[p + 'final_w'] = f32(layer.weight.data)
        out[p + 'buf_scales'] = f32(layer.buf_scales).reshape(-1)
        out[p + 'buf_scales_dtype'] = np.array(str(layer.buf_scales.dtype))
        fq = g.w_qdq(layer, wq)
        out[p + 'w_qdq_bits'], out[p + 'w_qdq_dtype'] = bits16(fq, dt), np.array(str(fq.dtype))
        if not g.need_perm:
            cw, cs, cz = g.w_q(layer, wq)
            assert cz is None
            out[p + 'w_q_bytes'] = cw.view(torch.uint8).numpy().copy()
            out[p + 'w_q_dtype'] = np.array(str(cw.dtype))
            out[p + 'w_q_scales'] = f32(cs)
            out[p + 'w_q_scales_dtype'] = np.array(str(cs.dtype))
        out[p + 'meta'] = np.array([wq.e_bits, wq.m_bits, gs, int(actorder), int(static_groups), R, K, float(qmin), float(qmax)],
                                   dtype=np.float64)
        out[p + 'dt'] = np.array(dt)
        out[p + 'bit'] = np.array(bit)
        # the largest scaled value the loop rounded: tmp holds every weight as it was when visited, so tmp / s is the very
        # quotient (both fp32). e4m3 saturates from 248 on (the scale maps the range to 448, the grid ends at 240); e5m2 only
        # from 61440 on, beyond the range the scale was taken from: the outlier case exists to reach it
        sc = out[p + 'g_scales']
        if gs and not static_groups:
            col_s = np.repeat(sc, gs, axis=1)[:, :K]
        elif gs:
            col_s = sc[:, (perm.numpy() if perm is not None else np.arange(K)) // gs]
        else:
            col_s = np.repeat(sc, K, axis=1)
        t = np.abs(out[p + 'tmp'] / col_s)
        nsat = int((t >= (248.0 if bit == 'e4m3' else 61440.0)).sum())
        print(f'{name}: max |w / s| = {t.max():.1f} (format max {float(qmax)}), {nsat} saturating elements, '
              f'max |tmp| = {np.abs(out[p + "tmp"]).max():.3g}')
        assert np.isfinite(out[p + 'tmp']).all() and np.isfinite(out[p + 'losses']).all(), name
        assert nsat > 0 or (bit == 'e5m2' and planted != 'outliers'), name
    out['names'] = np.array([c[0] for c in CASES])
    save('gptq_fp8', **out)


if __name__ == '__main__':
    main()
