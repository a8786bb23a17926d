"""Write tests/golden/fp4.npz: the reference's FloatQuantizer on the narrow grids e2m1 / e3m2 (use_qtorch), on CPU.

Usage (where the reference tree exists; it needs no GPU):  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_fp4.py

The reference imports, CPU shims and helpers come from oracle/make_golden.py, read-only; float_quantize is bound to the
restated qtorch (_qtorch_stub) as suite_fp8_qtorch does, so the reference's own class code around it (qmax = tensor(6) /
tensor(28), the division in the tensor dtype, the fp32 dequantisation product) runs unchanged. Per case: the input (x_bits),
the scales get_tensor_qparams / get_batch_tensors_qparams return (scales, fp32 container, with scales_dtype), the fake_quant_*
output (fake_bits), quant()'s output (q, fp32) and, for the case marked so, fake_quant_weight_static with given scales
(static_scales, static_fake_bits). Values of the model dtype are stored as 16-bit patterns.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.make_golden import DT, _qtorch_stub, f32, save  # noqa: E402
from make_golden_gptq_mse import bits16  # noqa: E402

# (name, bit, kind, granularity, group_size, dtype, shape, planted)
CASES = [
    ('e2m1_g128_bf16', 'e2m1', 'weight', 'per_group', 128, 'bf16', (5, 384), 'static'),
    ('e2m1_g128_f16_zero_row', 'e2m1', 'weight', 'per_group', 128, 'f16', (5, 384), 'zero_row'),   # an all-zero row: the scale clamp(1e-5) / 6 stays an fp16 subnormal
    ('e2m1_g32_f16', 'e2m1', 'weight', 'per_group', 32, 'f16', (4, 96), None),
    ('e2m1_pc_bf16_outlier', 'e2m1', 'weight', 'per_channel', 0, 'bf16', (3, 320), 'outlier'),
    ('e2m1_pt_bf16', 'e2m1', 'weight', 'per_tensor', 0, 'bf16', (3, 320), None),                    # pins the scale dtype
    ('e3m2_g64_bf16', 'e3m2', 'weight', 'per_group', 64, 'bf16', (4, 192), None),
    ('e2m1_token_bf16', 'e2m1', 'act_dynamic', 'per_token', 0, 'bf16', (2, 7, 320), None),
    ('e2m1_static_pt_bf16', 'e2m1', 'act_static', 'per_tensor', 0, 'bf16', (2, 7, 320), None),
]


def main():
    import llmc.compression.quantization.quant as qmod
    qmod.float_quantize = _qtorch_stub
    out = {}
    gen = torch.Generator().manual_seed(4016)
    for name, bit, kind, gran, gs, dt, shape, planted in CASES:
        kw = dict(group_size=gs) if gs else {}
        if kind == 'act_static':
            kw['calib_algo'] = 'static_minmax'
        q = qmod.FloatQuantizer(bit, True, gran, use_qtorch=True, **kw)
        assert q.qmax.dtype == torch.int64 and q.qmax.dim() == 0
        x = torch.randn(*shape, generator=gen) * (0.05 if kind == 'weight' else 1.0)
        if kind != 'weight':
            x = x * torch.exp(0.7 * torch.randn(shape[-1], generator=gen))
        if planted == 'zero_row':
            x[2, :] = 0.0
        if planted == 'outlier':
            x[:, 77] *= 30
        x = x.to(DT[dt])
        x.view(-1)[3] = 0.0
        x.view(-1)[4] = -0.0
        p = name + '/'
        out[p + 'x_bits'] = bits16(x, dt)
        if kind == 'act_static':
            s_list, z_list, qmin_list, qmax_list = q.get_batch_tensors_qparams([x])
            scales, zeros, qmax, qmin = s_list[0], z_list[0], qmax_list[0], qmin_list[0]
            t = q.reshape_tensor(x)
            fake = q.fake_quant_act_static(x, dict(scales=scales.clone(), zeros=zeros, qmax=qmax, qmin=qmin))
        else:
            t, scales, zeros, qmax, qmin = q.get_tensor_qparams(x)
            fake = q.fake_quant_weight_dynamic(x) if kind == 'weight' else q.fake_quant_act_dynamic(x)
        assert fake.dtype == DT[dt] and float(zeros) == 0.0
        out[p + 'scales'] = f32(scales).reshape(-1)
        out[p + 'scales_dtype'] = np.array(str(scales.dtype))
        out[p + 'fake_bits'] = bits16(fake, dt)
        qv = q.quant(t, scales.clone(), zeros, qmax, qmin)
        assert qv.dtype == torch.float32
        out[p + 'q'] = f32(qv)
        if planted == 'static':
            s2 = (scales.float() * (0.5 + torch.rand(scales.shape, generator=gen))).to(scales.dtype)
            sf = q.fake_quant_weight_static(x, dict(scales=s2.clone(), zeros=zeros, qmax=qmax, qmin=qmin))
            out[p + 'static_scales'] = f32(s2).reshape(-1)
            out[p + 'static_fake_bits'] = bits16(sf, dt)
        out[p + 'meta'] = np.array([q.e_bits, q.m_bits, q.num_bits, gs, float(qmin), float(qmax)], dtype=np.float64)
        out[p + 'dt'], out[p + 'bit'], out[p + 'kind'], out[p + 'gran'] = np.array(dt), np.array(bit), np.array(kind), np.array(gran)
        lv = np.unique(np.abs(out[p + 'q']))
        print(f'{name}: scales {scales.dtype} {tuple(scales.shape)}, |q| levels {lv.tolist()}')
    out['names'] = np.array([c[0] for c in CASES])
    save('fp4', **out)


if __name__ == '__main__':
    main()
