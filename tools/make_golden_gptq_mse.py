"""Write tests/golden/gptq_mse.npz: the reference's GPTQ.weight_transform with calib_algo='mse' and dynamic groups, on CPU.

Usage (where the reference tree exists; it needs no GPU):  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_gptq_mse.py

The reference imports, CPU shims and helpers come from oracle/make_golden.py, read-only. Every case stores the keys the
GPTQ suites of that file store (W0, perm, Wp, tmp, losses, g_scales, g_zeros, final_w, buf_scales(_dtype), buf_zeros,
w_qdq(_dtype), w_q_*, meta) plus W_after, the reference's running W after weight_transform: its visited columns hold the
block-start panels on which every group's range was searched. To stay small, the loop runs with a synthetic upper
factor (synth_upper; U_seed holds its seed and a checksum of its bits), values of the model dtype are stored as 16-bit
patterns (W0_bits, Wp_bits, w_qdq_bits), and final_w (tmp with the columns put back in original order) is stored for the
OWQ case only.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.make_golden import DT, IntegerQuantizer, _gptq_instance, f32, rand_weight, save  # noqa: E402

# (name, bit, sym, group_size, actorder, dtype, R, K, dead columns, extra quantizer kwargs, n_out (OWQ))
CASES = [
    ('w4a_g128_act_bf16_dead', 4, False, 128, True, 'bf16', 16, 384, True, {}, 0),
    ('w4s_g128_noact_f16', 4, True, 128, False, 'f16', 16, 256, False, {}, 0),
    ('w3a_g64_act_f16', 3, False, 64, True, 'f16', 16, 256, False, {}, 0),
    ('w4a_g32_act_bf16', 4, False, 32, True, 'bf16', 16, 256, False, {}, 0),
    ('w2s_g16_noact_f16', 2, True, 16, False, 'f16', 16, 256, False, {}, 0),
    ('w8a_g128_act_f16_shrink', 8, False, 128, True, 'f16', 16, 256, False,
     dict(maxshrink=0.5, mse_grid=50, mse_b_num=2), 0),
    ('w4a_g64_noact_f16_k320', 4, False, 64, False, 'f16', 16, 320, False, {}, 0),
    ('w4a_g128_owq_bf16', 4, False, 128, False, 'bf16', 16, 256, False, {}, 10),
]


def synth_upper(K, seed):
    """The upper factor both the reference loop and the tests run with (tests/test_gptq_mse_gpu.py restates it): the loop
    takes any upper factor, and one made of exact dyadic values from integer arithmetic is rebuilt anywhere bit for bit,
    so the fixture need not carry K x K floats. Off-diagonal entries in [-1/32, 1/32], diagonal in [0.5, 1.45]."""
    i = np.arange(K, dtype=np.int64)[:, None]
    j = np.arange(K, dtype=np.int64)[None, :]
    h = (i * 2654435761 + j * 40503 + seed * 7919) % 65521
    off = ((h % 257) - 128).astype(np.float32) / np.float32(4096.0)
    diag = np.float32(0.5) + (i % 61).astype(np.float32) / np.float32(64.0)
    return np.where(j > i, off, np.where(j == i, diag, np.float32(0.0))).astype(np.float32)


def bits16(t, dt):
    """values of a 16-bit dtype (held in any float tensor), as their 16-bit patterns"""
    return t.detach().to(DT[dt]).view(torch.int16).numpy().view(np.uint16).copy()


def main():
    import torch.distributed as dist
    if not dist.is_initialized():
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:29597', rank=0, world_size=1)
    out = {}
    gen = torch.Generator().manual_seed(4242)
    for ci, (name, bit, sym, gs, actorder, dt, R, K, dead, extra, n_out) in enumerate(CASES):
        keep_final = n_out > 0
        wq = IntegerQuantizer(bit, sym, 'per_group', group_size=gs, calib_algo='mse', **extra)
        g = _gptq_instance(wq, actorder, False, dtype=DT[dt])
        if n_out:
            g.owq, g.need_perm, g.n_out_dict = True, True, {'fc': n_out}
        layer = torch.nn.Linear(K, R, bias=False).to(DT[dt])
        layer.weight.data = rand_weight(gen, R, K, dt)
        # collect_block_qparams (base_blockwise_quantization.py:338-365)
        _, s0, z0, qmax, qmin = wq.get_tensor_qparams(layer.weight.data)
        layer.register_buffer('buf_scales', s0.detach())
        layer.register_buffer('buf_zeros', z0.detach())
        layer.register_buffer('buf_qmax', torch.tensor(qmax))
        layer.register_buffer('buf_qmin', torch.tensor(qmin))
        g.layers_cache['fc'] = {}
        g.layer_init(layer, 'fc')
        for _ in range(2):
            x = torch.randn(1, 96, K, generator=gen) * torch.exp(0.5 * torch.randn(K, generator=gen))
            x[..., 5] *= 30
            if dead:
                x[..., 17] = 0
                x[..., 200] = 0
            g.add_batch(layer, 'fc', x.to(DT[dt]), None)
        rtn_s, rtn_z = layer.buf_scales.clone(), layer.buf_zeros.clone()
        g.initialize_qparams_and_prepare_weights(layer, 'fc')
        perm = g.perm.clone() if (actorder or n_out) else None
        W0 = layer.weight.data.clone()
        Wp, _ = g.process_hessian_and_weights(layer, 'fc')
        U = torch.from_numpy(synth_upper(K, ci))
        Wp_in = Wp.clone()
        Losses, tmp, Wrun = torch.zeros_like(Wp), torch.zeros_like(Wp), Wp.clone()
        g.weight_transform(Wrun, U, Losses, tmp)
        p = name + '/'
        out[p + 'W0_bits'] = bits16(W0, dt)
        out[p + 'perm'] = perm.numpy().astype(np.int64) if perm is not None else np.zeros(0, np.int64)
        out[p + 'Wp_bits'] = bits16(Wp_in, dt)
        out[p + 'U_seed'] = np.array([ci, int(U.numpy().view(np.uint32).astype(np.uint64).sum())], np.int64)
        out[p + 'tmp'], out[p + 'losses'], out[p + 'W_after'] = f32(tmp), f32(Losses), f32(Wrun)
        out[p + 'g_scales'] = np.stack([f32(q['scale']).reshape(-1) for q in g.groups], axis=1)
        if not sym:
            out[p + 'g_zeros'] = np.stack([f32(q['zero']).reshape(-1) for q in g.groups], axis=1)
        out[p + 'rtn_scales'] = f32(rtn_s).reshape(-1)
        out[p + 'rtn_zeros'] = f32(rtn_z).reshape(-1) if rtn_z.dim() > 0 else np.zeros(0, np.float32)
        # finish the layer like update_layer_with_transformed_weights (gptq.py:186-196)
        t2 = tmp.clone()
        if perm is not None:
            t2[:, g.n_nonout:] = Wrun[:, g.n_nonout:]
            t2 = t2[:, torch.argsort(g.perm)]
        layer.weight.data = t2.reshape(layer.weight.shape)
        g.update_model_qparams(layer)
        out[p + 'final_w'] = f32(layer.weight.data) if keep_final else np.zeros(0, np.float32)
        out[p + 'buf_scales'] = f32(layer.buf_scales).reshape(-1)
        out[p + 'buf_scales_dtype'] = np.array(str(layer.buf_scales.dtype))
        bz = layer.buf_zeros
        out[p + 'buf_zeros'] = f32(bz).reshape(-1) if bz.dim() > 0 else np.zeros(0, np.float32)
        fq = g.w_qdq(layer, wq)
        out[p + 'w_qdq_bits'], out[p + 'w_qdq_dtype'] = bits16(fq, dt), np.array(str(fq.dtype))
        if not g.need_perm:
            cw, cs, cz = g.w_q(layer, wq)
            out[p + 'w_q_codes'] = cw.numpy().astype(np.uint8)      # low bytes: symmetric codes are negative
            out[p + 'w_q_scales'] = f32(cs)
            out[p + 'w_q_zeros'] = cz.numpy().astype(np.int32) if cz is not None else np.zeros(0, np.int32)
        out[p + 'meta'] = np.array([bit, int(sym), gs, int(actorder), 0, R, K, float(qmin), float(qmax), n_out,
                                    wq.maxshrink, wq.mse_grid, wq.mse_b_num, int(wq.round_zp)], dtype=np.float64)
        out[p + 'dt'] = np.array(dt)
    out['names'] = np.array([c[0] for c in CASES])
    save('gptq_mse', **out)


if __name__ == '__main__':
    main()
