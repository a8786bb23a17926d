"""Write tests/golden/hqq.npz: the reference's HQQ solver (hqq.py, quant.py:588-610, 680-697) on CPU.

Usage (where the reference tree exists; it needs no GPU):  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_hqq.py

The reference imports and CPU shims come from oracle/make_golden.py, read-only. Per case: the weight (16-bit patterns),
the quantizer / special settings, the min / max qparams the reference starts from, its result (scales, zeros), the
per-iteration errors HQQ.optimize_weights_proximal logs (hqq.py:51, forwarded by the loguru shim to `logging`) and the
stop iteration. One case runs HQQ.block_opt + w_qdq on a two-Linear block. The shipped hqq_w_only.yml quant section is
stored as JSON text (`shipped_quant`).
"""
import json
import logging
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.make_golden import DT, IntegerQuantizer, f32, save  # noqa: E402

from llmc.compression.quantization.hqq import HQQ  # noqa: E402  (reference)

SHIPPED = os.path.join('/root/reference', 'configs', 'quantization', 'methods', 'HQQ', 'hqq_w_only.yml')

# (name, R, K, dt, sigma, weight kind, bit, sym, group_size, round_zp, special {axis, lp_norm, beta, kappa, iters},
#  quantizer calib_algo hqq kwargs or None, expect a stop before iters). Axis-0 cases have R >= 2 g: then reshape_tensor
#  copies W.T and the group mean is ATen's contiguous inner sum. (With R <= g the reference reduces a strided view of W.T,
#  whose order ATen's outer-sum kernel sets)
SHIP = dict(axis=0, lp_norm=0.7, beta=10, kappa=1.01, iters=20)
CASES = [
    ('ship_ax0_s002', 256, 128, 'bf16', 0.02, 'llm', 4, False, 128, False, SHIP, None, False),
    ('ship_ax1_s002', 128, 256, 'bf16', 0.02, 'llm', 4, False, 128, False, dict(SHIP, axis=1), None, False),
    ('ship_ax0_s2', 256, 128, 'bf16', 2.0, 'normal', 4, False, 128, False, SHIP, None, False),
    ('ship_ax1_s1', 128, 256, 'f16', 1.0, 'normal', 4, False, 128, False, dict(SHIP, axis=1), None, False),
    ('brk_ax0_i100', 256, 128, 'bf16', 0.02, 'normal', 4, False, 128, False, dict(SHIP, iters=100), None, True),
    ('brk_ax1_i100', 64, 1024, 'bf16', 0.02, 'normal', 4, False, 128, False, dict(SHIP, axis=1, iters=100), None, True),
    ('grid_tie_ax1', 32, 256, 'bf16', 0.0, 'grid', 4, False, 64, False, dict(SHIP, axis=1), None, True),
    ('g32_ax1_f16', 64, 256, 'f16', 0.02, 'llm', 4, False, 32, False, dict(SHIP, axis=1), None, False),
    ('g64_ax0_bf16', 128, 128, 'bf16', 0.02, 'llm', 4, False, 64, False, SHIP, None, False),
    ('w3_g16_ax1_s5', 32, 256, 'bf16', 5.0, 'normal', 3, False, 16, False, dict(SHIP, axis=1), None, False),
    ('w8_ax0', 256, 128, 'f16', 0.02, 'llm', 8, False, 128, False, SHIP, None, False),
    ('sym4_ax1', 64, 256, 'bf16', 0.02, 'llm', 4, True, 128, False, dict(SHIP, axis=1), None, False),
    ('rzp_ax0', 256, 128, 'bf16', 0.02, 'llm', 4, False, 128, True, SHIP, None, False),
    ('lp1_ax1_s1', 64, 256, 'bf16', 1.0, 'normal', 4, False, 64, False, dict(SHIP, axis=1, lp_norm=1), None, False),
    ('iters3_ax1', 64, 256, 'f16', 0.02, 'llm', 2, False, 32, False, dict(SHIP, axis=1, iters=3), None, False),
    ('double_ax0', 256, 128, 'bf16', 0.5, 'normal', 4, False, 128, False, SHIP,
     dict(lp_norm=0.6, beta=5, kappa=1.05, iters=4), False),
]


def bits16(t, dt):
    return t.detach().to(DT[dt]).view(torch.int16).numpy().view(np.uint16).copy()


class _Log(logging.Handler):
    def __init__(self):
        super().__init__()
        self.errs = []

    def emit(self, rec):
        m = re.match(r'iter : (\d+), error : (\S+)', rec.getMessage())
        if m:
            self.errs.append(float(m.group(2)))


def make_weight(gen, R, K, dt, sigma, kind, bit):
    if kind == 'grid':
        # values already on each group's quantization grid: every row of 64 holds codes 0 and 2^bit - 1, step 2^-6
        codes = torch.randint(0, 2 ** bit, (R, K), generator=gen).float()
        codes[:, ::64] = 0
        codes[:, 1::64] = 2 ** bit - 1
        return (codes * 2.0 ** -6).to(DT[dt])
    w = torch.randn(R, K, generator=gen) * sigma
    if kind == 'llm':       # 0.1 % outliers x20, like LLM weights
        m = torch.rand(R, K, generator=gen) < 1e-3
        w = torch.where(m, w * 20, w)
    # a constant group and an all-zero group for both axes: rows 0..15 of columns 0..15 and rows 16..31 of column 16..31
    w[:16, :16] = 0.0
    w[16:32, 16:32] = 0.0173
    return w.to(DT[dt])


def hqq_instance(wq, special):
    h = HQQ.__new__(HQQ)
    h.quant_config = {'special': dict(special)}
    h.wquantizer = wq
    h.add_quant_config()
    return h


def main():
    log = logging.getLogger('llmc-ref')
    log.setLevel(logging.INFO)
    cap = _Log()
    log.addHandler(cap)
    gen = torch.Generator().manual_seed(20261016)
    out = {}
    for (name, R, K, dt, sigma, kind, bit, sym, gs, rzp, special, qhqq, expect_stop) in CASES:
        kw = dict(group_size=gs, round_zp=rzp)
        if qhqq:
            kw.update(calib_algo='hqq', **qhqq)
        wq = IntegerQuantizer(bit, sym, 'per_group', **kw)
        W = make_weight(gen, R, K, dt, sigma, kind, bit)
        h = hqq_instance(wq, special)
        # HQQ.block_opt's per-layer steps (hqq.py:70-84)
        tensor = W.float()
        if special['axis'] == 0:
            tensor = tensor.T
        qm = IntegerQuantizer(bit, sym, 'per_group', group_size=gs, round_zp=rzp)
        _, s_mm, z_mm, _, _ = qm.get_tensor_qparams(tensor)
        tensor, s0, z0, qmax, qmin = wq.get_tensor_qparams(tensor)
        cap.errs = []
        s, z = h.optimize_weights_proximal(tensor, s0, z0, qmax, qmin)
        errs = np.array(cap.errs, np.float64)
        n = len(errs)
        stopped = n < special['iters'] or (n >= 2 and np.float32(errs[-1]) >= np.float32(errs[:-1]).min())
        if expect_stop:
            assert stopped, f'{name}: expected a stop, ran {n} of {special["iters"]} iterations'
        p = name + '/'
        out[p + 'W_bits'] = bits16(W, dt)
        out[p + 'dt'] = np.array(dt)
        out[p + 'meta'] = np.array([R, K, bit, int(sym), gs, int(rzp), special['axis'], special['lp_norm'], special['beta'],
                                    special['kappa'], special['iters'], float(qmin), float(qmax), sigma], np.float64)
        out[p + 'qhqq'] = np.array([qhqq['lp_norm'], qhqq['beta'], qhqq['kappa'], qhqq['iters']] if qhqq else [],
                                   np.float64)
        out[p + 's_mm'], out[p + 'z_mm'] = f32(s_mm).reshape(-1), f32(z_mm).reshape(-1)
        out[p + 's_start'], out[p + 'z_start'] = f32(s0).reshape(-1), f32(z0).reshape(-1)
        out[p + 'scales'], out[p + 'zeros'] = f32(s).reshape(-1), f32(z).reshape(-1)
        out[p + 'errs'] = errs
        out[p + 'T'] = np.array(n - 1, np.int64)
        out[p + 'stopped'] = np.array(int(stopped))
        print(f'{name}: T={n - 1} stopped={stopped}')
    out['names'] = np.array([c[0] for c in CASES])

    # HQQ.block_opt + w_qdq on a block of two Linears (axis 0, the shipped special)
    class _Model:
        def __init__(self, block):
            self.block = block

        def get_block_linears(self, block):
            return {'fc1': block[0], 'fc2': block[1]}

    block = torch.nn.Sequential(torch.nn.Linear(128, 256, bias=False), torch.nn.Linear(128, 256, bias=False)).to(torch.bfloat16)
    for lin in block:
        lin.weight.data = make_weight(gen, lin.weight.shape[0], lin.weight.shape[1], 'bf16', 0.02, 'llm', 4)
    wq = IntegerQuantizer(4, False, 'per_group', group_size=128, round_zp=False)
    h = hqq_instance(wq, SHIP)
    h.model = _Model(block)
    W0 = [bits16(lin.weight.data, 'bf16') for lin in block]
    h.block_opt(block)
    for i, lin in enumerate(block):
        p = f'block/fc{i + 1}/'
        out[p + 'W_bits'] = W0[i]
        out[p + 'buf_scales'] = f32(lin.buf_scales).reshape(-1)
        out[p + 'buf_zeros'] = f32(lin.buf_zeros).reshape(-1)
        out[p + 'buf_shape'] = np.array(list(lin.buf_scales.shape), np.int64)
        out[p + 'qdq_bits'] = bits16(h.w_qdq(lin, wq), 'bf16')
    import yaml
    with open(SHIPPED) as fh:
        out['shipped_quant'] = np.array(json.dumps(yaml.safe_load(fh)['quant']))
    save('hqq', **out)


if __name__ == '__main__':
    main()
