"""Write tests/golden/kvquant.npz: the reference's NaiveQuantKVCache and KiviQuantKVCache (llmc/compression/quantization/
kvquant.py) on CPU, step by step, on small seeded states.

Usage (where the reference tree exists; it needs no GPU):  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_kvquant.py

The reference imports and CPU shims come from oracle/make_golden.py, read-only. The two classes run unmodified. They lean on
attributes of transformers' DynamicCache that later releases dropped, so the tool sets them on the instance: _seen_tokens = 0 and
two empty lists key_cache / value_cache (Kivi's residuals).

Per case and step the file holds the bits of the states given to update(), of the keys / values it returned, and of
_quantized_key_cache[0] / _quantized_value_cache[0] after it: q_tensor, scales, zeros (16-bit tensors as uint16, fp32 as uint32;
q_tensor, integers held in the tensor dtype, as int16 values).
Keys: '<case>/<k|v>_<in|out|q|scales|zeros>', each the concatenation over the steps of the flattened arrays (a zip member per
step and array would cost more than its data); '<case>/rows' = the store's row count after each step; '<case>/meta' = [bit, sym,
granularity (0 per_token, 1 per_group, 2 per_tensor), group_size, B, H, T0, D, steps, kivi, residual_length]; 'names'. The
shapes follow from meta and rows: in [B, H, n, D] with n = T0 at step 0 and 1 after it, out [B, H, T0 + step, D], q
[B, H, rows, D], scales [B, H, rows, 1] / [B * H * rows * D / g, 1] / 0-dim, zeros like scales or a 0-dim 0.0 when symmetric
(tests/kvquant_oracle.py: golden_steps reads them back).

Cases, each in bf16 and fp16, [B, H, T0, D] = [1, 2, 5, 64], a prefill and 6 one-token decode steps: 8-bit symmetric per_token,
8-bit asymmetric per_token, 4-bit and 2-bit asymmetric per_group 32, 8-bit asymmetric per_tensor; one B = 2, D = 128 per_token
case ([2, 2, 3, 128], 2 decode steps); Kivi 4-bit asymmetric group 32 with residual_length 4 over 9 steps (two flushes: stores of 5 -> 9 -> 13 rows).
The tool asserts that in at least one bf16 case a stored code changes when it is derived again from its own dequantized value:
without that the file would not tell a cache that skips the requantization from one that does it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.make_golden import DT, save  # noqa: E402

from easydict import EasyDict  # noqa: E402  (oracle/_shims)
from llmc.compression.quantization.kvquant import KiviQuantKVCache, NaiveQuantKVCache  # noqa: E402  (reference)

GRAN = {'per_token': 0, 'per_group': 1, 'per_tensor': 2}


def bits(t):
    t = t.detach().contiguous()
    if t.dtype in (torch.float32, torch.float64):
        return t.float().view(torch.int32).numpy().view(np.uint32).copy()
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def states(gen, B, H, T, D, dt):
    x = torch.randn(B, H, T, D, generator=gen) * torch.exp(0.7 * torch.randn(1, H, 1, D, generator=gen))
    return x.to(dt)


def run_case(gen, name, dt, bit, sym, gran, group, B, H, T0, D, steps, kivi=False, residual_length=0):
    cfg = EasyDict(bit=bit, symmetric=sym, granularity=gran)
    if gran == 'per_group':
        cfg.group_size = group
    if kivi:
        cfg.residual_length = residual_length
    cache = (KiviQuantKVCache if kivi else NaiveQuantKVCache)('int-quant', cfg, 1)
    cache._seen_tokens = 0
    cache.key_cache, cache.value_cache = [], []
    out = {f'{name}/meta': np.array([bit, int(sym), GRAN[gran], group or 0, B, H, T0, D, steps, int(kivi), residual_length],
                                    np.int64)}
    changed, prev, rows, parts = 0, None, [], {}
    for s in range(steps):
        n = T0 if s == 0 else 1
        k, v = states(gen, B, H, n, D, dt), states(gen, B, H, n, D, dt)
        ko, vo = cache.update(k, v, 0, {})
        step = {'k_in': bits(k), 'v_in': bits(v), 'k_out': bits(ko), 'v_out': bits(vo)}
        assert ko.shape == vo.shape == (B, H, T0 + s, D) and ko.dtype == dt
        for tag, store in (('k', cache._quantized_key_cache[0]), ('v', cache._quantized_value_cache[0])):
            qt = store['q_tensor']
            assert qt.dtype == dt and bool((qt.float() == qt.float().round()).all())
            step[tag + '_q'] = qt.float().numpy().astype(np.int16)
            step[tag + '_scales'] = bits(store['scales'])
            step[tag + '_zeros'] = bits(store['zeros'])
        for key, arr in step.items():
            parts.setdefault(key, []).append(arr.reshape(-1))
        q = cache._quantized_key_cache[0]['q_tensor'].float()
        if prev is not None and q.shape[-2] > prev.shape[-2]:
            changed += int((q[:, :, :prev.shape[-2]] != prev).sum())
        prev = q
        rows.append(q.shape[-2])
        assert cache.get_seq_length() == T0 + s
    out.update({f'{name}/{key}': np.concatenate(v) for key, v in parts.items()})
    out[f'{name}/rows'] = np.array(rows, np.int64)
    return out, changed, rows


def main():
    gen = torch.Generator().manual_seed(20261020)
    out, names, changed_bf16 = {}, [], 0
    for dname in ('bf16', 'f16'):
        dt = DT[dname]
        for tag, bit, sym, gran, group in (('w8sym_tok', 8, True, 'per_token', None), ('w8asym_tok', 8, False, 'per_token', None),
                                           ('w4asym_g32', 4, False, 'per_group', 32), ('w2asym_g32', 2, False, 'per_group', 32),
                                           ('w8asym_tensor', 8, False, 'per_tensor', None)):
            name = f'naive_{dname}_{tag}'
            o, ch, rows = run_case(gen, name, dt, bit, sym, gran, group, 1, 2, 5, 64, 7)
            assert rows == [5, 6, 7, 8, 9, 10, 11], rows
            out.update(o)
            names.append(name)
            changed_bf16 += ch if dname == 'bf16' else 0
            print(f'{name}: {ch} stored codes changed by requantization')
        name = f'naive_{dname}_b2_d128'
        o, ch, rows = run_case(gen, name, dt, 8, False, 'per_token', None, 2, 2, 3, 128, 3)
        out.update(o)
        names.append(name)
        name = f'kivi_{dname}_w4asym_g32'
        o, ch, rows = run_case(gen, name, dt, 4, False, 'per_group', 32, 1, 2, 5, 64, 9, kivi=True, residual_length=4)
        assert rows == [5, 5, 5, 5, 9, 9, 9, 9, 13], rows
        out.update(o)
        names.append(name)
    assert changed_bf16 > 0, 'no bf16 case has a stored code changed by requantization'
    out['names'] = np.array(names)
    save('kvquant', **out)


if __name__ == '__main__':
    main()
