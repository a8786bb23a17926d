"""Write tests/golden/mixed_quant.npz and tests/golden/ref_mixed_configs.json: the reference's mixed int / fp column paths
(IntegerQuantizer.fake_quant_act_dynamic / fake_quant_weight_dynamic with int_indices, quant.py:754-783, 833-869),
LlmInt8.get_outlier_indices (llmint8.py:25-34) and QUIK.block_opt's index choice (quik.py:91-126) on CPU.

Usage (where the reference tree exists; it needs no GPU):  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_mixed.py

The reference imports and CPU shims come from oracle/make_golden.py, read-only. The methods run unmodified, bound onto a
SimpleNamespace that carries what they read. Inputs and outputs are stored as bit patterns of the tensor dtype.

QUIK sorts its activation scales with torch.sort, whose order among equal values is not defined; the planted scales are all
distinct (asserted here), so the golden does not depend on it."""
import glob
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.make_golden import DT, GOLD, IntegerQuantizer, save  # noqa: E402
from oracle.build_ref import REF  # noqa: E402

from llmc.compression.quantization.llmint8 import LlmInt8  # noqa: E402  (reference)
from llmc.compression.quantization.quik import QUIK  # noqa: E402

REF_CONFIGS = os.path.join(REF, 'configs', 'quantization')
THRESHOLD = 6.0


def bits(t):
    """a tensor's own bit pattern (uint16 for 16-bit dtypes, uint32 for fp32)"""
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32).copy()
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def make_act(gen, shape, dt):
    """|x| well below the threshold, then planted outliers: 30 and -20, a value exactly at the threshold, and for a batch of
    two the same column over the threshold in both batch rows (the reference then lists it twice)."""
    x = torch.randn(*shape, generator=gen).clamp(-4, 4)
    B, T, K = shape
    x[0, T - 1, 7] = 30.0
    x[0, 1, 19] = -20.0
    x[0, 0, 11] = THRESHOLD
    if B > 1:
        x[1, 2, 7] = 30.0
        x[1, 0, K - 1] = -20.0
    return x.to(DT[dt])


def outlier_indices(x):
    ns = types.SimpleNamespace(threshold=THRESHOLD)
    return LlmInt8.get_outlier_indices(ns, x)


def run_act(name, shape, dt, gen, out):
    x = make_act(gen, shape, dt)
    int_ids, fp_ids = outlier_indices(x)
    q = IntegerQuantizer(8, True, 'per_token')
    y = q.fake_quant_act_dynamic(x, {'int_indices': int_ids, 'fp_indices': fp_ids})
    p = name + '/'
    out[p + 'dt'] = np.array(dt)
    out[p + 'shape'] = np.array(shape, np.int64)
    out[p + 'x_bits'], out[p + 'y_bits'] = bits(x), bits(y)
    out[p + 'int_ids'], out[p + 'fp_ids'] = int_ids.numpy().astype(np.int64), fp_ids.numpy().astype(np.int64)
    out[p + 'cfg'] = np.array(json.dumps(dict(bit=8, symmetric=True, granularity='per_token')))
    print(f'{name}: fp columns {fp_ids.tolist()}')
    return x, int_ids, fp_ids


def run_weight(name, w, cfg, int_ids, fp_ids, dt, out):
    q = IntegerQuantizer(cfg['bit'], cfg['symmetric'], cfg['granularity'],
                         **({'group_size': cfg['group_size']} if 'group_size' in cfg else {}))
    y = q.fake_quant_weight_dynamic(w, {'int_indices': int_ids, 'fp_indices': fp_ids})
    p = name + '/'
    out[p + 'dt'] = np.array(dt)
    out[p + 'shape'] = np.array(w.shape, np.int64)
    out[p + 'x_bits'], out[p + 'y_bits'] = bits(w), bits(y)
    out[p + 'int_ids'], out[p + 'fp_ids'] = int_ids.numpy().astype(np.int64), fp_ids.numpy().astype(np.int64)
    out[p + 'cfg'] = np.array(json.dumps(cfg))
    print(f'{name}: done')


def run_quik(gen, out):
    """QUIK.block_opt on one block of two Linears: fp_features 4 of K = 40, fp_threshold 0.0, all scales distinct."""
    K, prefix = 40, 'blocks'
    block = torch.nn.Module()
    block.q_proj = torch.nn.Linear(K, 8, bias=False)
    block.down_proj = torch.nn.Linear(K, 8, bias=False)
    scales = {}
    for n in ('q_proj', 'down_proj'):
        s = torch.rand(K, generator=gen) * 10 + 0.01
        assert torch.unique(s).numel() == K, 'planted activation scales must be all distinct'
        scales[f'{prefix}.0.{n}'] = s
        out[f'quik/{n}/scales'] = s.numpy().copy()
    ns = types.SimpleNamespace(prefix=prefix, block_idx=0, fp_relative=False, fp_features=4, fp_threshold=0.0,
                               act_scales=dict(scales),
                               model=types.SimpleNamespace(get_block_linears=lambda b: {n: m for n, m in b.named_modules()
                                                                                        if isinstance(m, torch.nn.Linear)}))
    QUIK.block_opt(ns, block)
    for n in ('q_proj', 'down_proj'):
        m = getattr(block, n)
        out[f'quik/{n}/int_ids'] = m.buf_int_ids.numpy().astype(np.int64)
        out[f'quik/{n}/fp_ids'] = m.buf_fp_ids.numpy().astype(np.int64)
        assert m.buf_fp_ids.numel() == 4 and m.buf_int_ids.numel() == K - 4
    out['quik/cfg'] = np.array(json.dumps(dict(fp_relative=False, fp_features=4, fp_threshold=0.0, K=K)))
    print('quik: done')


def configs():
    import yaml
    res = {}
    for f in sorted(glob.glob(REF_CONFIGS + '/**/*.y*ml', recursive=True)):
        try:
            c = yaml.safe_load(open(f))
        except Exception:       # noqa: BLE001
            continue
        q = (c or {}).get('quant') or {}
        if isinstance(q, dict) and q.get('method') in ('QUIK', 'LlmInt8'):
            rel = os.path.relpath(f, REF_CONFIGS)
            assert json.loads(json.dumps(c)) == c, f'{rel} does not survive JSON'
            res[rel] = c
    path = os.path.join(GOLD, 'ref_mixed_configs.json')
    with open(path, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(f'wrote {path}: {len(res)} files')


def main():
    gen = torch.Generator().manual_seed(20261019)
    out = {}
    act_names, weight_names = [], []
    kept = {}
    for shape in ((1, 5, 40), (2, 3, 72)):
        for dt in ('f16', 'bf16'):
            name = f'act_{shape[0]}x{shape[1]}x{shape[2]}_{dt}'
            kept[name] = run_act(name, shape, dt, gen, out)
            act_names.append(name)
    # weight [6, 40] int8 sym per_channel, cut by the columns LlmInt8 chose for the matching activation
    for dt in ('f16', 'bf16'):
        _, int_ids, fp_ids = kept[f'act_1x5x40_{dt}']
        w = (torch.randn(6, 40, generator=gen) * 0.05).to(DT[dt])
        name = f'w_6x40_int8_sym_per_channel_{dt}'
        run_weight(name, w, dict(bit=8, symmetric=True, granularity='per_channel'), int_ids, fp_ids, dt, out)
        weight_names.append(name)
    # the same for hidden size 72: the weight LlmInt8.w_qdq meets after a_qdq saw the [2, 3, 72] activation
    for dt in ('f16', 'bf16'):
        _, int_ids, fp_ids = kept[f'act_2x3x72_{dt}']
        w = (torch.randn(6, 72, generator=gen) * 0.05).to(DT[dt])
        name = f'w_6x72_int8_sym_per_channel_{dt}'
        run_weight(name, w, dict(bit=8, symmetric=True, granularity='per_channel'), int_ids, fp_ids, dt, out)
        weight_names.append(name)
    # weight [6, 48] int4 asym per_group g = 16: 32 integer columns in a random order, 8 fp columns, 8 columns left zero
    for dt in ('f16', 'bf16'):
        perm = torch.randperm(48, generator=gen)
        int_ids, fp_ids = perm[:32].clone(), perm[32:40].clone()
        w = (torch.randn(6, 48, generator=gen) * 0.05).to(DT[dt])
        name = f'w_6x48_int4_asym_per_group16_{dt}'
        run_weight(name, w, dict(bit=4, symmetric=False, granularity='per_group', group_size=16), int_ids, fp_ids, dt, out)
        weight_names.append(name)
    run_quik(gen, out)
    out['act_names'] = np.array(act_names)
    out['weight_names'] = np.array(weight_names)
    out['threshold'] = np.array(THRESHOLD)
    save('mixed_quant', **out)
    configs()


if __name__ == '__main__':
    main()
