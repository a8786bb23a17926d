"""Write tests/golden/adadim.npz and tests/golden/ref_adadim_configs.json: the reference's AdaDim.search_dim_subset and
AdaDim.w_qdq (llmc/compression/quantization/adadim.py:21-88) on CPU, on planted fp16 layers.

Usage (where the reference tree exists; it needs no GPU):  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_adadim.py

The reference imports and CPU shims come from oracle/make_golden.py, read-only. The two methods run unmodified, unbound, on a
SimpleNamespace that carries what they read: the reference's IntegerQuantizer, n_samples and get_layer_out. The reference keeps
its two losses in a local dictionary, so get_layer_out is wrapped to record every output it returns; the losses stored here are
the reference's own expression, (org_out - out).float().pow(2).mean().item() with its weighting, on those recorded outputs, and
the decision they give is asserted equal to the buf_qdim the reference registered.

Planted layers, each R = 96, K = 128, three samples [1, 256, 128]: one outlier input column (x30, expected 'ic'), one outlier
output row (x30, expected 'oc'), and both (a column x30 and a row x6); the outliers are |w| x 30, of one sign like the
channels of a shifted activation (a signed x30 column leaves the two int4 losses within a factor 1.5: its own rounding error
dominates both), for int8 sym per_channel (the shipped config) and int4 asym per_group g = 32. A condition on the inputs: the reference's two losses differ by at least a factor 2 in every planted layer, so
that the decision does not hang on the rounding of a GEMM; the seed is advanced until the reference alone meets it."""
import glob
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.make_golden import GOLD, IntegerQuantizer, save  # noqa: E402
from oracle.build_ref import REF  # noqa: E402

from llmc.compression.quantization.adadim import AdaDim  # noqa: E402  (reference)

REF_CONFIGS = os.path.join(REF, 'configs', 'quantization')
R, K, TOKENS, N_SAMPLES = 96, 128, 256, 3
CASES = {
    'int8_sym_per_channel': dict(bit=8, symmetric=True, granularity='per_channel'),
    'int4_asym_per_group32': dict(bit=4, symmetric=False, granularity='per_group', group_size=32),
}
LAYERS = ('col', 'row', 'both')
EXPECTED = {'col': 0, 'row': 1}


def bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def plant(gen, kind):
    w = torch.randn(R, K, generator=gen) * 0.05
    if kind in ('col', 'both'):
        c = int(torch.randint(K, (1,), generator=gen))
        w[:, c] = w[:, c].abs() * 30
    if kind in ('row', 'both'):
        r = int(torch.randint(R, (1,), generator=gen))
        w[r] = w[r].abs() * (30 if kind == 'row' else 6)
    return w.half()


def run_case(cfg, seed):
    """-> dict of arrays, or None when a planted layer misses the factor-2 condition"""
    gen = torch.Generator().manual_seed(seed)
    layers = {}
    for kind in LAYERS:
        lin = torch.nn.Linear(K, R, bias=False).half()
        lin.weight.data = plant(gen, kind)
        layers[kind] = lin
    xs = [torch.randn(1, TOKENS, K, generator=gen).half() for _ in range(N_SAMPLES)]
    q = IntegerQuantizer(cfg['bit'], cfg['symmetric'], cfg['granularity'],
                         **({'group_size': cfg['group_size']} if 'group_size' in cfg else {}))
    recorded = []
    ns = types.SimpleNamespace(wquantizer=q, n_samples=N_SAMPLES)

    def get_layer_out(x, layer):
        out = AdaDim.get_layer_out(ns, x, layer)
        recorded.append(out.clone())
        return out
    ns.get_layer_out = get_layer_out
    weights = {k: m.weight.data.clone() for k, m in layers.items()}
    inputs = [x.clone() for x in xs]
    AdaDim.search_dim_subset(ns, layers, inputs)
    assert len(recorded) == len(LAYERS) * 2 * N_SAMPLES * 2
    out = {}
    for li, kind in enumerate(LAYERS):
        m = layers[kind]
        assert torch.equal(m.weight.data, weights[kind]), 'the reference leaves the weight in place'
        loss = {}
        for di, dim in enumerate(('oc', 'ic')):
            loss_mean = 0
            for i in range(N_SAMPLES):
                org_out, o = recorded[((li * 2 + di) * N_SAMPLES + i) * 2:][:2]
                loss_mean += xs[i].shape[0] * 1.0 / N_SAMPLES * (org_out - o).float().pow(2).mean().item()
            loss[dim] = loss_mean
        qdim = int(m.buf_qdim)
        assert qdim == (0 if loss['ic'] < loss['oc'] else 1), 'recorded losses do not give the reference\'s decision'
        print(f'  {kind}: oc {loss["oc"]:.6g}  ic {loss["ic"]:.6g}  -> buf_qdim {qdim}')
        lo, hi = sorted(loss.values())
        if not hi >= 2 * lo:
            return None
        if kind in EXPECTED and qdim != EXPECTED[kind]:
            return None
        out[f'{kind}/w_bits'] = bits(weights[kind])
        out[f'{kind}/losses'] = np.array([loss['oc'], loss['ic']], np.float64)
        out[f'{kind}/qdim'] = np.array(qdim, np.int64)
        out[f'{kind}/wq_bits'] = bits(AdaDim.w_qdq(ns, m, q))
    for i, x in enumerate(xs):
        out[f'x{i}_bits'] = bits(x)
    out['cfg'] = np.array(json.dumps(cfg))
    out['seed'] = np.array(seed, np.int64)
    return out


def configs():
    import yaml
    res = {}
    for f in sorted(glob.glob(REF_CONFIGS + '/**/*.y*ml', recursive=True)):
        try:
            c = yaml.safe_load(open(f))
        except Exception:       # noqa: BLE001
            continue
        q = (c or {}).get('quant') or {}
        if isinstance(q, dict) and q.get('method') == 'AdaDim':
            rel = os.path.relpath(f, REF_CONFIGS)
            assert json.loads(json.dumps(c)) == c, f'{rel} does not survive JSON'
            res[rel] = c
    path = os.path.join(GOLD, 'ref_adadim_configs.json')
    with open(path, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(f'wrote {path}: {len(res)} files')


def main():
    out = {}
    for name, cfg in CASES.items():
        for seed in range(20261019, 20261019 + 50):
            print(f'{name}: seed {seed}')
            res = run_case(cfg, seed)
            if res is not None:
                break
        else:
            raise SystemExit(f'{name}: no seed meets the factor-2 condition')
        out.update({f'{name}/{k}': v for k, v in res.items()})
    out['names'] = np.array(list(CASES))
    out['layers'] = np.array(LAYERS)
    out['shape'] = np.array([R, K, TOKENS, N_SAMPLES], np.int64)
    save('adadim', **out)
    configs()


if __name__ == '__main__':
    main()
