"""Write tests/golden/shortgpt.npz and tests/golden/ref_shortgpt_config.json: the reference's ShortGPT.compute_bi and
ShortGPT.remove_layers (llmc/compression/sparsification/shortgpt.py:40-55, 69-83) on CPU, on small seeded features.

Usage (where the reference tree exists; it needs no GPU):  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_shortgpt.py

The reference imports and CPU shims come from oracle/make_golden.py, read-only. The two methods run unmodified and unbound on a
SimpleNamespace that carries what they read: nothing for compute_bi; `importances`, `n_prune_layers` and `blocks` (a list of
the block numbers) for remove_layers. The JSON is the parsed shortgpt.yml (its sparse, calib and save sections: settings only).

Score cases, each input and output [2, 24, 96] (48 tokens): output = input + noise whose size grows from token to token, so the
per-token values span 3e-5 .. 0.3, in bf16, f16 and fp32; the bf16 case with input token 29 zeroed (the NaN -> 0.5 branch); the
bf16 case's input as its own output. Keys per case: 'dt', 'shape', 'source' (the case whose 'x_bits', 'y_bits' bit patterns it
reads: its own for the three random ones), 'zero_token' (the input row set to 0, or -1), 'same' (1: the output is the input),
'ref_bi' (what compute_bi returned, as exact float32), 'ref_total' (subset_transform's .sum().cpu().item()), 'ref_dist' (max
over the tokens of |ref_bi - fp64 truth|). tests/shortgpt_oracle.py: golden_case reads them back.
Removal: 'importances' (fp64 [6]), 'removed_n0', 'removed_n2' and 'blocks_n0', 'blocks_n2' (what remove_layers() returned and
left with n_prune_layers 0 and 2), 'explicit_in' = [1, 9, 4] (block 9 does not exist), 'explicit_out', 'explicit_blocks'.

The tool asserts what the tests lean on: (a) no two recorded importances are equal; (b) on every 16-bit case the numpy oracle's
total (tests/shortgpt_oracle.py) is at least as near the fp64 truth's as the reference's; (c) on the fp32 case every per-token
reference value lies within the oracle's derived bound plus ref_dist of the oracle's value."""
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.make_golden import DT, GOLD, save  # noqa: E402
from oracle.build_ref import REF  # noqa: E402

from llmc.compression.sparsification.shortgpt import ShortGPT  # noqa: E402  (reference)

import shortgpt_oracle as O  # noqa: E402

SHAPE = (2, 24, 96)
ZERO_TOKEN = 29


def bits(t):
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32).copy()
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def score_case(name, dname, x, y, source=None, zero_token=-1, same=False):
    ns = types.SimpleNamespace()
    ref = ShortGPT.compute_bi(ns, x, y)
    assert ref.dtype == x.dtype and tuple(ref.shape) == (SHAPE[0] * SHAPE[1],)
    ref_total = ref.sum().cpu().item()                                     # shortgpt.py:64-66
    xf, yf = x.float().numpy().reshape(-1, SHAPE[-1]), y.float().numpy().reshape(-1, SHAPE[-1])
    tr = O.truth(xf, yf)
    ours = O.block_influence(xf, yf, dname)
    ref_bi = ref.float().numpy().copy()
    ref_dist = float(np.abs(ref_bi.astype(np.float64) - tr).max())
    b = O.bound(SHAPE[-1], dname)
    assert float(np.abs(ours.astype(np.float64) - tr).max()) <= b, (name, 'the oracle leaves its own bound')
    ours_err, ref_err = abs(float(O.total(ours)) - tr.sum()), abs(ref_total - tr.sum())
    print(f'{name}: truth total {tr.sum():.9f}  oracle off by {ours_err:.3e}  reference off by {ref_err:.3e}  '
          f'per token: bound {b:.3e}, reference up to {ref_dist:.3e}, values {tr.min():.2e} .. {tr.max():.2e}')
    if dname != 'f32':
        assert ours_err <= ref_err, (name, '(b): the oracle total is farther from the truth than the reference')
    else:
        assert (np.abs(ours.astype(np.float64) - ref_bi) <= b + ref_dist).all(), (name, '(c)')
    out = {f'{name}/dt': np.array(dname), f'{name}/shape': np.array(SHAPE, np.int64), f'{name}/source': np.array(source or name),
           f'{name}/zero_token': np.array(zero_token, np.int64), f'{name}/same': np.array(int(same), np.int64),
           f'{name}/ref_bi': ref_bi, f'{name}/ref_total': np.array(ref_total, np.float64),
           f'{name}/ref_dist': np.array(ref_dist, np.float64)}
    if source is None:
        out[f'{name}/x_bits'], out[f'{name}/y_bits'] = bits(x).reshape(-1), bits(y).reshape(-1)
    return out


def removal(importances, n, explicit=None):
    ns = types.SimpleNamespace(importances=importances.copy(), n_prune_layers=n, blocks=list(range(len(importances))))
    out = ShortGPT.remove_layers(ns) if explicit is None else ShortGPT.remove_layers(ns, list(explicit))
    return np.array(out, np.int64), np.array(ns.blocks, np.int64)


def config():
    import yaml
    c = yaml.safe_load(open(os.path.join(REF, 'configs', 'sparsification', 'methods', 'ShortGPT', 'shortgpt.yml')))
    c = {k: c[k] for k in ('sparse', 'calib', 'save')}
    assert json.loads(json.dumps(c)) == c, 'shortgpt.yml does not survive JSON'
    path = os.path.join(GOLD, 'ref_shortgpt_config.json')
    with open(path, 'w') as fh:
        json.dump(c, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(f'wrote {path}')


def main():
    gen = torch.Generator().manual_seed(20261021)
    out, names = {}, []
    tokens = SHAPE[0] * SHAPE[1]
    noise = torch.logspace(-2, 0, tokens).reshape(SHAPE[0], SHAPE[1], 1)

    def features(dt):
        x = torch.randn(SHAPE, generator=gen) * torch.exp(0.5 * torch.randn(SHAPE[-1], generator=gen))
        return x.to(dt), (x + noise * torch.randn(SHAPE, generator=gen)).to(dt)

    kept = {}
    for dname, dt in DT.items():
        x, y = kept[dname] = features(dt)
        out.update(score_case(f'random_{dname}', dname, x, y))
        names.append(f'random_{dname}')
    x, y = (t.clone() for t in kept['bf16'])
    x.reshape(tokens, -1)[ZERO_TOKEN] = 0
    out.update(score_case('zero_token_bf16', 'bf16', x, y, source='random_bf16', zero_token=ZERO_TOKEN))
    assert out['zero_token_bf16/ref_bi'][ZERO_TOKEN] == 0.5
    x = kept['bf16'][0]
    out.update(score_case('same_bf16', 'bf16', x, x.clone(), source='random_bf16', same=True))
    names += ['zero_token_bf16', 'same_bf16']

    importances = (torch.rand(6, generator=gen, dtype=torch.float64) * 10).numpy()
    assert len(set(importances.tolist())) == 6, '(a): tied importances'
    out['importances'] = importances
    for n in (0, 2):
        out[f'removed_n{n}'], out[f'blocks_n{n}'] = removal(importances, n)
    assert out['removed_n0'].size == 0 and out['blocks_n0'].size == 6 and out['removed_n2'].size == 2 and out['blocks_n2'].size == 4
    out['explicit_in'] = np.array([1, 9, 4], np.int64)
    out['explicit_out'], out['explicit_blocks'] = removal(importances, 2, [1, 9, 4])
    assert out['explicit_out'].tolist() == [1, 9, 4] and out['explicit_blocks'].tolist() == [0, 2, 3, 5]
    print('importances', importances, 'removed', out['removed_n2'], 'left', out['blocks_n2'])
    out['names'] = np.array(names)
    save('shortgpt', **out)
    config()


if __name__ == '__main__':
    main()
