"""Write tests/golden/sparse.npz and tests/golden/ref_sparse_configs.json: the reference's Wanda.get_row_scale,
Wanda.subset_transform (llmc/compression/sparsification/wanda.py:16-56) and Magnitude.subset_transform (magnitude.py:15-31)
on CPU, on small seeded layers.

Usage (where the reference tree exists; it needs no GPU):  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_sparse.py

The reference imports and CPU shims come from oracle/make_golden.py, read-only (its shim makes Tensor.cuda() the identity, so
magnitude.py:27 runs on CPU). The methods run unmodified and unbound on a SimpleNamespace that carries what they read:
`sparser.sparsity` (which the reference itself never defines) and, for Wanda, get_row_scale. Magnitude.subset_transform zeroes
only the LAST layer of a subset (its masked assignment sits after the loop), so it is given one-layer subsets. It keeps its
threshold in a local; the threshold stored here is this tool's restatement of magnitude.py:27-29,
torch.sort(|W|.flatten())[0][int(numel * sparsity)], checked against what the reference left: every |w| <= thresh is zero and
every other element has its own bits.

Wanda cases, each R = 24, K = 96, activations [3, 20, 96]: random weights in bf16 / fp16 / fp32 at sparsity 0.5 and 0.3 (no
exact zero among the weights, so the reference's mask is `pruned == 0`), and a bf16 case whose weights take 7 distinct values
under a two-valued activation norm, full of ties that only the stable sort decides. Magnitude cases: bf16 / fp16 / fp32
[24, 96] at sparsity 0.5."""
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.make_golden import DT, GOLD, save  # noqa: E402
from oracle.build_ref import REF  # noqa: E402

from llmc.compression.sparsification.magnitude import Magnitude  # noqa: E402  (reference)
from llmc.compression.sparsification.wanda import Wanda  # noqa: E402  (reference)

REF_CONFIGS = os.path.join(REF, 'configs', 'sparsification', 'methods')
R, K, N_SEQ, TOKENS = 24, 96, 3, 20


def bits(t):
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32).copy()
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def linear(w):
    lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=False)
    lin.weight.data = w.clone()
    return lin


def wanda_case(w, act, sparsity):
    ns = types.SimpleNamespace(sparser=types.SimpleNamespace(sparsity=sparsity))
    ns.get_row_scale = lambda layer, a: Wanda.get_row_scale(ns, layer, a)
    lin = linear(w)
    scaler_row = Wanda.get_row_scale(ns, lin, act)
    Wanda.subset_transform(ns, {'layers': {'fc': lin}, 'input': ['fc']}, {'fc': [act]}, {})
    out = {'w_bits': bits(w), 'act_bits': bits(act), 'scaler_row': scaler_row.numpy().copy(),
           'pruned_bits': bits(lin.weight.data), 'sparsity': np.array(sparsity, np.float64),
           'n_prune': np.array(int(K * sparsity), np.int64)}
    if not (w == 0).any():
        mask = (lin.weight.data == 0)
        assert int(mask.sum()) == R * int(K * sparsity)
        out['mask'] = mask.numpy().astype(np.uint8)
    return out


def magnitude_case(w, sparsity):
    ns = types.SimpleNamespace(sparser=types.SimpleNamespace(sparsity=sparsity))
    lin = linear(w)
    Magnitude.subset_transform(ns, {'layers': {'fc': lin}}, {}, {})
    kth = int(w.numel() * sparsity)
    thresh = torch.sort(torch.abs(w).flatten())[0][kth]                      # magnitude.py:27-29, restated
    got = lin.weight.data
    cut = torch.abs(w) <= thresh
    assert bool((got[cut] == 0).all()) and np.array_equal(bits(got)[~cut.numpy()], bits(w)[~cut.numpy()])
    return {'w_bits': bits(w), 'pruned_bits': bits(got), 'thresh_bits': bits(thresh.reshape(1)), 'kth': np.array(kth, np.int64),
            'mask': cut.numpy().astype(np.uint8), 'sparsity': np.array(sparsity, np.float64)}


def configs():
    import yaml
    res = {}
    for rel in ('Wanda/wanda.yml', 'Magnitude/magnitude.yml'):
        c = yaml.safe_load(open(os.path.join(REF_CONFIGS, rel)))
        c = {k: c[k] for k in ('sparse', 'calib', 'save')}
        assert json.loads(json.dumps(c)) == c, f'{rel} does not survive JSON'
        res[rel] = c
    path = os.path.join(GOLD, 'ref_sparse_configs.json')
    with open(path, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(f'wrote {path}: {len(res)} files')


def main():
    gen = torch.Generator().manual_seed(20261020)
    out, wanda_names, mag_names = {}, [], []
    for dname, dt in DT.items():
        w = (torch.randn(R, K, generator=gen) * 0.05).to(dt)
        w[w == 0] = 0.01
        act = (torch.randn(N_SEQ, TOKENS, K, generator=gen) * torch.exp(0.5 * torch.randn(K, generator=gen))).to(dt)
        for sparsity in (0.5, 0.3):
            name = f'wanda_{dname}_s{int(sparsity * 100)}'
            out.update({f'{name}/{k}': v for k, v in wanda_case(w, act, sparsity).items()})
            wanda_names.append(name)
        name = f'magnitude_{dname}'
        out.update({f'{name}/{k}': v for k, v in magnitude_case(w, 0.5).items()})
        mag_names.append(name)
    vals = torch.tensor([-0.5, -0.25, 0.0, 0.125, 0.25, 0.5, 1.0])
    w = vals[torch.randint(7, (R, K), generator=gen)].to(torch.bfloat16)
    act = torch.ones(N_SEQ, TOKENS, K)
    act[:, :, K // 2:] = 2.0
    out.update({f'wanda_ties/{k}': v for k, v in wanda_case(w, act.to(torch.bfloat16), 0.5).items()})
    wanda_names.append('wanda_ties')
    out['wanda_names'] = np.array(wanda_names)
    out['magnitude_names'] = np.array(mag_names)
    save('sparse', **out)
    configs()


if __name__ == '__main__':
    main()
