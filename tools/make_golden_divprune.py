"""Write tests/golden/divprune.npz: the reference's divprune() (llmc/compression/token_reduction/divprune.py:19-53) unmodified on
the CPU, on supplied matrices and on exact features.

Usage (where the reference tree exists; it needs no GPU):  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_divprune.py

The reference's token_reduction package imports every method and through them VLM packages that need not be installed, so where
that import fails divprune.py is loaded as a module on its own: its package is a placeholder that carries only the directory, and
`.utils` (one decorator, behind a CLIP import) is replaced by a placeholder when it does not import either. divprune() itself runs
as it is written.

(a) selection on supplied matrices, each in f32, bf16 and f16 (a matrix is rounded to the dtype first, so all three select on
    values the dtype holds). Keys per case `a_<name>_<dt>`: 'dt', 'k', 'D_bits' (uint32 / uint16 [N, N]), 'sel' (int64 [k]).
      sym      random symmetric, zero diagonal, N = 48, k = 20      asym     random, not symmetric, N = 48, k = 20
      ties     symmetric, values in {0, 1/4, 1/2, 3/4}, N = 64, k = 30: most steps tie
      nan      `sym` with row and column 7 NaN, N = 48, k = 20       dup      1 - cos of 20 random tokens each present twice,
      full     `sym` with k = N = 48                                          computed by the reference in the dtype, k = 30 > 20
(b) exact features (tests/divprune_oracle.py: exact_tokens, EXACT_SHAPES), the reference computing the matrix itself in each dtype.
    Keys per shape `b_<N>_<d>`: 'N', 'd', 'k', 'seed', 'D' (fp32 [N, N]: the reference's matrix, asserted equal in the three
    dtypes and equal to the fp64 value), 'sel_<dt>' (int64 [k]), 'ties' (steps whose greatest score is shared).
(c) asserted on every recorded case: tests/divprune_oracle.py: select reproduces the reference's indices."""
import importlib
import importlib.util
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.make_golden import DT, save  # noqa: E402
from oracle.build_ref import REF  # noqa: E402

import divprune_oracle as O  # noqa: E402

SEED = 20261021


def reference_divprune():
    try:
        from llmc.compression.token_reduction.divprune import divprune
        return divprune
    except Exception as exc:          # noqa: BLE001  (a VLM package of another method that is not installed)
        print(f'the reference package does not import here ({type(exc).__name__}: {exc}); loading divprune.py on its own')
    here = os.path.join(REF, 'llmc', 'compression', 'token_reduction')
    pkg = 'llmc.compression.token_reduction'
    for name in [m for m in sys.modules if m.startswith(pkg)]:
        del sys.modules[name]
    holder = types.ModuleType(pkg)
    holder.__path__ = [here]
    sys.modules[pkg] = holder
    try:
        importlib.import_module(pkg + '.utils')
    except Exception:                 # noqa: BLE001
        utils = types.ModuleType(pkg + '.utils')
        utils.prefill_wrapper = lambda fn: fn
        sys.modules[pkg + '.utils'] = utils
    spec = importlib.util.spec_from_file_location(pkg + '.divprune', os.path.join(here, 'divprune.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.divprune


def bits(t):
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32).copy()
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def count_ties(D, sel):
    """steps of select() at which more than one index holds the greatest score"""
    K = O.keys(D)
    n, score = 0, None
    for i in range(len(sel)):
        if i == 0:
            score = np.partition(K, 1, axis=0)[1]
        elif i == 1:
            score = K[sel[0]].copy()
        else:
            row = K[sel[i - 1]]
            score = np.where((score == O.NAN_KEY) | (row == O.NAN_KEY), O.NAN_KEY, np.minimum(score, row))
        n += int((score == score.max()).sum() > 1)
    return n


def main():
    divprune = reference_divprune()
    gen = torch.Generator().manual_seed(SEED)
    out, names = {}, []

    def sym(n):
        a = torch.rand(n, n, generator=gen)
        a = (a + a.t()) / 2
        a.fill_diagonal_(0)
        return a

    base = sym(48)
    nan = base.clone()
    nan[7, :] = float('nan')
    nan[:, 7] = float('nan')
    q = torch.randint(0, 4, (64, 64), generator=gen).float() / 4
    q = torch.maximum(q, q.t())
    tokens = torch.randn(20, 32, generator=gen)
    tokens = torch.cat([tokens, tokens])[torch.randperm(40, generator=gen)]
    given = [('sym', base, 20), ('asym', torch.rand(48, 48, generator=gen), 20), ('ties', q, 30), ('nan', nan, 20), ('dup', None, 30),
             ('full', base, 48)]
    for name, M, k in given:
        for dname, dt in DT.items():
            if M is None:
                x = tokens.to(dt)
                _, D = divprune(x, 0, None, 1.0)                        # k = 0: the reference's own matrix in the dtype
            else:
                D = M.to(dt)
            s, same = divprune(D, k, D, 1.0)
            assert same is D and s.dtype == torch.long and tuple(s.shape) == (k,)
            s = s.numpy().copy()
            mine = O.select(D.float().numpy(), k)
            assert np.array_equal(mine, s), ('(c)', name, dname, mine, s)
            case = f'a_{name}_{dname}'
            names.append(case)
            out.update({f'{case}/dt': np.array(dname), f'{case}/k': np.array(k, np.int64), f'{case}/D_bits': bits(D),
                        f'{case}/sel': s})
            print(f'{case}: N {D.shape[0]} k {k} distinct chosen {len(set(s.tolist()))} ties {count_ties(D.float().numpy(), s)}')
        if name == 'dup':
            assert len(set(s.tolist())) < k, 'the duplicated tokens never made the reference choose an index twice'

    exact = []
    for N, d, k in O.EXACT_SHAPES:
        x = O.exact_tokens(N, d, SEED + N)
        truth = O.truth_dist(x)
        case = f'b_{N}_{d}'
        exact.append(case)
        ref32 = None
        for dname, dt in DT.items():
            xt = torch.from_numpy(x).to(dt)
            assert np.array_equal(xt.float().numpy(), x), (case, dname, 'the features are not exact in the dtype')
            s, D = divprune(xt, k, None, 1.0)
            assert D.dtype == dt
            Df = D.float().numpy()
            assert np.array_equal(Df.astype(np.float64), truth), (case, dname, 'the reference matrix is not the fp64 value')
            ref32 = Df if ref32 is None else ref32
            assert np.array_equal(ref32.view(np.uint32), Df.view(np.uint32))
            s = s.numpy().copy()
            assert np.array_equal(O.select(Df, k), s), ('(c)', case, dname)
            out[f'{case}/sel_{dname}'] = s
        ties = count_ties(ref32, out[f'{case}/sel_f32'])
        out.update({f'{case}/N': np.array(N, np.int64), f'{case}/d': np.array(d, np.int64), f'{case}/k': np.array(k, np.int64),
                    f'{case}/seed': np.array(SEED + N, np.int64), f'{case}/D': ref32, f'{case}/ties': np.array(ties, np.int64)})
        print(f'{case}: k {k}, {ties} steps tie, distinct distances {len(np.unique(ref32))}')
    out['names'] = np.array(names)
    out['exact'] = np.array(exact)
    save('divprune', **out)


if __name__ == '__main__':
    main()
