"""HQQ on the CPU: configuration, refusals, the solver's scalars and sum order, and the numpy oracle (tests/hqq_oracle.py)
against the reference's own results (tests/golden/hqq.npz, tools/make_golden_hqq.py)."""
import ast
import inspect
import json
import os

import numpy as np
import pytest
import torch

import hqq_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden', 'hqq.npz')
REF_HQQ = os.path.join(os.path.dirname(HERE), 'oracle', '_ref', 'llmc', 'compression', 'quantization', 'hqq.py')
f32 = np.float32
DT = {'bf16': torch.bfloat16, 'f16': torch.float16}


def _gold():
    return np.load(GOLD)


def case_weight(z, name):
    dt = str(z[name + '/dt'])
    bits = torch.from_numpy(z[name + '/W_bits'].view(np.int16).copy())
    return bits.view(DT[dt]).float().numpy()


def case_settings(z, name):
    R, K, bit, sym, gs, rzp, axis, lp, beta, kappa, iters, qmin, qmax, sigma = z[name + '/meta']
    return dict(R=int(R), K=int(K), bit=int(bit), sym=bool(sym), gs=int(gs), round_zp=bool(rzp), axis=int(axis),
                lp_norm=float(lp), beta=float(beta), kappa=float(kappa), iters=int(iters), qmin=float(qmin),
                qmax=float(qmax))


def oracle_case(z, name, stop_at=None):
    """the oracle's run of one golden case from the weight alone (min / max start, and the quantizer's own solve first
    when the case has calib_algo hqq on the quantizer)"""
    c = case_settings(z, name)
    Wg = O.groups(case_weight(z, name), c['axis'], c['gs'])
    s, zz = O.minmax_qparams(Wg, c['sym'], c['round_zp'], c['qmin'], c['qmax'])
    q = z[name + '/qhqq']
    if q.size:
        r0 = O.solve(Wg, s, zz, c['qmin'], c['qmax'], float(q[0]), float(q[1]), int(q[3]))
        s, zz = r0['scales'], r0['zeros']
    return O.solve(Wg, s, zz, c['qmin'], c['qmax'], c['lp_norm'], c['beta'], c['iters'], stop_at=stop_at), Wg, (s, zz)


def _shipped():
    return json.loads(str(_gold()['shipped_quant']))


class _Model:
    def __init__(self, block):
        self.block = block

    def get_blocks(self):
        return [self.block]

    def get_block_linears(self, block):
        return {'fc': block[0]}


def _hqq(quant):
    from llmc_amd.compression.quantization import HQQ
    block = torch.nn.Sequential(torch.nn.Linear(256, 128, bias=False))
    return HQQ(_Model(block), quant, None, None, {})


# ---- configuration -------------------------------------------------------------------------------------------------------
def test_shipped_config_constructs_data_free():
    quant = _shipped()
    assert quant['method'] == 'HQQ'
    h = _hqq(quant)
    assert h.data_free and h.w_only
    assert (h.axis, h.lp_norm, h.beta, h.kappa, h.iters) == (0, 0.7, 10, 1.01, 20)
    wq = h.wquantizer
    assert (wq.bit, wq.sym, wq.granularity, wq.group_size, wq.round_zp) == (4, False, 'per_group', 128, False)


@pytest.mark.parametrize('key', ['lp_norm', 'beta', 'kappa', 'iters', 'axis'])
def test_special_keys_required(key):
    quant = _shipped()
    del quant['special'][key]
    with pytest.raises(KeyError):
        _hqq(quant)


def test_quantizer_hqq_defaults():
    from llmc_amd.compression.quantization import IntegerQuantizer
    q = IntegerQuantizer(4, False, 'per_group', group_size=128, calib_algo='hqq')
    assert (q.lp_norm, q.beta, q.kappa, q.iters) == (0.7, 10, 1.01, 20)


def test_float_quantizer_refuses_hqq():
    from llmc_amd.compression.quantization import FloatQuantizer
    with pytest.raises(NotImplementedError, match='hqq'):
        FloatQuantizer('e4m3', True, 'per_channel', calib_algo='hqq', use_qtorch=True)


def test_hqq_refuses_per_channel():
    quant = _shipped()
    quant['weight'] = dict(bit=4, symmetric=False, granularity='per_channel')
    with pytest.raises(NotImplementedError, match='per_group'):
        _hqq(quant)


def _wq_hqq():
    return dict(bit=4, symmetric=False, granularity='per_group', group_size=128, calib_algo='hqq')


def test_gptq_refuses_hqq():
    from llmc_amd.compression.quantization import GPTQ
    g = GPTQ.__new__(GPTQ)
    g.quant_config = {'special': {}, 'weight': _wq_hqq()}
    from llmc_amd.compression.quantization import IntegerQuantizer
    g.wquantizer = IntegerQuantizer(4, False, 'per_group', group_size=128, calib_algo='hqq')
    with pytest.raises(NotImplementedError, match='hqq'):
        g.add_quant_config()


def test_spqr_refuses_hqq():
    from llmc_amd.compression.quantization import IntegerQuantizer, SpQR
    s = SpQR.__new__(SpQR)
    s.quant_config = {'special': {}}
    s.wquantizer = IntegerQuantizer(4, False, 'per_group', group_size=128, calib_algo='hqq')
    with pytest.raises(NotImplementedError, match='hqq'):
        s.add_quant_config()


def test_awq_refuses_hqq():
    from llmc_amd.compression.quantization import Awq
    block = torch.nn.Sequential(torch.nn.Linear(256, 128, bias=False))
    with pytest.raises(NotImplementedError, match='hqq'):
        Awq(_Model(block), {'weight': _wq_hqq(), 'special': {}}, None, None, {})


def test_autoclipper_refuses_hqq():
    from llmc_amd.compression.quantization import AutoClipper, IntegerQuantizer
    wq = IntegerQuantizer(4, False, 'per_group', group_size=128, calib_algo='hqq')
    with pytest.raises(NotImplementedError, match='hqq'):
        AutoClipper(True, wq, None, 'v1', False, False, None)


# ---- the solver's scalars and sum order ------------------------------------------------------------------------------------
def test_shrink_scalars_match_torch():
    """c and p1 as ATen uses them: (1.0 / beta) * pow(...) and pow(x, lp_norm - 1) with Python scalars on fp32 tensors"""
    c, p1 = O.shrink_consts(0.7, 10)
    assert c == f32(0.1) and p1 == f32(0.7 - 1)
    x = torch.tensor([0.5, 1.7, 3.0, 1e-3], dtype=torch.float32)
    assert torch.equal((1.0 / 10) * x, torch.tensor(c) * x)
    # pow with a Python exponent uses the fp32 exponent: fp64 pow with it, rounded, agrees far more often
    xs = torch.rand(200000, generator=torch.Generator().manual_seed(1)) * 4 + 1e-3
    t = torch.pow(xs, 0.7 - 1).numpy()
    a32 = (xs.double().numpy() ** float(p1)).astype(f32)
    a64 = (xs.double().numpy() ** (0.7 - 1)).astype(f32)
    assert (a32 == t).mean() > 0.95 > (a64 == t).mean()


@pytest.mark.parametrize('g', [16, 32, 64, 128])
def test_inner_sum_fp32_matches_torch(g):
    gen = torch.Generator().manual_seed(g)
    x = torch.randn(4096, g, generator=gen) * torch.exp(4 * torch.randn(4096, 1, generator=gen))
    x[::7, ::3] = 0.0
    x[::11] = -0.0
    want = torch.sum(x, dim=-1).numpy()
    got = O.inner_sum_fp32(x.numpy())
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and the mean the solver takes
    assert np.array_equal((got / f32(g)).astype(f32), torch.mean(x, dim=-1).numpy())


def test_pow_f64_accuracy():
    x = np.concatenate([np.linspace(1e-6, 50, 100001), [1e-30, 3e20]]).astype(f32).astype(np.float64)
    for p in (float(f32(-0.3)), float(f32(-0.5)), float(f32(0.25))):
        got = O.pow_f64(x, p)
        assert np.max(np.abs(got / x ** p - 1)) < 1e-13
    assert O.pow_f64(np.zeros(1), -0.3)[0] == np.inf


# ---- the oracle against the reference --------------------------------------------------------------------------------------
def _names():
    return [str(n) for n in _gold()['names']]


@pytest.mark.parametrize('name', _names())
def test_oracle_matches_reference(name):
    z = _gold()
    c = case_settings(z, name)
    r, Wg, (s_start, z_start) = oracle_case(z, name)
    # the start: min / max qparams (and the quantizer's own solve for the double case)
    np.testing.assert_array_equal(O.minmax_qparams(Wg, c['sym'], c['round_zp'], c['qmin'], c['qmax'])[0], z[name + '/s_mm'])
    np.testing.assert_array_equal(s_start, z[name + '/s_start'])
    ref_errs = z[name + '/errs'].astype(f32)
    T = int(z[name + '/T'])
    # the stop iteration, and each logged fp32 error within 2 ulps (the reference's multi-threaded fp32 mean)
    assert r['T'] == T, (r['T'], T, r['errs32'], ref_errs)
    n = min(len(ref_errs), len(r['errs32']))
    ulps = np.abs(r['errs32'][:n].view(np.int32).astype(np.int64) - ref_errs[:n].view(np.int32).astype(np.int64))
    assert ulps.max() <= 2, ulps
    np.testing.assert_array_equal(r['scales'], z[name + '/scales'])
    zs_ref = z[name + '/zeros']
    if c['lp_norm'] == 1 or c['beta'] <= 0:
        np.testing.assert_array_equal(r['zeros'], zs_ref)
        return
    # pow: the reference's Sleef fp32 pow against the kernel's fp64 pow rounded once. Where the shrink never acts the
    # zeros agree bit for bit; where it acts, a few groups may differ in the last bits of z
    # zeros agree bit for bit; where it acts (sigma >= 0.5), observed: <= 0.4 % of groups, by <= 1e-6, no code changed
    diff = r['zeros'] != zs_ref
    if z[name + '/meta'][-1] <= 0.02:
        assert not diff.any()
    assert diff.mean() <= 0.005, diff.mean()
    assert np.max(np.abs(r['zeros'] - zs_ref), initial=0) <= 2e-6


def test_stop_cases_stop():
    z = _gold()
    for name in ('brk_ax0_i100', 'brk_ax1_i100', 'grid_tie_ax1'):
        assert int(z[name + '/stopped']) == 1
        assert int(z[name + '/T']) < int(case_settings(z, name)['iters']) - 1
    assert int(z['grid_tie_ax1/T']) == 1


@pytest.mark.skipif(not os.path.exists(REF_HQQ), reason='oracle/_ref (the reference build) is absent')
def test_surface_matches_reference():
    """HQQ's methods and their argument names against the reference class"""
    from llmc_amd.compression.quantization import hqq as ours
    tree = ast.parse(open(REF_HQQ).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'HQQ')
    for fn in cls.body:
        if isinstance(fn, ast.FunctionDef):
            mine = getattr(ours.HQQ, fn.name)
            want = [a.arg for a in fn.args.args]
            got = list(inspect.signature(mine).parameters)        # through torch.no_grad's wrapper
            assert got == want, (fn.name, got, want)
