"""HQQ's solver kernel (llmc_hqq_optimize) on the MI355X.

1. Every case of tests/golden/hqq.npz: scales, zeros and the stop iteration T bit for bit against the numpy oracle
   (tests/hqq_oracle.py, which test_hqq_config.py pins to the reference), per-iteration errors to 1e-12 relative.
2. A grid of bits x sym x round_zp x group size x axis x lp_norm x dtype against the oracle, bit for bit.
3. Llama-3-8B widths, both axes: per-iteration errors against a torch restatement over the whole tensor, T against the
   stop rule on those errors, a seeded sample of groups bit for bit against the oracle run to that T.
4. The class path: HQQ.run_block_loop + deploy('fake_quant') on the toy model and a small HF Llama; RTN with
   calib_algo hqq.
"""
import itertools

import numpy as np
import pytest
import torch

import hqq_oracle as O
from test_hqq_config import _gold, _names, case_settings, case_weight, oracle_case

pytestmark = pytest.mark.gpu
f32 = np.float32
TD = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}


class Cfg(dict):
    __getattr__ = dict.get


def quantizer(bit, sym, gs, round_zp, **kw):
    from llmc_amd.compression.quantization import IntegerQuantizer
    return IntegerQuantizer(bit, sym, 'per_group', group_size=gs, round_zp=round_zp, **kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def run_kernel(W, wq, axis, lp_norm, beta, iters, s=None, z=None):
    s_, z_, T, errs = wq.hqq_solve(W, axis=axis, scales=s, zeros=z, lp_norm=lp_norm, beta=beta, iters=iters)
    return (s_.reshape(-1).cpu().numpy(), z_.reshape(-1).cpu().numpy(), int(T.item()), errs.cpu().numpy())


def check_case(res, r):
    s, z, T, errs = res
    assert T == r['T'], (T, r['T'])
    assert np.array_equal(bits(s), bits(r['scales']))
    bad = bits(z) != bits(r['zeros'])
    assert not bad.any(), f'{bad.sum()} of {bad.size} zeros differ'
    n = T + 1
    np.testing.assert_allclose(errs[:n], r['errs'][:n], rtol=1e-12, atol=0)


# ---- 1. the golden cases -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', _names())
def test_golden_case_bit_exact(name):
    z = _gold()
    c = case_settings(z, name)
    W = torch.from_numpy(case_weight(z, name)).to(TD[str(z[name + '/dt'])]).cuda()
    r, Wg, _ = oracle_case(z, name)
    q = z[name + '/qhqq']
    wq = quantizer(c['bit'], c['sym'], c['gs'], c['round_zp'])
    s0 = z0 = None
    if q.size:       # the quantizer's own solve first (calib_algo hqq on the weight quantizer)
        wq1 = quantizer(c['bit'], c['sym'], c['gs'], c['round_zp'], calib_algo='hqq', lp_norm=float(q[0]),
                        beta=float(q[1]), kappa=float(q[2]), iters=int(q[3]))
        s0, z0, _, _ = wq1.hqq_solve(W, axis=c['axis'])
    res = run_kernel(W, wq, c['axis'], c['lp_norm'], c['beta'], c['iters'], s0, z0)
    check_case(res, r)
    assert res[2] == int(z[name + '/T'])          # and the reference's stop iteration
    # the min / max start is llmc_minmax_qparams' bits on the fp32 view
    _, s_mm, _, _, _ = wq.get_tensor_qparams((W.float().T if c['axis'] == 0 else W.float()).contiguous())
    np.testing.assert_array_equal(bits(s_mm.reshape(-1).cpu().numpy()), bits(z[name + '/s_mm']))


# ---- 2. the grid ----------------------------------------------------------------------------------------------------------
GRID = list(itertools.product([2, 3, 4, 8], [False, True], [False, True], [16, 32, 64, 128], [0, 1], [0.7, 1.0],
                              ['bf16', 'f16']))


def test_grid_bit_exact():
    gen = torch.Generator().manual_seed(7)
    fails = []
    for i, (bit, sym, rzp, gs, axis, lp, dt) in enumerate(GRID):
        R, K = (2 * gs, 128) if axis == 0 else (32, 2 * gs)
        sigma = 1.0 if i % 3 == 0 else 0.02            # every third case with the shrink active
        W = (torch.randn(R, K, generator=gen) * sigma).to(TD[dt])
        W[:, :1] = 0
        wq = quantizer(bit, sym, gs, rzp)
        res = run_kernel(W.cuda(), wq, axis, lp, 10, 20)
        Wg = O.groups(W.float().numpy(), axis, gs)
        s, z = O.minmax_qparams(Wg, sym, rzp, float(wq.qmin), float(wq.qmax))
        r = O.solve(Wg, s, z, float(wq.qmin), float(wq.qmax), lp, 10, 20)
        try:
            check_case(res, r)
        except AssertionError as e:
            fails.append(((bit, sym, rzp, gs, axis, lp, dt), str(e)[:200]))
    assert not fails, fails[:5]


def test_fp32_weight_strided_rows_and_given_qparams():
    """fp32 weights with a row stride > K, and a solve from given (s, z)"""
    gen = torch.Generator().manual_seed(3)
    big = (torch.randn(256, 640, generator=gen) * 0.3).cuda()
    W = big[:, :512]
    Wh = W.cpu().numpy()
    wq = quantizer(4, False, 128, False)
    for axis in (0, 1):
        Wg = O.groups(Wh, axis, 128)
        s, z = O.minmax_qparams(Wg, False, False, 0.0, 15.0)
        check_case(run_kernel(W, wq, axis, 0.7, 10, 20), O.solve(Wg, s, z, 0.0, 15.0, 0.7, 10, 20))
        s1, z1 = (s * f32(1.25)).astype(f32), (z + f32(0.5)).astype(f32)
        res = run_kernel(W, wq, axis, 0.7, 10, 5, torch.from_numpy(s1).cuda(), torch.from_numpy(z1).cuda())
        check_case(res, O.solve(Wg, s1, z1, 0.0, 15.0, 0.7, 10, 5))
    # iters 0: the min / max zeros and 1 / (1 / s)
    s, z, T, _ = run_kernel(W, wq, 1, 0.7, 10, 0)
    s0, z0 = O.minmax_qparams(O.groups(Wh, 1, 128), False, False, 0.0, 15.0)
    assert T == -1 and np.array_equal(z, z0) and np.array_equal(s, (f32(1) / (f32(1) / s0)).astype(f32))


# ---- 3. Llama-3-8B widths ---------------------------------------------------------------------------------------------------
def torch_error(W32g, s, z, qmin, qmax):
    """mean |W - W_r| of one iteration from (s, z), fp32 elementwise, fp64 sum (torch on the GPU)"""
    inv = 1.0 / s
    q = torch.round(W32g * inv + z).clamp(qmin, qmax)
    r = (q - z) / inv
    return (W32g - r).abs().double().sum().item() / W32g.numel()


WIDTHS = [(4096, 4096, 0, 20), (4096, 4096, 1, 20), (1024, 4096, 0, 20), (1024, 4096, 1, 20), (14336, 4096, 0, 20),
          (14336, 4096, 1, 20), (4096, 14336, 0, 20), (4096, 14336, 1, 20), (1024, 4096, 1, 100)]


@pytest.mark.parametrize('R,K,axis,iters', WIDTHS)
def test_llama_width(R, K, axis, iters):
    gen = torch.Generator(device='cuda').manual_seed(R + K + axis + iters)
    W = torch.randn(R, K, generator=gen, device='cuda') * 0.02
    m = torch.rand(R, K, generator=gen, device='cuda') < 1e-3
    W = torch.where(m, W * 20, W).to(torch.bfloat16)
    wq = quantizer(4, False, 128, False)
    s, z, T, errs = run_kernel(W, wq, axis, 0.7, 10, iters)
    assert T == O.reference_T(errs[:T + 1].astype(f32))
    if iters == 100:
        assert T < iters - 1, 'expected a stop'
    W32g = (W.float().T if axis == 0 else W.float()).contiguous().reshape(-1, 128)
    qmin, qmax = 0.0, 15.0
    for i in range(T + 1):
        # (s, z) entering iteration i: the solver run for i iterations (no stop can come before T). Its scales are
        # 1 / (1 / s), whose inverse is the same inv
        si, zi, Ti, _ = wq.hqq_solve(W, axis=axis, lp_norm=0.7, beta=10, iters=i)
        assert int(Ti.item()) == i - 1
        np.testing.assert_allclose(errs[i], torch_error(W32g, si, zi, qmin, qmax), rtol=1e-12)
    # a seeded sample of groups bit for bit against the oracle run to T
    G = W32g.shape[0]
    idx = np.sort(np.random.default_rng(R * 7 + K + axis).choice(G, 2048, replace=False))
    Wg = W32g[torch.from_numpy(idx).cuda()].cpu().numpy()
    s0, z0 = O.minmax_qparams(Wg, False, False, qmin, qmax)
    r = O.solve(Wg, s0, z0, qmin, qmax, 0.7, 10, iters, stop_at=T)
    assert np.array_equal(bits(s[idx]), bits(r['scales']))
    bad = bits(z[idx]) != bits(r['zeros'])
    print(f'{R}x{K} axis {axis}: T={T}, sampled groups differing {bad.sum()}, flagged {r["flagged"].sum()}')
    assert not (bad & ~r['flagged']).any()


# ---- 4. the class path ------------------------------------------------------------------------------------------------------
def _hqq_cfg(axis=0, qkw=None):
    w = Cfg(bit=4, symmetric=False, granularity='per_group', group_size=128, round_zp=False, **(qkw or {}))
    return Cfg(method='HQQ', weight=w, special=Cfg(axis=axis, lp_norm=0.7, beta=10, kappa=1.01, iters=20))


def _run(model, axis, qkw=None):
    from llmc_amd.compression.quantization import HQQ
    algo = HQQ(model, _hqq_cfg(axis, qkw), None, None, Cfg())
    algo.run_block_loop()
    before = {}
    for bi, blk in enumerate(model.get_blocks()):
        for n, m in model.get_block_linears(blk).items():
            R, K = m.weight.shape
            assert m.buf_scales.shape == (R * K // 128, 1) and m.buf_scales.dtype == torch.float32
            assert m.buf_zeros.shape == (R * K // 128, 1) and m.buf_zeros.dtype == torch.float32
            before[(bi, n)] = (m.weight.data.clone(), m.buf_scales.clone(), m.buf_zeros.clone(), m.buf_qmax.clone(),
                               m.buf_qmin.clone())
    algo.deploy('fake_quant')
    return algo, before


def _check_deployed(model, algo, before):
    """each deployed Linear computes with fake_quant_weight_static of the registered buffers (what w_qdq returns)"""
    n = 0
    for (bi, name), (w0, sc, zr, qmax, qmin) in before.items():
        m = model.get_blocks()[bi].get_submodule(name)
        args = {'scales': sc.cuda(), 'zeros': zr.cuda(), 'qmax': qmax.cuda(), 'qmin': qmin.cuda()}
        if algo.axis == 0:
            args['dim'] = 'ic'
        want = algo.wquantizer.fake_quant_weight_static(w0.cuda(), args)
        got = m.weight.data.cuda()
        assert got.shape == want.shape and torch.equal(got, want), name
        n += 1
    assert n > 0


@pytest.mark.parametrize('axis', [0, 1])
def test_toy_model_block_loop_and_deploy(axis):
    from toy_model import ToyModel
    model = ToyModel(hidden=256, inner=384, n_blocks=2)
    algo, before = _run(model, axis)
    _check_deployed(model, algo, before)
    for (bi, name), (w0, sc, zr, _, _) in list(before.items())[:2]:
        s, z, _, _ = algo.wquantizer.hqq_solve(w0.cuda(), axis=axis, lp_norm=0.7, beta=10, iters=20)
        assert torch.equal(s.cpu(), sc.cpu()) and torch.equal(z.cpu(), zr.cpu())


def test_hf_llama_block_loop_and_deploy():
    import hf_adapters as H
    model = H.tiny_llama(torch.bfloat16)
    algo, before = _run(model, 0, dict(calib_algo='hqq', iters=3))
    _check_deployed(model, algo, before)
    model.model.cuda()
    ids = H.calib_ids(1, 64, 160, seed=5)[0].cuda()
    with torch.no_grad():
        assert torch.isfinite(model.model(ids).logits).all()


def test_rtn_with_calib_algo_hqq():
    from llmc_amd.compression.quantization import RTN
    from toy_model import ToyModel
    model = ToyModel(hidden=256, inner=384, n_blocks=1)
    name, m = next(iter(model.get_block_linears(model.get_blocks()[0]).items()))
    w0 = m.weight.data.clone().cuda()
    qc = Cfg(weight=Cfg(bit=4, symmetric=False, granularity='per_group', group_size=128, calib_algo='hqq'), special=Cfg())
    algo = RTN(model, qc, None, None, Cfg())
    wq = algo.wquantizer
    fq = wq.fake_quant_weight_dynamic(w0)
    s, z, _, _ = wq.hqq_solve(w0, axis=1)
    want = wq.quant_dequant(w0.float().reshape(-1, 128), s, z, wq.qmax.cuda(), wq.qmin.cuda()).reshape(w0.shape)
    assert fq.dtype == w0.dtype and torch.equal(fq, want.to(w0.dtype))
    codes, cs, cz = wq.real_quant_weight_dynamic(w0)
    assert codes.dtype == torch.int32 and cs.shape == (w0.shape[0], w0.shape[1] // 128)
    assert torch.equal(cs.reshape(-1, 1), s)
    algo.run_block_loop()
    algo.deploy('fake_quant')
