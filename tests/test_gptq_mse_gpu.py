"""GPTQ with calib_algo 'mse' and dynamic groups (llmc_gptq_quantize_mse, llmc_mse_qparams_panel) on MI355X.

1. The strided panel search gives, bit for bit, what llmc_mse_qparams gives on a contiguous copy of each group.
2. At model shapes the loop equals the C oracle run in static mode with the GPU's qparams, and those qparams are the
   search of the oracle's block-start panels: the GPU searched each panel and then ran the reference loop.
3. Against the reference's own GPTQ (tests/golden/gptq_mse.npz, tools/make_golden_gptq_mse.py): the searched range is a
   discrete choice decided by fp32 sums of |q - x|^2.4, so a row may leave the reference at a near-tie; everything before
   a row's first differing group is bit-identical, and >= 97 % of the (row, group) pairs lie there.
4. The class path on a small Llama: build, quantize, deploy; row-sharded quantize_stacked keeps the bits.
"""
import copy

import numpy as np
import pytest
import torch

from conftest import load_golden
from llmc_amd import _ffi
from oracle import gptq_ref as G
from oracle import quant_ref as Q

pytestmark = pytest.mark.gpu
TD = {'f16': torch.float16, 'bf16': torch.bfloat16, 'torch.float16': torch.float16, 'torch.bfloat16': torch.bfloat16,
      'torch.float32': torch.float32}


class Cfg(dict):
    __getattr__ = dict.get


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def host(t):
    return t.detach().float().cpu().numpy()


def mse_args(maxshrink=0.8, grid=100):
    return int(maxshrink * grid), int(grid), 2.4


def mse_contig(x, sym, round_zp, qmin, qmax, nsteps=80, grid=100, norm=2.4):
    """llmc_mse_qparams on a contiguous fp32 [G, g] tensor -> (scales, zeros) fp32 [G]"""
    L = _ffi.lib()
    x = x.contiguous()
    s = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    z = torch.empty_like(s)
    _ffi.check(L.llmc_mse_qparams(_ffi.ptr(x), _ffi.dt(x), x.shape[0], x.shape[1], int(sym), int(round_zp), float(qmin),
                                  float(qmax), nsteps, grid, float(norm), _ffi.ptr(s), _ffi.ptr(z), None, None,
                                  _ffi.stream()), 'llmc_mse_qparams')
    return s, z


def mse_panel(W, c0, width, gs, sym, round_zp, qmin, qmax, scales, zeros, g0, nsteps=80, grid=100, norm=2.4):
    L = _ffi.lib()
    R, K = W.shape
    return L.llmc_mse_qparams_panel(_ffi.ptr(W), R, K, c0, width, gs, int(sym), int(round_zp), float(qmin), float(qmax),
                                    nsteps, grid, float(norm), _ffi.ptr(scales), _ffi.ptr(zeros), scales.shape[1], g0,
                                    _ffi.stream())


# =========================================================================================================================
# 1. panel search == llmc_mse_qparams on a contiguous copy
PANEL_SHAPES = [(4096, 4096), (6144, 4096), (28672, 4096), (4096, 14336)]
# (gs, bit, sym, round_zp, ragged tail)
PANEL_SETTINGS = [(128, 4, False, True, 0), (64, 3, False, False, 0), (32, 2, True, True, 4), (16, 8, False, True, 0),
                  (128, 4, True, True, 10), (16, 4, False, False, 0), (64, 8, True, False, 0), (32, 4, False, True, 0)]


@pytest.mark.parametrize('shape', PANEL_SHAPES)
def test_panel_search_equals_contiguous_search(shape):
    R, K = shape
    gen = torch.Generator(device='cuda').manual_seed(R + K)
    W = torch.randn(R, K, generator=gen, device='cuda') * 0.02
    checked = 0
    for si, (gs, bit, sym, round_zp, tail) in enumerate(PANEL_SETTINGS):
        qmin, qmax = Q.int_range(bit, sym)
        # first, a middle and the last block; a ragged width leaves a short last group
        c0 = [0, (K // 256) * 128, K - 128][si % 3]
        width = 128 - tail
        nb = -(-width // gs)
        # planted groups in rows of the panel: constant, all zero, one outlier, negative only
        Wc = W.clone()
        Wc[0, c0:c0 + gs] = 0.0173
        Wc[1, c0:c0 + gs] = 0.0
        Wc[2, c0 + 3] = 4.5
        Wc[3, c0:c0 + gs] = -Wc[3, c0:c0 + gs].abs() - 0.001
        ng = nb + 2
        s = torch.full((R, ng), float('nan'), device='cuda')
        z = torch.full((R, ng), float('nan'), device='cuda')
        _ffi.check(mse_panel(Wc, c0, width, gs, sym, round_zp, qmin, qmax, s, z, 1), 'llmc_mse_qparams_panel')
        sh, zh = host(s), host(z)
        assert np.isnan(sh[:, 0]).all() and np.isnan(sh[:, nb + 1]).all()      # only groups g0 .. g0 + nb - 1 written
        for j in range(nb):
            a, b = c0 + j * gs, c0 + min((j + 1) * gs, width)
            rs, rz = mse_contig(Wc[:, a:b], sym, round_zp, qmin, qmax)
            tag = f'{R}x{K} c0={c0} w={width} g{gs} b{bit} sym={sym} rzp={round_zp} group {j}'
            np.testing.assert_array_equal(bits(sh[:, 1 + j]), bits(host(rs)), err_msg=tag + ' scales')
            np.testing.assert_array_equal(bits(zh[:, 1 + j]), bits(host(rz)), err_msg=tag + ' zeros')
            checked += 1
    assert checked >= len(PANEL_SETTINGS)


def test_panel_search_refuses_other_group_sizes():
    W = torch.zeros(8, 256, device='cuda')
    s = torch.zeros(8, 4, device='cuda')
    assert mse_panel(W, 0, 96, 96, False, True, 0.0, 15.0, s, s.clone(), 0) == -95      # LLMC_ENOTSUP
    L = _ffi.lib()
    ws = _ffi.workspace(L.llmc_gptq_quantize_mse_ws_bytes(8, 256), W.device)
    U = torch.eye(256, device='cuda')
    rc = L.llmc_gptq_quantize_mse(_ffi.ptr(W), _ffi.ptr(U), 8, 256, 256, 0, 0.0, 15.0, 96, 1, 80, 100, 2.4, _ffi.ptr(s),
                                  _ffi.ptr(s), _ffi.ptr(W.clone()), None, 128, _ffi.ptr(ws), _ffi.stream())
    assert rc == -95


# =========================================================================================================================
# 2. model shapes against the C oracle
def _prep(R, K, seed):
    from llmc_amd.compression.quantization import gptq_pipeline as P
    gen = torch.Generator(device='cuda').manual_seed(seed)
    W = (torch.randn(R, K, generator=gen, device='cuda') * 0.02).to(torch.bfloat16)
    X = torch.randn(K + 512, K, generator=gen, device='cuda') * torch.exp(0.5 * torch.randn(K, generator=gen, device='cuda'))
    H = (X.T @ X) / X.shape[0]
    del X
    perm = torch.argsort(torch.diagonal(H), descending=True)
    U, Wp, info = P._prep_and_factor(H, W, perm, 0.01, None)
    assert int(info.item()) == 0
    return Wp, U.clone()


@pytest.mark.parametrize('R,K,gs,nrows', [(6144, 4096, 128, 128), (28672, 4096, 128, 96), (4096, 14336, 128, 12),
                                          (6144, 4096, 32, 96)])
def test_model_shapes_match_oracle_exactly(R, K, gs, nrows):
    from llmc_amd.compression.quantization.gptq_ops import gptq_quantize
    bit, sym = 4, False
    qmin, qmax = Q.int_range(bit, sym)
    Wp, U = _prep(R, K, R + K + gs)
    W_in = Wp.clone()
    tmp, losses, s, z = gptq_quantize(Wp, U, sym, qmin, qmax, gs, mse=(True,) + mse_args())
    if R == 6144 and gs == 128:
        # helper streams off: the same bits
        W2 = W_in.clone()
        with _ffi.helper_streams(False):
            t2, l2, s2, z2 = gptq_quantize(W2, U, sym, qmin, qmax, gs, mse=(True,) + mse_args())
        assert torch.equal(t2.view(torch.int32), tmp.view(torch.int32)) and torch.equal(s2.view(torch.int32), s.view(torch.int32))
        assert torch.equal(l2.view(torch.int32), losses.view(torch.int32)) and torch.equal(z2, z)
        del W2, t2, l2
    rows = np.sort(np.random.RandomState(K + gs).choice(R, nrows, replace=False))
    ri = torch.from_numpy(rows).cuda()
    col_group = (np.arange(K) // gs).astype(np.int32)
    Uh = host(U)
    ref = G.weight_transform(host(W_in[ri]), Uh, sym, qmin, qmax, gs, True, col_group, host(s[ri]), host(z[ri]))
    # (a) the reference loop with the GPU's qparams reproduces the GPU's loop
    np.testing.assert_array_equal(bits(host(tmp[ri])), bits(ref['tmp']))
    np.testing.assert_array_equal(bits(host(losses[ri])), bits(ref['losses']))
    # (b) those qparams are the search of the block-start panels (the oracle's running W keeps them in visited columns)
    Wrun = torch.from_numpy(ref['W']).cuda()
    for j in range(K // gs):
        rs, rz = mse_contig(Wrun[:, j * gs:(j + 1) * gs], sym, True, qmin, qmax)
        np.testing.assert_array_equal(bits(host(rs)), bits(host(s[ri, j])), err_msg=f'group {j} scales')
        np.testing.assert_array_equal(bits(host(rz)), bits(host(z[ri, j])), err_msg=f'group {j} zeros')


# =========================================================================================================================
# 3. the reference's GPTQ (golden)
def synth_upper(K, seed):
    """tools/make_golden_gptq_mse.py:synth_upper — the upper factor the golden's reference loop ran with"""
    i = np.arange(K, dtype=np.int64)[:, None]
    j = np.arange(K, dtype=np.int64)[None, :]
    h = (i * 2654435761 + j * 40503 + seed * 7919) % 65521
    off = ((h % 257) - 128).astype(np.float32) / np.float32(4096.0)
    diag = np.float32(0.5) + (i % 61).astype(np.float32) / np.float32(64.0)
    return np.where(j > i, off, np.where(j == i, diag, np.float32(0.0))).astype(np.float32)


def from_bits16(b, dt):
    return torch.from_numpy(b.view(np.int16).copy()).view(TD[dt])


def _gptq_for(case, g):
    from llmc_amd.compression.quantization import IntegerQuantizer
    from llmc_amd.compression.quantization.gptq import GPTQ
    from llmc_amd.compression.quantization.gptq_pipeline import GptqConfig
    p = case + '/'
    bit, sym, gs, actorder, _, R, K, qmin, qmax, n_out, maxshrink, grid, b_num, round_zp = g[p + 'meta']
    wq = IntegerQuantizer(int(bit), bool(sym), 'per_group', group_size=int(gs), calib_algo='mse', maxshrink=float(maxshrink),
                          mse_grid=int(grid), mse_b_num=int(b_num), round_zp=bool(round_zp))
    a = GPTQ.__new__(GPTQ)
    a.wquantizer, a.static_groups, a.actorder, a.blocksize, a.owq = wq, False, bool(actorder), 128, int(n_out) > 0
    a.n_nonout = int(K) - int(n_out)
    a.columns = int(K)
    a.qparams, a.groups = {}, []
    a.model_dtype = TD[str(g[p + 'dt'])]
    a.need_perm = bool(actorder) or a.owq
    a.gcfg = GptqConfig(bit=int(bit), symmetric=bool(sym), group_size=int(gs), actorder=bool(actorder),
                        mse=(bool(round_zp), int(float(maxshrink) * int(grid)), int(grid), 2.4))
    return a, wq, dict(bit=int(bit), sym=bool(sym), gs=int(gs), R=int(R), K=int(K), n_out=int(n_out), qmin=qmin, qmax=qmax,
                       round_zp=bool(round_zp), nsteps=int(float(maxshrink) * int(grid)), grid=int(grid))


def test_reference_golden_through_weight_transform():
    g = load_golden('gptq_mse')
    tot_pairs = agree_pairs = panel_same = panel_tot = 0
    fracs = {}
    for ci, case in enumerate(str(n) for n in g['names']):
        p = case + '/'
        a, wq, c = _gptq_for(case, g)
        R, K, gs, n_out = c['R'], c['K'], c['gs'], c['n_out']
        dt = str(g[p + 'dt'])
        seed, csum = g[p + 'U_seed']
        Uh = synth_upper(K, int(seed))
        assert int(Uh.view(np.uint32).astype(np.uint64).sum()) == int(csum), case
        W = from_bits16(g[p + 'Wp_bits'], dt).float().cuda()
        U = torch.from_numpy(Uh).cuda()
        perm = torch.from_numpy(g[p + 'perm']).cuda()
        if perm.numel():
            a.perm = perm
        Losses, tmp = torch.zeros_like(W), torch.zeros_like(W)
        a.weight_transform(W, U, Losses, tmp)
        nq = K - n_out
        ngv = -(-nq // gs)
        s = torch.cat([gr['scale'].reshape(R, 1) for gr in a.groups[:ngv]], 1)
        sh = host(s)
        diff = bits(sh) != bits(g[p + 'g_scales'][:, :ngv])
        if not c['sym']:
            z = torch.cat([gr['zero'].reshape(R, 1) for gr in a.groups[:ngv]], 1)
            diff |= host(z) != g[p + 'g_zeros'][:, :ngv]
        first = np.where(diff.any(1), diff.argmax(1), ngv)          # first differing group of each row
        th, lh = host(tmp), host(Losses)
        for r in range(R):
            cend = min(int(first[r]) * gs, nq)
            np.testing.assert_array_equal(bits(th[r, :cend]), bits(g[p + 'tmp'][r, :cend]), err_msg=f'{case} row {r} tmp')
            np.testing.assert_array_equal(bits(lh[r, :cend]), bits(g[p + 'losses'][r, :cend]), err_msg=f'{case} row {r} losses')
        tot_pairs += R * ngv
        agree_pairs += int(first.sum())
        fracs[case] = float(first.sum()) / (R * ngv)
        full = first == ngv                                          # rows that never left the reference
        # the search on the reference's own block-start panels (its running W keeps them in the visited columns)
        Wa = torch.from_numpy(g[p + 'W_after']).cuda()
        for j in range(ngv):
            rs, rz = mse_contig(Wa[:, j * gs:min((j + 1) * gs, nq)], c['sym'], c['round_zp'], c['qmin'], c['qmax'],
                                c['nsteps'], c['grid'])
            panel_same += int((bits(host(rs)) == bits(g[p + 'g_scales'][:, j])).sum())
            panel_tot += R
        # finish the layer like update_layer_with_transformed_weights and deploy it
        t2 = tmp.clone()
        if perm.numel():
            t2[:, nq:] = W[:, nq:]
            t2 = t2[:, torch.argsort(perm)]
        layer = torch.nn.Linear(K, R, bias=False).cuda()
        layer.weight.data = t2
        layer.register_buffer('buf_qmax', torch.tensor(c['qmax']))
        layer.register_buffer('buf_qmin', torch.tensor(c['qmin']))
        layer.buf_zeros = torch.tensor(0.0)
        a.update_model_qparams(layer)
        if n_out:
            layer.register_buffer('buf_perm', perm)
            layer.register_buffer('buf_invperm', torch.argsort(perm))
            layer.register_buffer('buf_n_nonout', torch.tensor(nq))
        elif perm.numel():
            layer.register_buffer('buf_perm', perm)
            layer.register_buffer('buf_invperm', torch.argsort(perm))
        assert layer.buf_scales.dtype == torch.float32 and tuple(layer.buf_scales.shape) == (R * ngv, 1), case
        assert str(layer.buf_scales.dtype) == str(g[p + 'buf_scales_dtype'])
        bs = host(layer.buf_scales).reshape(R, ngv)
        np.testing.assert_array_equal(bits(bs[full]), bits(g[p + 'buf_scales'].reshape(R, ngv)[full]), err_msg=case)
        if not c['sym']:
            assert layer.buf_zeros.dtype == torch.float32 and tuple(layer.buf_zeros.shape) == (R * ngv, 1), case
            np.testing.assert_array_equal(host(layer.buf_zeros).reshape(R, ngv)[full],
                                          g[p + 'buf_zeros'].reshape(R, ngv)[full], err_msg=case)
        if g[p + 'final_w'].size:
            np.testing.assert_array_equal(bits(host(layer.weight)[full]), bits(g[p + 'final_w'][full]), err_msg=case)
        fq = a.w_qdq(layer, wq)
        assert fq.dtype == TD[str(g[p + 'w_qdq_dtype'])], case
        ref_fq = from_bits16(g[p + 'w_qdq_bits'], dt).float().numpy()
        np.testing.assert_array_equal(bits(host(fq)[full]), bits(ref_fq[full]), err_msg=case + ' w_qdq')
        if (p + 'w_q_codes') in g.files:
            codes, _, _ = a.w_q(layer, wq)
            # the fixture keeps the codes' low bytes (symmetric codes are negative)
            np.testing.assert_array_equal((codes.cpu().numpy().astype(np.int64) & 0xff).reshape(R, -1)[full],
                                          g[p + 'w_q_codes'].astype(np.int64).reshape(R, -1)[full], err_msg=case + ' w_q')
    frac = agree_pairs / tot_pairs
    print(f'\ngptq_mse golden: (row, group) pairs in the agreeing prefix {frac:.4f} ({agree_pairs}/{tot_pairs}); per case '
          + ', '.join(f'{k} {v:.3f}' for k, v in fracs.items()))
    print(f'search on the reference\'s block-start panels: same scales {panel_same / panel_tot:.4f}')
    assert frac >= 0.97, fracs
    assert panel_same / panel_tot >= 0.97


# =========================================================================================================================
# 4. the class path
def _llama_with_inputs(n=4, seq=128):
    import hf_adapters as H
    model = H.tiny_llama(torch.bfloat16)
    inp = model.collect_first_block_input(H.calib_ids(n, seq, 160))
    return model, inp


@pytest.mark.parametrize('actorder,fmt', [(True, 'fake_quant'), (False, 'vllm_quant')])
def test_gptq_mse_on_llama_blocks_builds_quantizes_and_deploys(actorder, fmt):
    import llmc_amd.compression.quantization as Qz
    model, inp = _llama_with_inputs()
    qc = Cfg(weight=Cfg(bit=4, symmetric=False, granularity='per_group', group_size=128, calib_algo='mse'),
             special=Cfg(actorder=actorder, static_groups=False, percdamp=0.01, blocksize=128, true_sequential=True),
             quant_out=True)
    config = Cfg(calib=Cfg(seq_len=128), model=Cfg(type='Llama'))
    algo = Qz.GPTQ(model, qc, copy.deepcopy(inp), None, config)
    assert algo.gcfg.mse == (True, 80, 100, 2.4)
    algo.run_block_loop()
    blk = model.get_blocks()[0]
    for n in ('self_attn.q_proj', 'self_attn.o_proj', 'mlp.gate_proj', 'mlp.down_proj'):
        m = blk.get_submodule(n)
        R, K = m.weight.shape
        assert m.weight.dtype == torch.float32 and torch.isfinite(m.weight).all(), n
        assert m.buf_scales.shape == (R * K // 128, 1) and m.buf_scales.dtype == torch.float32, n
        assert m.buf_zeros.shape == (R * K // 128, 1) and m.buf_zeros.dtype == torch.float32, n
    algo.deploy(fmt)
    if fmt == 'fake_quant':
        # the deployed model runs end to end on the GPU
        import hf_adapters as H
        model.model.cuda()
        ids = H.calib_ids(1, 64, 160, seed=5)[0].cuda()
        with torch.no_grad():
            logits = model.model(ids).logits
        assert torch.isfinite(logits).all()
    else:
        # the real-quant export packs codes from the searched qparams
        lin = model.get_blocks()[0].mlp.gate_proj
        packed = [b for n, b in lin.named_buffers() if b.dtype in (torch.int32, torch.uint8, torch.int8)]
        assert packed, [n for n, _ in lin.named_buffers()]


def test_row_sharded_stacked_quantize_keeps_the_bits():
    from llmc_amd.compression.quantization.gptq_pipeline import GptqConfig, quantize_stacked
    R1, R2, K = 384, 640, 512
    gen = torch.Generator(device='cuda').manual_seed(7)
    Ws = [(torch.randn(r, K, generator=gen, device='cuda') * 0.02).to(torch.bfloat16) for r in (R1, R2)]
    X = torch.randn(2048, K, generator=gen, device='cuda')
    H = X.T @ X / 2048
    cfg = GptqConfig(bit=4, symmetric=False, group_size=64, actorder=True, mse=(True, 80, 100, 2.4))
    whole = quantize_stacked(Ws, H.clone(), cfg)
    w_all = torch.cat([r.weight for r in whole])
    s_all = torch.cat([r.scales for r in whole])
    z_all = torch.cat([r.zeros for r in whole])
    for r0, r1 in ((0, 256), (256, 1024)):
        part = quantize_stacked(Ws, H.clone(), cfg, rows=(r0, r1))[0]
        assert torch.equal(part.weight.view(torch.int32), w_all[r0:r1].view(torch.int32))
        assert torch.equal(part.scales.view(torch.int32), s_all[r0:r1].view(torch.int32))
        assert torch.equal(part.zeros, z_all[r0:r1])
