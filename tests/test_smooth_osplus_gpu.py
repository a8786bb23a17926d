"""SmoothQuant and OsPlus on the GPU: the new kernels (csrc/smooth_osplus.hip) bit for bit against the reference's CPU results
(tests/golden/smooth_osplus.npz, tools/make_golden_smooth_osplus.py) and against the parent kernels they fuse, the threshold
search's loss curve and winner, and both algorithms end to end through run_block_loop -> deploy."""
import copy

import numpy as np
import pytest
import torch

import smooth_osplus_cases as C

pytestmark = pytest.mark.gpu

DT = C.DT
# units in the last place of the loss dtype: the loss takes two roundings in it (`sum(-1)`, `mean()`)
ULP = {'bf16': 2.0 ** -7, 'f16': 2.0 ** -10, 'f32': 2.0 ** -23}
# Largest relative deviation of a grid point's loss between the reference run on an MI355X (oracle/_ref/plain through
# PyTorch-ROCm) and its own CPU golden, per loss dtype: profiles/osplus_parity.txt (tools/osplus_parity.py), arm ref_gpu.
# Our curve is allowed twice that against the golden — the spread is a single sample.
REF_SELF_SPREAD = {'bf16': 7.6336e-03, 'f16': 2.7273e-03, 'f32': 5.8232e-06}


class Cfg(dict):
    __getattr__ = dict.get


def eq_bits(t, want_bits):
    return np.array_equal(C.bits_of(t).reshape(-1), want_bits.reshape(-1))


# ---- column statistics ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['bf16', 'f16', 'f32'])
@pytest.mark.parametrize('N,K', [(512, 4096), (37, 120), (5, 1001), (1, 8), (3000, 264), (70000, 24)])
def test_col_stats_bit_exact(dt, N, K):
    from llmc_amd.compression.quantization import smooth_ops
    g = torch.Generator().manual_seed(N * 7 + K)
    x = (torch.randn(N, K, generator=g) * torch.exp(torch.randn(K, generator=g))).to(DT[dt]).cuda()
    x[0] = 0.0
    st = smooth_ops.col_stats(x)
    xf = x.float()
    assert torch.equal(st.max, xf.amax(0)) and torch.equal(st.min, xf.amin(0)) and torch.equal(st.absmax, xf.abs().amax(0))
    assert float(st.glob[0]) == max(float(xf.max()), 0.0) and float(st.glob[1]) == min(float(xf.min()), 0.0)
    # batches accumulate; an unaligned view takes the scalar form
    y = (torch.randn(N + 3, K, generator=g) * 3).to(DT[dt]).cuda()
    st.update(y)
    both = torch.cat([xf, y.float()])
    assert torch.equal(st.max, both.amax(0)) and torch.equal(st.min, both.amin(0)) and torch.equal(st.absmax, both.abs().amax(0))
    if K > 1:
        v = x.reshape(-1)[1:1 + (N - 1) * K].reshape(N - 1, K) if N > 1 else None
        if v is not None:
            assert v.data_ptr() % 16 != 0
            sv = smooth_ops.col_stats(v)
            assert torch.equal(sv.max, v.float().amax(0)) and torch.equal(sv.min, v.float().amin(0))


def test_col_stats_positive_only_and_nan():
    from llmc_amd.compression.quantization import smooth_ops
    x = torch.rand(64, 256).add_(1.0).to(torch.bfloat16).cuda()
    st = smooth_ops.col_stats(x)
    assert float(st.glob[1]) == 0.0 and float(st.glob[0]) == float(x.float().max())       # amn clamps against 0
    x[5, 9] = float('nan')
    st = smooth_ops.col_stats(x)
    assert torch.isnan(st.max[9]) and torch.isnan(st.min[9]) and torch.isnan(st.absmax[9]) and torch.isnan(st.glob[0])
    assert int(torch.isnan(st.max).sum()) == 1                                          # like torch.amax: only that column


# ---- SmoothQuant scales against the reference -------------------------------------------------------------------------------
def _sq(alpha):
    import llmc_amd.compression.quantization as Q
    from toy_model import ToyModel
    qc = {'method': 'SmoothQuant', 'weight': dict(bit=8, symmetric=True, granularity='per_channel'),
          'act': dict(bit=8, symmetric=True, granularity='per_token'), 'special': {'alpha': alpha}}
    return Q.SmoothQuant(ToyModel(), qc, None, None, {})


@pytest.mark.parametrize('name', [str(n) for n in C.gold()['sq_names']])
def test_smoothquant_scales_match_the_reference_bit_for_bit(name):
    """w_max, x_max and the returned scale against the reference's CPU run, bit for bit. An exponent other than 0.5 goes through
    ATen's vectorised CPU pow, which is not correctly rounded in fp32; the kernel restates that routine (csrc/vec_powf.h)."""
    z = C.gold()
    dt = str(z[name + '/dt'])
    K = int(z[name + '/x_shape'][2])
    fcs = []
    for i in range(2):
        w = C.from_bits(z[name + f'/w{i}_bits'], dt)
        fc = torch.nn.Linear(K, w.shape[0], bias=False).to(DT[dt])
        fc.weight.data = w
        fcs.append(fc.cuda())
    xs = [C.from_bits(z[name + f'/x{i}_bits'], dt).reshape(tuple(int(v) for v in z[name + '/x_shape'])).cuda()
          for i in range(int(z[name + '/n_batches']))]
    sq = _sq(float(z[name + '/alpha']))
    w_max = sq.get_weight_scale(fcs)
    assert w_max.dtype == DT[dt] and eq_bits(w_max, z[name + '/w_max'])
    x_max = sq.get_act_scale(xs)
    assert x_max.dtype == torch.float32 and np.array_equal(x_max.cpu().numpy(), z[name + '/x_max'])
    scale = sq.search_scale_subset(fcs, xs)
    got, want = C.bits_of(scale), z[name + '/scale'].reshape(-1)
    print(f'{name}: {int((got != want).sum())} of {want.size} scales differ')
    assert scale.dtype == DT[dt] and np.array_equal(got, want)


@pytest.mark.parametrize('alpha', [0.75, 0.25, 0.3, 0.8])
def test_smooth_scales_pow_is_the_vectorised_cpu_pow(alpha):
    """x^alpha through llmc_smooth_scales (w_max = 1, so the quotient and the clamp change nothing) against torch.pow on an fp32
    CPU tensor. 32768 elements: one chunk of ATen's parallel loop and a whole number of vectors, so every element takes the
    vectorised routine. The fp64 power rounded once differs from it on 2 % (0.75) to 60 % (0.3) of these inputs."""
    from llmc_amd.compression.quantization import smooth_ops
    g = torch.Generator().manual_seed(int(alpha * 100))
    x = torch.cat([torch.rand(16384, generator=g) * 200 + 1e-3, torch.exp(torch.randn(16384, generator=g) * 6)])
    want = torch.pow(x, alpha).clamp(min=1e-5)
    got = smooth_ops.smooth_scales(x.cuda(), torch.ones_like(x).cuda(), alpha, torch.float32).cpu()
    # smooth_scales raises w_max to 1 - alpha: 1^y is exactly 1 in the routine (log 1 = 0, exp 0 = 1)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), int((got != want).sum())
    assert int((want != (x.double() ** alpha).float().clamp(min=1e-5)).sum()) > 100


# ---- OS+ against the reference ----------------------------------------------------------------------------------------------
def _osplus(cfg, mod):
    import llmc_amd.compression.quantization as Q
    return Q.OsPlus(C.OneBlockModel(mod, cfg['has_bias']), C.quant_section(cfg), None, None, {})


OS_NAMES = [str(n) for n in C.gold()['os_names']]


@pytest.mark.parametrize('name', OS_NAMES)
def test_osplus_pieces_match_the_reference_bit_for_bit(name):
    """statistics, shift, cur_scale at the stored grid points, the scaled fake-quantized weight and q_x at the stored point"""
    from llmc_amd.compression.quantization import smooth_ops
    z = C.gold()
    cfg, dt, mod, x = C.os_case(z, name)
    mod, x = mod.cuda(), x.cuda()
    algo = _osplus(cfg, mod)
    if cfg['has_bias']:
        st = smooth_ops.col_stats(x)
        shift = (st.max.to(x.dtype) + st.min.to(x.dtype)) / 2
        assert eq_bits(shift, z[name + '/shift'])
        xs = x - shift
    else:
        xs = x
    st = smooth_ops.col_stats(xs)
    assert eq_bits(st.max.to(x.dtype), z[name + '/cmx']) and eq_bits(st.min.to(x.dtype), z[name + '/cmn'])
    assert float(st.glob[0]) == float(z[name + '/amx']) and float(st.glob[1]) == float(z[name + '/amn'])
    thr_host = smooth_ops.osplus_thresholds(float(st.glob[0]), float(st.glob[1]))
    assert np.array_equal(np.array(thr_host), z[name + '/thresholds'])
    thr = torch.tensor(thr_host, dtype=x.dtype).cuda()
    for row, g in enumerate(z[name + '/sample_idx']):
        assert eq_bits(smooth_ops.osplus_scale(st.max, st.min, thr, int(g)), z[name + '/cur_scale'][row]), int(g)
    g = int(z[name + '/g_star'])
    cur = smooth_ops.osplus_scale(st.max, st.min, thr, g)
    layer = mod.searched()[0]
    assert eq_bits(algo._fake_quantize_weight(layer.weight.data, cur), z[name + '/wq_bits'])
    q_x = smooth_ops.act_step(xs, cur, algo.aquantizer)
    assert smooth_ops.act_step_fused_ok(xs, algo.aquantizer)               # K = 128 / 120: whole 16-byte vectors, tier 2
    assert eq_bits(q_x, z[name + '/q_x_bits'])
    assert torch.equal(q_x, smooth_ops.act_step(xs, cur, algo.aquantizer, force_two_kernels=True))
    if cfg['has_bias']:
        # osplus.py:134-135: a GEMV whose fp32 accumulation order is the BLAS's; within one unit of the bias dtype
        b = layer.bias.data + shift @ layer.weight.data.T
        want = C.from_bits(z[name + '/bias_shifted'], dt).float().cuda()
        assert ((b.float() - want).abs() <= ULP[dt] * want.abs() + 1e-6).all()


@pytest.mark.parametrize('name', OS_NAMES)
def test_osplus_search_curve_and_winner(name):
    z = C.gold()
    cfg, dt, mod, x = C.os_case(z, name)
    mod, x = mod.cuda(), x.cuda()
    sd0 = {k: v.clone() for k, v in mod.state_dict().items()}
    algo = _osplus(cfg, mod)
    scale, shift = algo.search_scale_shift_subset(mod.searched(), [x.clone()], mod, {})
    for k, v in mod.state_dict().items():
        assert torch.equal(v, sd0[k]), k                                    # weights and biases are back, bit for bit
    ls = algo.last_search
    gold, win_ref = z[name + '/loss'].astype(np.float64), int(z[name + '/win'])
    ours = ls['losses'].float().cpu().numpy().astype(np.float64)
    assert ls['losses'].dtype == DT[dt] and len(ours) == len(gold)          # the loss stays in the model dtype
    win = int(ls['index'])
    assert win == int(np.argmax(ours == ours.min()))                        # strict `>`: the first minimum
    dev = float(np.max(np.abs(ours - gold) / gold))
    print(f'{name}: {len(gold)} points, winner ours {win} / reference {win_ref}, reference curve at ours {gold[win]:.6g} vs its '
          f'minimum {gold.min():.6g}, max curve deviation {dev:.3e} (allowed {2 * REF_SELF_SPREAD[dt]:.3e})')
    if int(z[name + '/clear']):
        assert win == win_ref
    assert gold[win] <= gold.min() * (1 + 2 * ULP[dt])
    assert dev <= 2 * REF_SELF_SPREAD[dt]
    if win == win_ref:
        assert eq_bits(scale, z[name + '/scale'])
        if cfg['has_bias']:
            assert eq_bits(shift, z[name + '/shift'])
    assert (shift is None) == (not cfg['has_bias'])


def test_osplus_subset_transform_keeps_the_float_function_like_the_reference():
    """apply_shift + apply_scale on the fc1 subset of an OPT-shaped block: the block's float output moves no further than twice
    what the reference's own before / after pair shows (stored in the golden)."""
    z = C.gold()
    dt = 'f16'
    blk = C.load_state(z, 'transform/sd/', C.OptShaped(128, 128), dt).cuda()
    x = C.from_bits(z['transform/x_bits'], dt).reshape(1, -1, 128).cuda()
    import llmc_amd.compression.quantization as Q
    qc = {'method': 'OsPlus', 'weight': dict(bit=8, symmetric=True, granularity='per_channel'),
          'act': dict(bit=8, symmetric=True, granularity='per_token')}
    algo = Q.OsPlus(C.OneBlockModel(blk, True), qc, None, None, {})
    with torch.no_grad():
        before = blk(x).float()
        feat = blk.final_layer_norm(x)
    subset = {'layers': {'fc1': blk.fc1}, 'prev_op': [blk.final_layer_norm], 'input': ['fc1'], 'inspect': blk.fc1,
              'has_kwargs': False}
    w0 = blk.fc1.weight.data.clone()
    algo.subset_transform(subset, {'fc1': [feat.clone()]}, {})
    assert not torch.equal(blk.fc1.weight.data, w0)
    with torch.no_grad():
        after = blk(x).float()
    moved = float((before - after).abs().max())
    print(f'transform: max |before - after| = {moved:.3e}, the reference\'s {float(z["transform/before_after_maxabs"]):.3e}')
    assert moved <= 2 * float(z['transform/before_after_maxabs'])
    # and the transformed parameters are the reference's where the search chose the same threshold
    ref_after = {k[len('transform/sd_after/'):]: C.from_bits(z[k], dt) for k in z.files if k.startswith('transform/sd_after/')}
    ln_b = blk.final_layer_norm.bias.data.float().cpu()
    print('transform: final_layer_norm.bias max diff to the reference', float((ln_b - ref_after['final_layer_norm.bias'].float()).abs().max()))


# ---- the fused activation step against the parent's two kernels -------------------------------------------------------------
def tier(dt, K):
    """csrc/smooth_osplus.hip:act_step_tier restated"""
    v = 16 // (4 if dt == 'f32' else 2)
    if K % v:
        return 0
    per = -(-(K // v) // 256)
    return next((t for t in (2, 4, 8, 14) if per <= t), 0)


def planted(N, K, dt, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, K, generator=g) * torch.exp(0.5 * torch.randn(K, generator=g))).to(DT[dt])
    s = (1 + torch.rand(K, generator=g) * 3).to(DT[dt])
    s[::5] = 1.0
    x[0] = 0.0                                        # all-zero row: the scale clamps at 1e-5
    x[1] = 0.25                                       # constant row
    x[2] = (s.float() * 2.5).to(DT[dt])               # quotients on exact ties of the rounding
    x[3] = (s.float() * -0.5).to(DT[dt])
    x[:, 7] *= 300                                    # an outlier column
    x[4, :] = 0.0
    x[4, 11] = -3.0                                   # one non-zero element
    return x.cuda(), s.cuda()


AQ = [('int8_sym', dict(bit=8, symmetric=True, granularity='per_token')),
      ('int8_asym', dict(bit=8, symmetric=False, granularity='per_token')),
      ('int4_asym', dict(bit=4, symmetric=False, granularity='per_token')),
      ('e4m3_qtorch', dict(bit='e4m3', symmetric=True, granularity='per_token', use_qtorch=True, quant_type='float-quant')),
      ('e4m3_cast', dict(bit='e4m3', symmetric=True, granularity='per_token', use_qtorch=True, quant_type='float-quant',
                         fp8_semantics='cast')),
      ('e5m2_qtorch', dict(bit='e5m2', symmetric=True, granularity='per_token', use_qtorch=True, quant_type='float-quant')),
      ('e5m2_cast', dict(bit='e5m2', symmetric=True, granularity='per_token', use_qtorch=True, quant_type='float-quant',
                         fp8_semantics='cast'))]


def make_aq(kw):
    from llmc_amd.compression.quantization import FloatQuantizer, IntegerQuantizer
    kw = dict(kw)
    cls = FloatQuantizer if kw.pop('quant_type', 'int-quant') == 'float-quant' else IntegerQuantizer
    return cls(kw.pop('bit'), kw.pop('symmetric'), kw.pop('granularity'), **kw)


# (K, dtype, rows, the tier the case is written for)
WIDTHS = [(4096, 'bf16', 64, 2), (8192, 'bf16', 48, 4), (14336, 'bf16', 40, 8), (28672, 'bf16', 24, 14),
          (4096, 'f16', 64, 2), (14336, 'f16', 24, 8), (28672, 'f16', 16, 14), (4096, 'f32', 32, 4), (14336, 'f32', 16, 14),
          (1000, 'bf16', 33, 2), (1000, 'f32', 33, 2)]


@pytest.mark.parametrize('aq_name,aq_kw', AQ, ids=[a[0] for a in AQ])
@pytest.mark.parametrize('K,dt,N,want_tier', WIDTHS)
def test_fused_act_step_equals_div_cols_then_fake_quant(K, dt, N, want_tier, aq_name, aq_kw):
    from llmc_amd.compression.quantization import smooth_ops
    assert tier(dt, K) == want_tier == smooth_ops.act_step_tier(DT[dt], K)
    aq = make_aq(aq_kw)
    x, s = planted(N, K, dt, K + N)
    assert smooth_ops.act_step_fused_ok(x, aq)
    fused = smooth_ops.act_step(x, s, aq)
    two = smooth_ops.act_step(x, s, aq, force_two_kernels=True)
    assert fused.shape == x.shape and fused.dtype == x.dtype
    assert torch.equal(fused.view(torch.int32 if dt == 'f32' else torch.int16), two.view(torch.int32 if dt == 'f32' else torch.int16))
    assert torch.isfinite(fused).all()
    # 3-D inputs are rows of tokens
    f3 = smooth_ops.act_step(x.reshape(1, N, K), s, aq)
    assert torch.equal(f3.reshape(N, K), fused)


def test_fused_act_step_falls_back_where_it_says():
    """widths beyond 14 vectors per thread and quantizers the kernel does not evaluate take the parent's two kernels"""
    from llmc_amd import _ffi
    from llmc_amd.compression.quantization import smooth_ops
    assert tier('bf16', 28680) == 0 == smooth_ops.act_step_tier(torch.bfloat16, 28680)
    assert tier('f32', 28672) == 0 == smooth_ops.act_step_tier(torch.float32, 28672)
    assert smooth_ops.act_step_tier(torch.bfloat16, 1004) == 0                  # not whole 16-byte vectors
    x, s = planted(8, 28680, 'bf16', 3)
    aq = make_aq(AQ[0][1])
    assert not smooth_ops.act_step_fused_ok(x, aq)
    assert torch.equal(smooth_ops.act_step(x, s, aq), aq.fake_quant_act_dynamic(x / s))
    L = _ffi.lib()
    out = torch.empty_like(x)
    rc = L.llmc_osplus_act_step(_ffi.ptr(x), _ffi.ptr(s), _ffi.BF16, 8, 28680, 0, 1, -128.0, 127.0, 0, _ffi.ptr(out), _ffi.stream())
    assert rc == -95 and '14 per thread' in _ffi.last_error()
    x, s = planted(8, 4096, 'bf16', 4)
    per_tensor = make_aq(dict(bit=8, symmetric=True, granularity='per_tensor'))
    assert not smooth_ops.act_step_fused_ok(x, per_tensor)
    assert torch.equal(smooth_ops.act_step(x, s, per_tensor), per_tensor.fake_quant_act_dynamic(x / s))


# ---- end to end ---------------------------------------------------------------------------------------------------------------
W8A8 = dict(weight=Cfg(bit=8, symmetric=True, granularity='per_channel'), act=Cfg(bit=8, symmetric=True, granularity='per_token'))


def _with_bias_api(adapter, has_bias):
    """the adapters of tests/hf_adapters.py with the three methods OS+ and the shift fold call on a model"""
    class A(type(adapter)):
        def has_bias(self):
            return has_bias

        def get_num_attention_heads(self):
            return self.model_config.num_attention_heads

        def get_model_config(self):
            return self.model_config
    adapter.__class__ = A
    return adapter


@pytest.mark.parametrize('method', ['SmoothQuant', 'OsPlus'])
@pytest.mark.parametrize('arch', ['llama', 'opt'])
def test_end_to_end_block_loop_and_fake_quant_deploy(method, arch):
    import hf_adapters as H
    import llmc_amd.compression.quantization as Q
    if arch == 'llama':
        model = _with_bias_api(H.tiny_llama(torch.bfloat16), False)
        vocab, skipped, searched = 160, ('self_attn.o_proj', 'mlp.down_proj'), ('self_attn.q_proj', 'mlp.gate_proj')
    else:
        model = _with_bias_api(H.opt_125m_shaped(torch.float16, layers=2), True)
        vocab, skipped, searched = 512, ('self_attn.out_proj', 'fc2'), ('self_attn.q_proj', 'fc1')
    model.model.eval()                         # OPT has dropout: two forwards of one block would differ by it
    inp = model.collect_first_block_input(H.calib_ids(2, 64, vocab))
    blocks = model.get_blocks()
    w0 = [{n: m.weight.data.clone() for n, m in model.get_block_linears(b).items()} for b in blocks]
    ref_blocks = copy.deepcopy(blocks)
    inp0 = copy.deepcopy(inp)
    qc = Cfg(method=method, special=Cfg(alpha=0.5), **W8A8)
    algo = getattr(Q, method)(model, qc, inp, None, Cfg(calib=Cfg(seq_len=64), model=Cfg(type=arch)))
    algo.run_block_loop()
    for i, b in enumerate(blocks):
        for n, m in model.get_block_linears(b).items():
            assert torch.isfinite(m.weight.data).all(), (i, n)
            if n in skipped:                   # prev_op is a Linear, not a norm: the subset is not transformed
                assert torch.equal(m.weight.data.cpu(), w0[i][n].cpu()), (i, n)
            if n in searched:
                assert not torch.equal(m.weight.data.cpu(), w0[i][n].cpu()), (i, n)
    # the folds keep the float function of block 0 (same inputs in both)
    x = inp0['data'][0].cuda()
    # (the kwargs the algorithm kept: its constructor took the KV cache out, which a second forward would otherwise find filled)
    kw = {k: (v.cuda() if torch.is_tensor(v) else tuple(t.cuda() for t in v) if isinstance(v, tuple) else v)
          for k, v in algo.input['kwargs'][0].items()}
    with torch.no_grad():
        y_new, y_old = blocks[0].cuda()(x, **kw), ref_blocks[0].cuda()(x, **kw)
    y_new = (y_new[0] if isinstance(y_new, tuple) else y_new).float()
    y_old = (y_old[0] if isinstance(y_old, tuple) else y_old).float()
    rel = float((y_new - y_old).norm() / y_old.norm())
    print(f'{method} {arch}: block 0 float output moved by {rel:.3e} (relative Frobenius)')
    assert rel < 2e-2
    blocks[0].cpu()
    algo.deploy('fake_quant')
    for b in blocks:
        for n, m in model.get_block_linears(b).items():
            assert type(m).__name__ == 'EffcientFakeQuantLinear' and torch.isfinite(m.weight.data).all(), n
    model.model.cuda()
    with torch.no_grad():
        logits = model.model(H.calib_ids(1, 64, vocab, seed=5)[0].cuda()).logits
    assert torch.isfinite(logits).all()


def test_smoothquant_w8a8_vllm_quant_deploy():
    import hf_adapters as H
    import llmc_amd.compression.quantization as Q
    model = _with_bias_api(H.tiny_llama(torch.bfloat16), False)
    model.model.eval()
    inp = model.collect_first_block_input(H.calib_ids(2, 64, 160))
    qc = Cfg(method='SmoothQuant', special=Cfg(alpha=0.5), **W8A8)
    algo = Q.SmoothQuant(model, qc, inp, None, Cfg(calib=Cfg(seq_len=64), model=Cfg(type='Llama')))
    algo.run_block_loop()
    algo.deploy('vllm_quant')
    for b in model.get_blocks():
        for n, m in model.get_block_linears(b).items():
            assert type(m).__name__ == 'VllmRealQuantLinear', (n, type(m).__name__)
            assert m.weight.dtype == torch.int8 and torch.isfinite(m.weight_scale.float()).all(), n
