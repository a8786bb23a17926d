"""The mixed int / fp column kernel (csrc/mixed_quant.hip), its wrappers, and the methods on it (QUIK, LLM.int8()) on the GPU.

Every comparison is bit for bit: the kernel evaluates quant_math.h's functions like llmc_quant_dynamic does, so there is no
tolerance to choose. References: the reference's own outputs (tests/golden/mixed_quant.npz, tools/make_golden_mixed.py) and
mixed_ops.fake_quant_mixed_composed, the reference's gather -> quantize -> scatter sequence on the existing kernels."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden', 'mixed_quant.npz')
CONFIGS = os.path.join(HERE, 'golden', 'ref_mixed_configs.json')
DT = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}
DEV = 'cuda'


def _g():
    return np.load(GOLD)


def _from_bits(a, dt):
    if dt == 'f32':
        return torch.from_numpy(a.view(np.int32).copy()).view(torch.float32)
    return torch.from_numpy(a.view(np.int16).copy()).view(DT[dt])


def _same_bits(a, b):
    iv = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def _quantizer(cfg, **kw):
    from llmc_amd.compression.quantization import IntegerQuantizer
    extra = {'group_size': cfg['group_size']} if 'group_size' in cfg else {}
    return IntegerQuantizer(cfg['bit'], cfg['symmetric'], cfg['granularity'], **extra, **kw)


GOLD_ACT = ['act_1x5x40_f16', 'act_1x5x40_bf16', 'act_2x3x72_f16', 'act_2x3x72_bf16']
GOLD_W = ['w_6x40_int8_sym_per_channel_f16', 'w_6x40_int8_sym_per_channel_bf16', 'w_6x72_int8_sym_per_channel_f16',
          'w_6x72_int8_sym_per_channel_bf16', 'w_6x48_int4_asym_per_group16_f16', 'w_6x48_int4_asym_per_group16_bf16']


# ---- 1. the reference's own outputs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', GOLD_ACT + GOLD_W)
def test_golden_cases_equal_the_reference_bit_for_bit(name):
    g = _g()
    assert sorted(GOLD_ACT) == sorted(str(n) for n in g['act_names']) and sorted(GOLD_W) == sorted(str(n) for n in g['weight_names'])
    dt = str(g[name + '/dt'])
    x = _from_bits(g[name + '/x_bits'], dt).to(DEV)
    want = _from_bits(g[name + '/y_bits'], dt).to(DEV)
    args = {'int_indices': torch.from_numpy(g[name + '/int_ids']).to(DEV), 'fp_indices': torch.from_numpy(g[name + '/fp_ids']).to(DEV)}
    q = _quantizer(json.loads(str(g[name + '/cfg'])))
    got = q.fake_quant_act_dynamic(x, args) if name.startswith('act') else q.fake_quant_weight_dynamic(x, args)
    assert _same_bits(got, want)
    if name.startswith('act') and x.shape[0] == 1:            # activations may come as [T, K] too
        assert _same_bits(q.fake_quant_act_dynamic(x[0], args), want[0])
    # current_bit rides along without an arithmetic effect
    args['current_bit'] = torch.tensor(4)
    got = q.fake_quant_act_dynamic(x, args) if name.startswith('act') else q.fake_quant_weight_dynamic(x, args)
    assert _same_bits(got, want)


# ---- 2. kernel == composition ---------------------------------------------------------------------------------------------------
def _make_x(gen, N, K, dtype):
    c = torch.exp(0.5 * torch.randn(K, generator=gen))
    c[torch.randperm(K, generator=gen)[:max(1, K // 64)]] *= 30
    x = torch.randn(N, K, generator=gen) * c
    x[0, : min(K, 16)] = 0.0                      # a constant stretch: max == min -> clamp(1e-5) in some groups
    x[-1, K // 2] = -0.0
    return x.to(dtype).to(DEV)


def _columns(gen, K, n_fp, g, order):
    """-> (int_indices in `order`, fp_indices, n_int): n_fp pass-through columns, as many whole groups of g as fit the rest
    (g None: one group of everything that is left), the remainder zero."""
    perm = torch.randperm(K, generator=gen)
    fp, rest = perm[:n_fp], perm[n_fp:]
    n_int = rest.numel() if g is None else rest.numel() // g * g
    ints = rest[:n_int]
    if order == 'sorted':
        ints = torch.sort(ints)[0]
    elif order == 'reversed':
        ints = torch.sort(ints, descending=True)[0]
    return ints.to(DEV), fp.to(DEV), n_int


# (group size or None for one group per row, sym, round_zp): per_token / per_channel, per_group 16 and 128
QCFG = [(g, sym, rz) for g in (None, 16, 128) for sym in (True, False) for rz in (True, False)]
SHAPES = [(1, 8, 'f16'), (3, 36, 'bf16'), (3, 36, 'f32'), (5, 4100, 'f16'), (7, 768, 'bf16'), (7, 768, 'f32'),
          (2, 4096, 'bf16'), (2, 14336, 'bf16'), (1, 28672, 'bf16'), (2, 14336, 'f32'), (1, 28672, 'f32')]


@pytest.mark.parametrize('N,K,dt', SHAPES)
def test_kernel_equals_the_composition(N, K, dt):
    from llmc_amd.compression.quantization import mixed_ops
    gen = torch.Generator().manual_seed(1000 * N + K)
    x = _make_x(gen, N, K, DT[dt])
    x0 = x.clone()
    ran = 0
    for g, sym, rz in QCFG:
        qmin, qmax = (-128.0, 127.0) if sym else (0.0, 15.0)
        n_fps = {0, 1, K - (g or 1)} | ({256} if 256 < K else set())
        for n_fp in sorted(n for n in n_fps if 0 <= n < K and (g is None or K - n >= g)):
            for order in ('sorted', 'reversed', 'random'):
                ints, fp, n_int = _columns(gen, K, n_fp, g, order)
                gg = n_int if g is None else g
                got = mixed_ops.fake_quant_mixed(x, ints, fp, gg, sym, rz, qmin, qmax)
                want = mixed_ops.fake_quant_mixed_composed(x, ints, fp, gg, sym, rz, qmin, qmax)
                assert _same_bits(got, want), (g, sym, rz, n_fp, order)
                ran += 1
    assert ran >= 12 * 3 * (1 if K < 16 else 2)
    assert _same_bits(x, x0)                      # the input is left alone
    # (1, 28672) f32 is 112 KiB of LDS: whichever route the wrapper takes, it said so up front
    assert mixed_ops.kernel_takes(x) == bool(K * x.element_size() + 64 <= 160 * 1024)


def test_rows_the_resident_kernel_refuses_take_the_composition():
    from llmc_amd import _ffi
    from llmc_amd.compression.quantization import mixed_ops
    gen = torch.Generator().manual_seed(5)
    K = 90112                                     # 176 KiB of bf16: above the LDS of a CU
    x = _make_x(gen, 1, K, torch.bfloat16)
    ints, fp, n_int = _columns(gen, K, 256, None, 'random')
    assert not mixed_ops.kernel_takes(x)
    role = mixed_ops.make_roles(K, ints, fp, x.device)
    out = torch.empty_like(x)
    rc = _ffi.lib().llmc_quant_dynamic_mixed(_ffi.ptr(x), _ffi.dt(x), 1, K, _ffi.ptr(role), None, n_int, n_int, 1, 1, -128.0,
                                             127.0, _ffi.ptr(out), _ffi.stream())
    assert rc == -95
    got = mixed_ops.fake_quant_mixed(x, ints, fp, n_int, True, True, -128.0, 127.0)
    assert _same_bits(got, mixed_ops.fake_quant_mixed_composed(x, ints, fp, n_int, True, True, -128.0, 127.0))


def test_long_groups_and_an_ordered_single_group():
    """Code paths the shipped granularities do not reach through the wrapper: groups above 1024 columns (the workgroup is the
    team), and one group per row given WITH its order (the entry point then gathers; the mask-driven kernel must agree)."""
    from llmc_amd import _ffi
    from llmc_amd.compression.quantization import mixed_ops
    gen = torch.Generator().manual_seed(6)
    x = _make_x(gen, 3, 8192, torch.bfloat16)
    ints, fp, n_int = _columns(gen, 8192, 100, 2048, 'random')
    assert n_int == 6144
    for sym, rz in ((True, True), (False, True), (False, False)):
        qmin, qmax = (-8.0, 7.0) if sym else (0.0, 15.0)
        got = mixed_ops.fake_quant_mixed(x, ints, fp, 2048, sym, rz, qmin, qmax)
        assert _same_bits(got, mixed_ops.fake_quant_mixed_composed(x, ints, fp, 2048, sym, rz, qmin, qmax))
    x = _make_x(gen, 5, 768, torch.float16)
    ints, fp, n_int = _columns(gen, 768, 40, None, 'random')
    role = mixed_ops.make_roles(768, ints, fp, x.device)
    idx = ints.to(torch.int32)
    out = torch.empty_like(x)
    _ffi.check(_ffi.lib().llmc_quant_dynamic_mixed(_ffi.ptr(x), _ffi.dt(x), 5, 768, _ffi.ptr(role), _ffi.ptr(idx), n_int, n_int, 0,
                                                   1, 0.0, 255.0, _ffi.ptr(out), _ffi.stream()), 'llmc_quant_dynamic_mixed')
    assert _same_bits(out, mixed_ops.fake_quant_mixed(x, ints, fp, n_int, False, True, 0.0, 255.0))


def test_a_column_named_in_both_lists_passes_through_and_counts_in_the_range():
    from llmc_amd.compression.quantization import mixed_ops
    gen = torch.Generator().manual_seed(7)
    x = _make_x(gen, 4, 256, torch.bfloat16)
    x[:, 9] = 500.0                               # the shared column dominates its group's range
    for g in (None, 16):
        ints, fp, n_int = _columns(gen, 256, 16, g, 'random')
        fp = torch.cat([fp, ints[3:4]])
        x[:, ints[3]] = 500.0
        gg = n_int if g is None else g
        got = mixed_ops.fake_quant_mixed(x, ints, fp, gg, True, True, -128.0, 127.0)
        assert _same_bits(got, mixed_ops.fake_quant_mixed_composed(x, ints, fp, gg, True, True, -128.0, 127.0))
        assert _same_bits(got[:, ints[3]], x[:, ints[3]])


# ---- 3. no fp columns == the plain path -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', [dict(bit=8, symmetric=True, granularity='per_token'),
                                 dict(bit=4, symmetric=False, granularity='per_group', group_size=128)])
def test_without_fp_columns_it_is_the_plain_dynamic_quantizer(cfg):
    gen = torch.Generator().manual_seed(8)
    x = _make_x(gen, 10, 768, torch.bfloat16).reshape(2, 5, 768)
    q = _quantizer(cfg)
    args = {'int_indices': torch.arange(768, device=DEV), 'fp_indices': torch.empty(0, dtype=torch.long, device=DEV)}
    assert _same_bits(q.fake_quant_act_dynamic(x, args), q.fake_quant_act_dynamic(x))
    w = x.reshape(10, 768)
    assert _same_bits(q.fake_quant_weight_dynamic(w, args), q.fake_quant_weight_dynamic(w))


# ---- 4. special values in the pass-through columns ---------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['f16', 'bf16', 'f32'])
@pytest.mark.parametrize('g', [None, 16])
def test_pass_through_columns_keep_their_bits_and_do_not_leak_into_the_ranges(dt, g):
    from llmc_amd.compression.quantization import mixed_ops
    gen = torch.Generator().manual_seed(9)
    N, K = 7, 768
    x = _make_x(gen, N, K, DT[dt])
    ints, fp, n_int = _columns(gen, K, 6, g, 'random')
    iv = torch.int32 if dt == 'f32' else torch.int16
    nan1, nan2, neg0 = {'f16': (0x7E01, 0xFE55, 0x8000), 'bf16': (0x7FC1, 0xFFA5, 0x8000),
                        'f32': (0x7FC00001, 0xFFA00055, 0x80000000)}[dt]

    def signed(v):
        bits_ = 32 if dt == 'f32' else 16
        return v - (1 << bits_) if v >= 1 << (bits_ - 1) else v
    xv = x.view(iv)
    xv[:, fp[0]] = signed(nan1)
    xv[:, fp[1]] = signed(nan2)
    x[:, fp[2]] = float('inf')
    x[:, fp[3]] = float('-inf')
    xv[:, fp[4]] = signed(neg0)
    x[:, fp[5]] = 65504.0
    zero_cols = torch.ones(K, dtype=torch.bool, device=DEV)
    zero_cols[ints] = False
    zero_cols[fp] = False
    x[:, zero_cols] = 3.0                         # whatever they hold, they come out +0
    gg = n_int if g is None else g
    for sym in (True, False):
        qmin, qmax = (-128.0, 127.0) if sym else (0.0, 255.0)
        got = mixed_ops.fake_quant_mixed(x, ints, fp, gg, sym, True, qmin, qmax)
        assert _same_bits(got[:, fp], x[:, fp])
        clean = x.clone()
        clean[:, fp] = 0.0                        # the integer columns do not see the outliers at all
        want = mixed_ops.fake_quant_mixed_composed(clean, ints, fp, gg, sym, True, qmin, qmax)
        assert _same_bits(got[:, ints], want[:, ints])
        assert torch.isfinite(got[:, ints].float()).all()
        if g is not None:
            assert int(zero_cols.sum()) > 0
        assert (got[:, zero_cols].contiguous().view(iv) == 0).all()


# ---- 5. in place -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,K,g', [(7, 768, None), (7, 768, 16), (2, 14336, None), (3, 36, 16)])
def test_in_place_gives_the_same_bits(N, K, g):
    from llmc_amd.compression.quantization import mixed_ops
    gen = torch.Generator().manual_seed(10)
    x = _make_x(gen, N, K, torch.bfloat16)
    ints, fp, n_int = _columns(gen, K, 5, g, 'random')
    gg = n_int if g is None else g
    want = mixed_ops.fake_quant_mixed(x, ints, fp, gg, False, True, 0.0, 15.0)
    y = x.clone()
    res = mixed_ops.fake_quant_mixed(y, ints, fp, gg, False, True, 0.0, 15.0, out=y)
    assert res.data_ptr() == y.data_ptr() and _same_bits(y, want)


# ---- 6. LLM.int8() on one FakeQuantLinear --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['f16', 'bf16'])
def test_llmint8_on_one_fake_quant_linear(dt):
    import llmc_amd.compression.quantization as Q
    g = _g()
    an, wn = f'act_2x3x72_{dt}', f'w_6x72_int8_sym_per_channel_{dt}'
    x = _from_bits(g[an + '/x_bits'], dt).to(DEV)
    lin = torch.nn.Linear(72, 6, bias=False)
    lin.weight.data = _from_bits(g[wn + '/x_bits'], dt)
    lin = lin.to(DEV)
    algo = object.__new__(Q.LlmInt8)
    algo.threshold = float(g['threshold'])
    algo.wquantizer = _quantizer(json.loads(str(g[wn + '/cfg'])))
    algo.aquantizer = _quantizer(json.loads(str(g[an + '/cfg'])))
    seen = {}

    def a_qdq(act, module):
        seen['a'] = algo.a_qdq(act, module, algo.aquantizer)
        return seen['a']
    mod = Q.FakeQuantLinear.new(lin, w_qdq=functools.partial(algo.w_qdq, wquantizer=algo.wquantizer), a_qdq=a_qdq)
    y = mod(x)
    assert y.shape == (2, 3, 6) and torch.isfinite(y.float()).all()
    want_fp = sorted(set(g[an + '/fp_ids'].tolist()))          # the reference lists column 7 once per batch row
    assert len(want_fp) < len(g[an + '/fp_ids'])
    assert mod.buf_fp_ids.tolist() == want_fp
    assert mod.buf_int_ids.tolist() == g[an + '/int_ids'].tolist() == [c for c in range(72) if c not in want_fp]
    assert _same_bits(seen['a'], _from_bits(g[an + '/y_bits'], dt).to(DEV))
    assert _same_bits(mod.tmp_weight, _from_bits(g[wn + '/y_bits'], dt).to(DEV))


# ---- 7. QUIK on the toy model -----------------------------------------------------------------------------------------------------
def _quik_cfg(fp_features):
    cfg = json.load(open(CONFIGS))['methods/QUIK/quik_w_a.yml']
    cfg['quant']['special'] = dict(cfg['quant']['special'], fp_features=fp_features)
    return cfg


def _torch_scales(model, inp):
    """per Linear: running max over the batches of |x|.amax over the tokens, with plain torch on the same device"""
    net = model.get_model()
    out, hooks = {}, []

    def hook(m, x, y, name):
        s = x[0].detach().reshape(-1, x[0].shape[-1]).abs().amax(0).float()
        out[name] = torch.maximum(out[name], s) if name in out else s
    for name, m in net.named_modules():
        if isinstance(m, torch.nn.Linear):
            hooks.append(m.register_forward_hook(functools.partial(hook, name=name)))
    data = [d.to(DEV) for d in inp['data']]
    with torch.no_grad():
        for b in model.get_blocks():
            b.to(DEV)
            data = [b(d) for d in data]
    for h in hooks:
        h.remove()
    return out


def test_quik_on_the_toy_model():
    import llmc_amd.compression.quantization as Q
    from llmc_amd.compression.quantization import mixed_ops
    from toy_model import ToyModel, calib_input
    model = ToyModel(hidden=256, inner=384, n_blocks=2)
    inp = calib_input(model, n_seq=4, seq=16)
    want_scales = _torch_scales(model, {'data': list(inp['data'])})
    cfg = _quik_cfg(32)
    algo = Q.QUIK(model, dict(cfg['quant']), inp, None, {'calib': cfg['calib'], 'model': cfg['model'], 'quant': cfg['quant']})
    assert set(algo.act_scales) == set(want_scales) and len(want_scales) == 6
    scales = {k: v.clone() for k, v in algo.act_scales.items()}
    for k in scales:
        assert scales[k].dtype == torch.float32 and torch.equal(scales[k], want_scales[k]), k
    algo.run_block_loop()
    assert algo.act_scales == {}
    model.get_model().to(DEV)
    gen = torch.Generator().manual_seed(11)
    for bi, block in enumerate(model.get_blocks()):
        for n, m in model.get_block_linears(block).items():
            K = m.in_features
            order = torch.sort(scales[f'blocks.{bi}.{n}'], stable=True)[1]
            assert torch.equal(m.buf_int_ids, order[:K - 32]) and torch.equal(m.buf_fp_ids, order[K - 32:])
            assert int(m.buf_current_bit) == 8 if n == 'down_proj' else not hasattr(m, 'buf_current_bit')
            n_int = K - 32
            w = algo.w_qdq(m, algo.wquantizer)
            assert _same_bits(w, mixed_ops.fake_quant_mixed_composed(m.weight.data, m.buf_int_ids, m.buf_fp_ids, n_int, True, True,
                                                                    -128.0, 127.0))
            a = _make_x(gen, 32, K, torch.bfloat16).reshape(2, 16, K)
            got = algo.a_qdq(a, m, algo.aquantizer)
            want = mixed_ops.fake_quant_mixed_composed(a.reshape(-1, K), m.buf_int_ids, m.buf_fp_ids, n_int, True, True, -128.0,
                                                       127.0)
            assert _same_bits(got, want.reshape(2, 16, K))
    algo.deploy('fake_quant', keep_device=True)
    assert all(type(getattr(b, n)).__name__ == 'EffcientFakeQuantLinear' for b in model.get_blocks()
               for n in ('gate_proj', 'up_proj', 'down_proj'))
    h = inp['data'][0].to(DEV)
    with torch.no_grad():
        for b in model.get_blocks():
            h = b(h)
    assert h.shape == (1, 16, 256) and torch.isfinite(h.float()).all()


@pytest.mark.parametrize('rel', ['methods/QUIK/quik_w_a.yml', 'methods/LlmInt8/llmint8_w_only.yml'])
def test_shipped_configs_run_through_the_block_loop_and_deploy(rel):
    """the reference's configs as they are (QUIK keeps 256 channels, so the toy model is 512 wide)"""
    import llmc_amd.compression.quantization as Q
    from toy_model import ToyModel, calib_input
    cfg = json.load(open(CONFIGS))[rel]
    model = ToyModel(hidden=512, inner=768, n_blocks=2)
    inp = calib_input(model, n_seq=2, seq=16)
    algo = getattr(Q, cfg['quant']['method'])(model, dict(cfg['quant']), inp, None,
                                              {'calib': cfg['calib'], 'model': cfg['model'], 'quant': cfg['quant']})
    algo.run_block_loop()
    algo.deploy('fake_quant', keep_device=True)
    h = inp['data'][0].to(DEV)
    with torch.no_grad():
        for b in model.get_blocks():
            h = b(h)
    assert h.shape == (1, 16, 512) and torch.isfinite(h.float()).all()
    lin = model.get_blocks()[0].down_proj
    assert lin.buf_int_ids.numel() + lin.buf_fp_ids.numel() == 768
    if cfg['quant']['method'] == 'QUIK':
        assert lin.buf_fp_ids.numel() == 256
