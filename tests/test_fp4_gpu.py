"""FloatQuantizer on the narrow float grids e2m1 / e3m2 on the GPU (llmc_fpx_quant, llmc_fp4_pack, llmc_fpx_dequant,
csrc/fp4_quant.hip) against the numpy oracle (tests/fp4_oracle.py) and the reference's own output (tests/golden/fp4.npz),
bit for bit."""
import copy

import numpy as np
import pytest
import torch

import fp4_oracle as O

pytestmark = pytest.mark.gpu

TDT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
BITS = ('e2m1', 'e3m2')
SEMS = ('qtorch', 'ocp')


class Cfg(dict):
    __getattr__ = dict.get


def quantizer(bit, gran, gs=0, sem='qtorch', scale_format='dtype', **kw):
    from llmc_amd.compression.quantization import FloatQuantizer
    if gs:
        kw['group_size'] = gs
    return FloatQuantizer(bit, True, gran, use_qtorch=True, float_semantics=sem, scale_format=scale_format, **kw)


def to_gpu(a, dt):
    """fp32 container of dt values -> a GPU tensor of that dtype, through the bit patterns (NaN payloads and signs survive)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dt == 'f32':
        return torch.from_numpy(a.view(np.int32).copy()).cuda().view(torch.float32)
    return torch.from_numpy(O.bits16(a, dt).view(np.int16).copy()).cuda().view(TDT[dt])


def bits_of(t):
    """a GPU float tensor -> its bit patterns (numpy)"""
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def want_bits(a, dt):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a.view(np.uint32) if dt == 'f32' else O.bits16(a, dt)


def all_patterns(dt):
    """every 16-bit pattern of dt / 1 M seeded fp32 values with the special ones among them, as an fp32 container"""
    if dt == 'f32':
        rng = np.random.default_rng(2024)
        x = (rng.standard_normal(1 << 20) * np.exp2(rng.integers(-12, 8, 1 << 20))).astype(np.float32)
        x[:16] = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 0.25, -0.25, 2.5, -2.5, 5.0, 0.75, 1e-40, -1e-40, 3e38, 6.0],
                          np.float32)
        x.view(np.uint32)[16] = 0xffc01234       # a negative NaN with a payload
        return x
    return O.from_bits16(np.arange(65536, dtype=np.uint32).astype(np.uint16), dt)


def defined(x, sem):
    """Where the semantics define the result: 'ocp' everywhere (a NaN gives the signed maximum); 'qtorch' on every non-NaN
    input (the restated bit arithmetic saturates an infinity; a NaN's result depends on payload bits no caller relies on)."""
    return np.ones(x.shape, bool) if sem == 'ocp' else ~np.isnan(x)


# ---- 1. exhaustive ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['bf16', 'f16', 'f32'])
def test_every_input_pattern_with_static_scales(dt):
    x = all_patterns(dt)
    xg = to_gpu(x, dt).reshape(1, -1)
    for bit in BITS:
        for sem in SEMS:
            q = quantizer(bit, 'per_tensor', sem=sem)
            for s in (1.0, 0.37):
                st = torch.tensor(s, dtype=torch.float32, device='cuda')
                want = O.run(x.reshape(1, -1), dt, bit, sem, scales=np.array([[s]], np.float32), sdt='f32')
                ok = defined(x, sem)
                codes, _ = q._run(xg, False, scales=st)
                fake, _ = q._run(xg, True, scales=st)
                got_c, got_f = codes.cpu().numpy().reshape(-1), bits_of(fake).reshape(-1)
                bad_c = (got_c != want['codes'].reshape(-1)) & ok
                bad_f = (got_f != want_bits(want['fake'], dt).reshape(-1)) & ok
                assert not bad_c.any(), (dt, bit, sem, s, int(bad_c.sum()), x[bad_c][:4], got_c[bad_c][:4])
                assert not bad_f.any(), (dt, bit, sem, s, int(bad_f.sum()), x[bad_f][:4])
                assert got_c.max() < (16 if bit == 'e2m1' else 64)          # the bits above the code are zero


def mixed_rows(dt, g=128):
    """Every finite pattern of a 16-bit dtype in rows of g whose elements span four binades (half a row from one magnitude
    band, a quarter each from one and three binades below), seeded signs: the quotients w / s of the dynamic path then cover
    the grid, rounding boundaries of the tensor dtype included."""
    x = all_patterns(dt)
    p = np.sort(np.abs(x[np.isfinite(x)]))
    p = np.unique(p)
    p = p[: len(p) // g * g].reshape(-1, g)
    nb = (128 if dt == 'bf16' else 1024) // g or 1          # rows per binade
    i = np.arange(p.shape[0])
    rows = np.concatenate([p[i, : g // 2], p[np.maximum(i - nb, 0), g // 2: 3 * g // 4], p[np.maximum(i - 3 * nb, 0), 3 * g // 4:]], axis=1)
    sign = np.random.default_rng(7).integers(0, 2, rows.shape) * 2 - 1
    return (rows * sign).astype(np.float32)


@pytest.mark.parametrize('dt', ['bf16', 'f16'])
def test_every_finite_pattern_with_dynamic_group_scales(dt):
    """The single-read kernels' division-free path (w * fl(1 / s) with the boundary guard) on every 16-bit pattern."""
    x = mixed_rows(dt)
    xg = to_gpu(x, dt)
    for bit in BITS:
        for sem in SEMS:
            q = quantizer(bit, 'per_group', 128, sem=sem)
            want = O.run(x, dt, bit, sem)
            codes, s = q._run(xg, False)
            fake, _ = q._run(xg, True)
            assert np.array_equal(bits_of(s).reshape(-1), want_bits(want['scales'], dt).reshape(-1)), (dt, bit, sem)
            bad = codes.cpu().numpy() != want['codes']
            assert not bad.any(), (dt, bit, sem, int(bad.sum()), x[bad][:4])
            assert np.array_equal(bits_of(fake), want_bits(want['fake'], dt)), (dt, bit, sem)


# ---- 2. goldens -------------------------------------------------------------------------------------------------------------
def test_reference_goldens_through_the_quantizer_methods(golden):
    g = golden('fp4')
    names = [str(n) for n in g['names']]
    assert len(names) == 8
    for n in names:
        dt, bit, gran, kind = str(g[n + '/dt']), str(g[n + '/bit']), str(g[n + '/gran']), str(g[n + '/kind'])
        gs = int(g[n + '/meta'][3])
        kw = dict(calib_algo='static_minmax') if kind == 'act_static' else {}
        q = quantizer(bit, gran, gs, **kw)
        assert (q.e_bits, q.m_bits, q.num_bits) == tuple(int(v) for v in g[n + '/meta'][:3])
        assert float(q.qmin) == g[n + '/meta'][4] and float(q.qmax) == g[n + '/meta'][5]
        x = torch.from_numpy(g[n + '/x_bits'].view(np.int16).copy()).cuda().view(TDT[dt])
        sdt = {'torch.bfloat16': torch.bfloat16, 'torch.float16': torch.float16, 'torch.float32': torch.float32}[str(g[n + '/scales_dtype'])]
        if kind == 'act_static':
            s_list, z_list, qmin_list, qmax_list = q.get_batch_tensors_qparams([x])
            scales, zeros, qmax, qmin = s_list[0], z_list[0], qmax_list[0], qmin_list[0]
            t = q.reshape_tensor(x)
            fake = q.fake_quant_act_static(x, dict(scales=scales.clone(), zeros=zeros, qmax=qmax, qmin=qmin))
        else:
            t, scales, zeros, qmax, qmin = q.get_tensor_qparams(x)
            fake = q.fake_quant_weight_dynamic(x) if kind == 'weight' else q.fake_quant_act_dynamic(x)
        assert scales.dtype == sdt, (n, scales.dtype)
        assert np.array_equal(scales.float().cpu().numpy().reshape(-1).view(np.uint32), g[n + '/scales'].view(np.uint32)), n
        assert fake.dtype == TDT[dt] and fake.shape == x.shape
        assert np.array_equal(bits_of(fake), g[n + '/fake_bits']), n
        qv = q.quant(t, scales.clone(), zeros, qmax, qmin)
        assert qv.dtype == torch.float32
        assert np.array_equal(qv.cpu().numpy().view(np.uint32).reshape(-1), g[n + '/q'].view(np.uint32).reshape(-1)), n
        qd = q.quant_dequant(t, scales.clone(), zeros, qmax, qmin)
        assert np.array_equal(bits_of(qd.to(TDT[dt])).reshape(-1), g[n + '/fake_bits'].reshape(-1)), n
        if n + '/static_scales' in g.files:
            s2 = torch.from_numpy(g[n + '/static_scales']).to(sdt).cuda().reshape(scales.shape)
            sf = q.fake_quant_weight_static(x, dict(scales=s2, zeros=zeros, qmax=qmax, qmin=qmin))
            assert np.array_equal(bits_of(sf), g[n + '/static_fake_bits']), n


# ---- 3. shapes --------------------------------------------------------------------------------------------------------------
def rand_rows(shape, dt, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 0.05 * np.exp(0.8 * rng.standard_normal(shape[-1]))).astype(np.float32)
    x.reshape(-1)[3], x.reshape(-1)[4] = 0.0, -0.0
    from oracle import quant_ref as Q
    return Q.rnd(x, dt)


SHAPES = [
    # (id, granularity, group size, shape, dtype): which kernel takes it
    ('g32', 'per_group', 32, (5, 96), 'bf16'),              # k_fpx_seg, 4 lanes per group
    ('g64', 'per_group', 64, (5, 192), 'f16'),              # k_fpx_seg, 8 lanes
    ('g128', 'per_group', 128, (5, 384), 'bf16'),           # k_fpx_seg, 16 lanes
    ('g128_f32', 'per_group', 128, (5, 384), 'f32'),        # k_fpx_seg, 32 lanes (cross-row exchange)
    ('g512', 'per_group', 512, (3, 1024), 'f16'),           # k_fpx_seg, 64 lanes
    ('g128_blocks', 'per_group', 128, (70, 512), 'bf16'),   # more than one workgroup, a partial last one
    ('pc320', 'per_channel', 0, (5, 320), 'bf16'),          # k_fpx_row (40 vectors)
    ('pc320_f32', 'per_channel', 0, (3, 320), 'f32'),
    ('pc33', 'per_channel', 0, (5, 33), 'f16'),             # scalar fallback
    ('pc16384', 'per_channel', 0, (2, 16384), 'bf16'),      # the resident bound itself
    ('pc16392', 'per_channel', 0, (3, 16392), 'bf16'),      # one vector past it: two reads
    ('pt', 'per_tensor', 0, (3, 320), 'bf16'),              # one row of 960: k_fpx_row
    ('pt_long', 'per_tensor', 0, (24, 1024), 'f16'),        # one row of 24576: two reads
]


@pytest.mark.parametrize('case', SHAPES, ids=[c[0] for c in SHAPES])
@pytest.mark.parametrize('sem', SEMS)
def test_shapes_where_the_kernel_takes_another_path(case, sem):
    name, gran, gs, shape, dt = case
    x = rand_rows(shape, dt, 100 + len(name))
    for bit in BITS:
        q = quantizer(bit, gran, gs, sem=sem)
        x2 = x.reshape(1, -1) if gran == 'per_tensor' else (x.reshape(-1, gs) if gs else x)
        want = O.run(x2, dt, bit, sem)
        xg = to_gpu(x, dt)
        fake = q.fake_quant_weight_dynamic(xg)
        codes, s = q._run(q.reshape_tensor(xg), False)
        assert s.dtype == TDT[dt]
        assert np.array_equal(bits_of(s).reshape(-1), want_bits(want['scales'], dt).reshape(-1)), (name, bit)
        assert np.array_equal(codes.cpu().numpy().reshape(x2.shape), want['codes']), (name, bit)
        assert np.array_equal(bits_of(fake).reshape(x2.shape), want_bits(want['fake'], dt)), (name, bit)


def test_misaligned_view_and_given_scales():
    """A view offset by one element (no 16-byte alignment: the scalar pass), and given scales with a zero among them (it
    quantizes with 1 and the caller's tensor is left alone)."""
    dt = 'bf16'
    x = rand_rows((5, 384), dt, 5)
    buf = torch.zeros(5 * 384 + 8, dtype=TDT[dt], device='cuda')
    buf[1:1 + 5 * 384] = to_gpu(x, dt).reshape(-1)
    view = buf[1:1 + 5 * 384].view(5, 384)
    assert view.data_ptr() % 16 != 0
    q = quantizer('e2m1', 'per_group', 128)
    want = O.run(x.reshape(-1, 128), dt, 'e2m1')
    t = view.reshape(-1, 128)
    assert t.data_ptr() == view.data_ptr()
    fake, s = q._run(t, True)
    assert np.array_equal(bits_of(fake), want_bits(want['fake'], dt))
    assert np.array_equal(bits_of(s).reshape(-1), want_bits(want['scales'], dt).reshape(-1))
    given = want['scales'].copy()
    given[::4] = 0.0
    sg = to_gpu(given, dt)
    keep = sg.clone()
    want2 = O.run(x.reshape(-1, 128), dt, 'e2m1', scales=given, sdt=dt)
    fake2 = q.fake_quant_weight_static(to_gpu(x, dt), dict(scales=sg, zeros=torch.tensor(0.0), qmax=q.qmax, qmin=q.qmin))
    assert np.array_equal(bits_of(fake2).reshape(-1, 128), want_bits(want2['fake'], dt))
    assert torch.equal(sg, keep)


# ---- 4. the column multiplier -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(6, 384), (4096, 512)])
@pytest.mark.parametrize('dt', ['bf16', 'f16'])
def test_fused_column_multiplier_equals_mul_cols_then_quantize(shape, dt):
    from llmc_amd.compression.quantization import awq_ops
    gen = torch.Generator().manual_seed(shape[0])
    w = (torch.randn(shape, generator=gen) * 0.05).to(TDT[dt]).cuda()
    cols = (0.5 + 1.5 * torch.rand(shape[1], generator=gen)).to(TDT[dt]).cuda()
    keep = w.clone()
    for bit, gran, gs, sem in (('e2m1', 'per_group', 128, 'qtorch'), ('e2m1', 'per_channel', 0, 'ocp'), ('e3m2', 'per_group', 64, 'qtorch')):
        q = quantizer(bit, gran, gs, sem=sem)
        t = q.reshape_tensor(w)
        assert q.fused_cols_ok(t)
        for fake in (True, False):
            out1, s1 = q._run(t, fake, cols=cols)
            assert torch.equal(w, keep)
            w2 = awq_ops.mul_cols_(w.clone(), cols)
            out2, s2 = q._run(q.reshape_tensor(w2), fake)
            assert torch.equal(out1.view(torch.uint8), out2.view(torch.uint8)), (bit, gran, fake)
            assert torch.equal(s1.view(torch.uint8), s2.view(torch.uint8)), (bit, gran, fake)
    # small case against the oracle too
    if shape[0] == 6:
        q = quantizer('e2m1', 'per_group', 128)
        out, _ = q._run(q.reshape_tensor(w), True, cols=cols)
        wn = O.mul_cols(w.float().cpu().numpy(), cols.float().cpu().numpy(), dt)
        want = O.run(wn.reshape(-1, 128), dt, 'e2m1')
        assert np.array_equal(bits_of(out), want_bits(want['fake'], dt))


# ---- 5. the stored form -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(4, 96), (64, 256)])
@pytest.mark.parametrize('mx', [False, True])
def test_pack_and_dequant(shape, mx):
    from llmc_amd.compression.quantization import dequant_fpx, pack_fp4
    dt = 'f16'
    x = rand_rows(shape, dt, 31 + shape[0])
    xg = to_gpu(x, dt)
    q = quantizer('e2m1', 'per_group', 32, sem='ocp' if mx else 'qtorch', scale_format='e8m0' if mx else 'dtype')
    want = O.run(x.reshape(-1, 32), dt, 'e2m1', 'ocp' if mx else 'qtorch', 'e8m0' if mx else 'dtype')
    codes, s = q._run(q.reshape_tensor(xg), False)
    codes = codes.reshape(shape)
    assert np.array_equal(codes.cpu().numpy(), want['codes'].reshape(shape))
    packed = pack_fp4(codes)
    assert packed.shape == (shape[0], shape[1] // 2) and packed.dtype == torch.uint8
    assert np.array_equal(packed.cpu().numpy(), O.pack_fp4(want['codes'].reshape(shape)))
    pw, ps, pz = q.real_quant_weight_dynamic(xg)
    assert pz is None and torch.equal(pw, packed) and ps.shape == (shape[0], shape[1] // 32)
    assert ps.dtype == (torch.uint8 if mx else TDT[dt]) and torch.equal(ps.reshape(-1), s.reshape(-1))
    fake = q.fake_quant_weight_dynamic(xg)
    assert np.array_equal(bits_of(fake).reshape(-1, 32), want_bits(want['fake'], dt))
    assert torch.equal(dequant_fpx(packed, ps, 'e2m1', 32, TDT[dt]).view(torch.int16), fake.view(torch.int16))
    assert torch.equal(dequant_fpx(codes, ps, 'e2m1', 32, TDT[dt], packed=False).view(torch.int16), fake.view(torch.int16))
    # e3m2: one code per byte
    q6 = quantizer('e3m2', 'per_group', 32, sem='ocp' if mx else 'qtorch', scale_format='e8m0' if mx else 'dtype')
    w6, s6, _ = q6.real_quant_weight_dynamic(xg)
    want6 = O.run(x.reshape(-1, 32), dt, 'e3m2', 'ocp' if mx else 'qtorch', 'e8m0' if mx else 'dtype')
    assert w6.shape == shape and np.array_equal(w6.cpu().numpy().reshape(-1, 32), want6['codes'])
    f6 = q6.fake_quant_weight_dynamic(xg)
    assert torch.equal(dequant_fpx(w6, s6, 'e3m2', 32, TDT[dt]).view(torch.int16), f6.view(torch.int16))


# ---- 6. MX ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bit', BITS)
@pytest.mark.parametrize('dt', ['bf16', 'f32'])
def test_mx_block_scales(bit, dt):
    x = rand_rows((8, 96), dt, 77)
    x2 = x.reshape(-1, 32).copy()
    x2[0] = 0.0                                            # an all-zero block: code 127
    x2[1, 5] = 4.0                                         # absmax an exact power of two
    x2[1, np.arange(32) != 5] *= 0.5
    x2[2, 7] = -np.float32(np.nextafter(np.float32(8.0), np.float32(0.0))) if dt == 'f32' else -7.96875      # just below one
    x2[3] *= 2.0 ** -40
    x2[4] *= 2.0 ** 30
    q = quantizer(bit, 'per_group', 32, sem='ocp', scale_format='e8m0')
    want = O.run(x2, dt, bit, 'ocp', 'e8m0')
    assert want['scales'][0, 0] == 127 and want['scales'][1, 0] == 127 + 2 - O.EMAX[bit] and want['scales'][2, 0] == want['scales'][1, 0]
    xg = to_gpu(x2, dt).reshape(8, 96)
    codes, s = q._run(q.reshape_tensor(xg), False)
    fake, s2 = q._run(q.reshape_tensor(xg), True)
    assert s.dtype == torch.uint8 and torch.equal(s, s2)
    assert np.array_equal(s.cpu().numpy().reshape(-1), want['scales'].reshape(-1))
    assert np.array_equal(codes.cpu().numpy(), want['codes'])
    assert np.array_equal(bits_of(fake), want_bits(want['fake'], dt))
    lv = np.unique(np.abs(O.decode(codes.cpu().numpy(), bit)))
    assert lv.max() == O.FORMATS[bit][2]                   # the OCP maximum is reached: 6 / 28, not qtorch's 3 / 14
    # given e8m0 scales reproduce the block
    fake3 = q.fake_quant_weight_static(xg, dict(scales=s, zeros=torch.tensor(0.0), qmax=q.qmax, qmin=q.qmin))
    assert torch.equal(fake3.reshape(-1).view(torch.uint8), fake.reshape(-1).view(torch.uint8))


# ---- 7. AWQ end to end ------------------------------------------------------------------------------------------------------
def run_awq(two_call):
    import json
    import os

    import llmc_amd.compression.quantization as Q
    from llmc_amd.compression.quantization import awq_ops
    from toy_model import ToyModel, calib_input
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_quant_configs.json')) as f:
        quant = json.load(f)['methods/FP_Quant/awq_we2m1a16_g128.yml']['quant']
    quant = copy.deepcopy(quant)
    quant['special'].update(save_scale=True, scale_path='/tmp/llmc_fp4_awq_scales')
    model = ToyModel(hidden=256, inner=384, n_blocks=2)
    inp = calib_input(model, n_seq=4, seq=64)
    inp1 = {'data': [torch.cat(inp['data'], dim=0)], 'kwargs': [{}]}
    algo = Q.Awq(model, quant, inp1, None, Cfg(calib=Cfg(seq_len=64), model=Cfg(type='Toy')))
    calls = []
    if two_call:
        def two(w0, cols, s0=None):
            calls.append(1)
            return algo.wquantizer.fake_quant_weight_dynamic(awq_ops.mul_cols_(w0.clone(), cols))
        algo._fake_quantize_weight = two
    else:
        fused = algo.wquantizer._run

        def counting(*a, **k):
            if k.get('cols') is not None:
                calls.append(1)
            return fused(*a, **k)
        algo.wquantizer._run = counting
    algo.run_block_loop()
    assert calls                                           # the route under test ran
    pre = [m.weight.data.clone() for b in model.get_blocks() for m in (b.gate_proj, b.up_proj, b.down_proj)]
    scales = {k: v.clone() for k, v in algo.act_scales.items()}
    algo.deploy('fake_quant')
    post = [m.weight.data.clone() for b in model.get_blocks() for m in (b.gate_proj, b.up_proj, b.down_proj)]
    return pre, scales, post


def test_awq_with_the_shipped_fp4_section_fused_equals_two_calls():
    pre_a, sc_a, post_a = run_awq(False)
    pre_b, sc_b, post_b = run_awq(True)
    assert sc_a.keys() == sc_b.keys() and len(sc_a) >= 2
    for k in sc_a:
        assert torch.equal(sc_a[k].view(torch.int16), sc_b[k].view(torch.int16)), k
    assert len(post_a) == 6
    for a, b in zip(pre_a + post_a, pre_b + post_b):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    # the deployed weights are the oracle's fake-quant of the transformed ones: value / group scale on the 11-level grid
    for w0, w1 in zip(pre_a, post_a):
        want = O.run(w0.float().cpu().numpy().reshape(-1, 128), 'bf16', 'e2m1')
        assert set(np.unique(want['values']).tolist()) <= {-3.0, -2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0}
        assert np.array_equal(bits_of(w1).reshape(-1, 128), want_bits(want['fake'], 'bf16'))
