"""The shared quantizer kernels (quant_kernels.hip, fp8_quant.hip, fp8_block.hip) at model shapes, on every dispatch branch.

The goldens stop at 24 x 512 (integer), 24 x 160 (FP8) and 200 x 384 (FP8 per_block). The host entry points pick a kernel from
the shape, the dtype and the alignment; each case below asserts the branch it was written for, with the host's own predicates
(`small_ok`, `use_two_stage`, `vec_ok`, restated here), so a change of the dispatch cannot move a case off its branch quietly.

A  IntegerQuantizer dynamic (llmc_quant_dynamic / llmc_minmax_qparams):
   small   k_quant_dynamic_small: g = lpr * V16 with lpr a power of two <= 64 (g <= 512 for 16-bit types, <= 256 for fp32);
           per_group 32 / 128 / 256 at 4096 x 4096, per_group 128 at 14336 x 4096 (several grid-stride passes of kMaxGrid)
   vector  k_quant_rows<V16>: fp32 per_group 512; per_channel rows of 11008 / 14336 / 28672 (lpr = 64); per_group 96
   scalar  k_quant_rows<1>: a view one element into its storage; per_channel K = 4100 (K % V16 != 0)
   tails   of both (a few rows, whole tensor compared): G no multiple of the 64 / lpr rows of a wave (sub-groups past the last
           row), lpr rounded up to a power of two (a lane that owns no vector of its row), a second stride that only some lanes
           take (5 x 520, 3 x 37)
   two     k_minmax_partial + k_minmax_final + k_quant_static (g >= 32768 and G < 4096): per_tensor 14336 x 4096,
           per_channel 1024 x 32776 (partial last chunk), 1024 x 32771 (scalar loads); 4096 x 32768 is the G = 4096 boundary
   every case also through get_tensor_qparams (llmc_minmax_qparams: k_quant_rows_qparams, quant_rows without its second
   pass, or the branch's own)
   per_tensor asymmetric: _per_tensor_asym_qparams + k_quant_static with SCALAR_QPARAM;  activations per_token / per_tensor
B  k_quant_static with given qparams: fp32 scales on 16-bit weights, integer zeros, 0-dim scale / zero (SCALAR_QPARAM),
   round_zp=False (FRACTIONAL_ZP), vector and scalar (unaligned) kernels
C  calib_algo 'mse' (k_mse_qparams) on sampled rows: rows with the oracle's range are bit-identical, >= 97 % of them agree
D  FloatQuantizer (k_fp8_cast): the packed 16-bit qtorch path (bf16, e4m3, codes), the division-free float form (fp8_fast8) with
   inputs planted on every guard, the general encoder (e5m2, fp32, promoted dtypes, vectors that fail a guard), the scalar loop
E  FP8 per_block (k_fp8_block_quant*) and weight_cast_to_fp8 / weight_cast_to_bf16 (k_fp8_block_dequant8 / k_fp8_block_dequant)
F  pack_lsb (k_pack_lsb) and pack_awq_gemm (k_pack_awq_w / k_pack_awq_z)

References: oracle/quant_ref.py, bit for bit (section C: on the rows whose searched range agrees). Where a scale is shared by a
whole tensor of a 16-bit dtype, the reference is evaluated once per bit pattern (65536 values) and looked up: the result of an
elementwise map of one 16-bit input is a function of its pattern, so this is the oracle's value for every element."""
import functools

import numpy as np
import pytest
import torch

from conftest import report
from oracle import quant_ref as Q

pytestmark = pytest.mark.gpu

TD = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}
V16 = {'f16': 8, 'bf16': 8, 'f32': 4}      # elements per 16-B vector
K_CHUNK = 8192                              # kChunk (quant_kernels.hip)
K_MAX_GRID = 2048                           # kMaxGrid
UNR = 4                                     # row sets per wave turn of k_quant_dynamic_small
FMAX = {'e4m3': 448.0, 'e5m2': 57344.0}


# ---- the host's dispatch predicates (quant_kernels.hip, fp8_quant.hip, fp8_block.hip) ---------------------------------------
def small_ok(g, vec):
    lpr = g // vec
    return g % vec == 0 and 1 <= lpr <= 64 and (lpr & (lpr - 1)) == 0


def use_two_stage(G, g):
    return g >= 4 * K_CHUNK and G < 4096


def vec_ok(t, g, dt):
    return g % V16[dt] == 0 and t.data_ptr() % 16 == 0


def dynamic_branch(t, G, g, dt):
    """quant_dynamic_tk / llmc_quant_dynamic for a contiguous [G, g] view (outputs are fresh, 16-B aligned allocations)"""
    if use_two_stage(G, g):
        return 'two_stage' if vec_ok(t, g, dt) else 'two_stage_scalar'
    if vec_ok(t, g, dt):
        return 'small' if small_ok(g, V16[dt]) else 'vector'
    return 'scalar'


def small_passes(G, g, dt):
    """grid-stride turns of k_quant_dynamic_small"""
    rpw = 64 // (g // V16[dt])
    blocks = min(K_MAX_GRID, max(1, -(-(-(-G // (rpw * UNR))) // 4)))
    return -(-G // (blocks * 4 * rpw * UNR))


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def host(t):
    return t.detach().float().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def eq_bits(a, b, tag):
    a, b = bits(a), bits(b)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        i = tuple(bad[0])
        raise AssertionError(f'{tag}: {len(bad)} of {a.size} differ, first at {i}: '
                             f'{a[i]:#010x} ({a.view(np.float32)[i]!r}) vs {b[i]:#010x} ({b.view(np.float32)[i]!r})')


def eq_fake8(a, b, tag):
    """eq_bits for FP8 fake values, except that any NaN equals any NaN: the oracle decodes both NaN codes (0x7f, 0xff) to +NaN,
    torch's decoder and the kernels keep the code's sign (the codes themselves are compared bit for bit)"""
    a, b = np.array(a, dtype=np.float32), np.array(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        i = tuple(np.argwhere(na != nb)[0])
        raise AssertionError(f'{tag}: NaN in different places, first at {i}: {a[i]!r} vs {b[i]!r}')
    a[na] = 0.0
    b[nb] = 0.0
    eq_bits(a, b, tag)


def eq_int(a, b, tag):
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        i = tuple(bad[0])
        raise AssertionError(f'{tag}: {len(bad)} of {a.size} differ, first at {i}: {a[i]} vs {b[i]}')


@functools.lru_cache(maxsize=2)
def _base(R, K, seed):
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(R, K, generator=gen) * 0.02
    w[:, ::97] *= 20
    return w


def cpu_weights(R, K, seed):
    """seeded fp32 weights with outlier columns (every 97th x 20), as the model-shaped tests use"""
    return _base(R, K, seed).clone()


def to_dt(w, dt):
    """fp32 torch -> dt torch and its exact fp32 numpy image"""
    t = w.to(TD[dt])
    return t, t.float().numpy()


def sample_rows(R, n, seed, must=()):
    rng = np.random.default_rng(seed)
    r = rng.choice(R, size=min(n, R), replace=False)
    return np.unique(np.concatenate([r, np.asarray([m % R for m in must], dtype=np.int64)]))


def patterns16(dt):
    """every finite value of a 16-bit dtype, as fp32"""
    u = np.arange(65536, dtype=np.uint32)
    v = (u << 16).view(np.float32) if dt == 'bf16' else u.astype(np.uint16).view(np.float16).astype(np.float32)
    return v[np.isfinite(v)]


def lut16(wt, dt, fn):
    """fn (elementwise on fp32 numpy) applied to every element of the 16-bit tensor wt, through a table of its 65536 patterns"""
    u = np.arange(65536, dtype=np.uint32)
    v = (u << 16).view(np.float32) if dt == 'bf16' else u.astype(np.uint16).view(np.float16).astype(np.float32)
    table = fn(v)
    idx = wt.contiguous().view(torch.int16).numpy().astype(np.int64) & 0xffff
    return table[idx]


# =============================================================================================================================
# A. IntegerQuantizer, dynamic
def plant_int(w, gw, bit, sym):
    """edge groups in the fp32 weight w (modified in place), gw = width of a quantization group (<= K), groups counted over the
    flat tensor: 0 all zero (scale from the 1e-5 clamp), 1 constant, 2 negative only, 3 and the last group: quotients that are
    exact .5 ties for s = 2^-6 (round half even; asymmetric: the zero point rint(-1.5) too), with the codes qmin / qmax reached
    exactly; 4: the group's extreme in its last element (the last chunk of a long row)"""
    qmin, qmax = Q.int_range(bit, sym)
    f = w.view(-1)
    s0 = 2.0 ** -6
    G = f.numel() // gw                      # a tensor of fewer than 5 groups gets the groups it has
    f[0:gw] = 0.0
    if G > 1:
        f[gw:2 * gw] = 0.0123
    if G > 2:
        f[2 * gw:3 * gw] = -f[2 * gw:3 * gw].abs() - 1e-3
    if sym:
        pat = [(m + 0.5) * s0 for m in range(int(qmin), int(qmax))]
        head = [qmax * s0, -qmax * s0]
    else:
        mn = -1.5 * s0
        pat = [mn + m * s0 for m in range(int(qmax - qmin) + 1)]
        head = [mn, mn + (qmax - qmin) * s0]
    vals = torch.tensor(head + pat * (-(-gw // len(pat))), dtype=torch.float32)[:gw]
    for gi in (3, G - 1):
        if gi < G:
            f[gi * gw:(gi + 1) * gw] = vals
    if G > 4:
        f[4 * gw + gw - 1] = 1.5 * f[4 * gw:5 * gw].abs().max() + 0.05
    return w


def int_quantizer(bit, sym, gran, g, **kw):
    from llmc_amd.compression.quantization import IntegerQuantizer
    if gran == 'per_group':
        kw['group_size'] = g
    return IntegerQuantizer(bit, sym, gran, **kw)


def int_reference(w2, dt, bit, sym, s=None, z=None):
    """(fake, codes, scales, zeros) of the oracle on the [G, g] rows w2 (qparams given for per_tensor)"""
    qmin, qmax = Q.int_range(bit, sym)
    if s is None:
        s, z = Q.minmax_qparams(w2, dt, sym, qmin, qmax)
    fake = Q.fake_quant_static(w2, dt, s, dt, z, dt, qmin, qmax)
    codes, _ = Q.quant_codes(w2, dt, s, dt, z, dt, qmin, qmax)
    return fake, codes.astype(np.int32), s, z


def code_dtype(bit, sym):
    return torch.int32 if bit != 8 else (torch.int8 if sym else torch.uint8)


# (id, dtype, R, K, granularity, group, bits, sym, branch)
A_CASES = [
    ('small_g32', 'bf16', 4096, 4096, 'per_group', 32, 2, False, 'small'),
    ('small_g32', 'f16', 4096, 4096, 'per_group', 32, 3, True, 'small'),
    ('small_g32', 'f32', 4096, 4096, 'per_group', 32, 4, False, 'small'),
    ('small_g128', 'bf16', 4096, 4096, 'per_group', 128, 4, False, 'small'),
    ('small_g128', 'f16', 4096, 4096, 'per_group', 128, 8, True, 'small'),
    ('small_g128', 'f32', 4096, 4096, 'per_group', 128, 3, False, 'small'),
    ('small_g256', 'bf16', 4096, 4096, 'per_group', 256, 8, False, 'small'),
    ('small_g256', 'f16', 4096, 4096, 'per_group', 256, 2, True, 'small'),
    ('small_g256', 'f32', 4096, 4096, 'per_group', 256, 4, True, 'small'),
    ('small_g512', 'bf16', 4096, 4096, 'per_group', 512, 4, True, 'small'),
    ('small_passes', 'bf16', 14336, 4096, 'per_group', 128, 4, False, 'small'),
    ('small_passes', 'f16', 14336, 4096, 'per_group', 128, 4, True, 'small'),
    ('vector_g512', 'f32', 4096, 4096, 'per_group', 512, 4, False, 'vector'),
    ('vector_g512', 'f32', 4096, 4096, 'per_group', 512, 8, True, 'vector'),
    ('vector_rows', 'bf16', 4096, 14336, 'per_channel', 0, 4, False, 'vector'),
    ('vector_rows', 'f16', 1024, 28672, 'per_channel', 0, 8, True, 'vector'),
    ('vector_rows', 'f32', 512, 11008, 'per_channel', 0, 3, False, 'vector'),
    ('vector_rows', 'bf16', 512, 11008, 'per_channel', 0, 8, False, 'vector'),
    ('vector_g96', 'bf16', 1024, 4608, 'per_group', 96, 4, False, 'vector'),
    ('vector_g96', 'f32', 1024, 4608, 'per_group', 96, 2, True, 'vector'),
    ('scalar_k4100', 'f16', 1024, 4100, 'per_channel', 0, 4, False, 'scalar'),
    ('scalar_k4100', 'bf16', 1024, 4100, 'per_channel', 0, 8, True, 'scalar'),
    ('vector_tail_g96', 'bf16', 5, 288, 'per_group', 96, 4, False, 'vector'),       # G = 15, lpr = 16: 4 rows per wave
    ('vector_idle_lane', 'bf16', 9, 24, 'per_channel', 0, 8, True, 'vector'),       # lpr 3 -> 4, 16 rows per wave
    ('vector_tail_lpr8', 'f32', 13, 20, 'per_channel', 0, 8, False, 'vector'),      # lpr 5 -> 8, 8 rows per wave
    ('vector_stride2', 'f16', 5, 520, 'per_channel', 0, 3, True, 'vector'),         # lpr = 64, 65 vectors: lane 0 reloads
    ('scalar_tail_lpr8', 'f16', 13, 5, 'per_channel', 0, 8, True, 'scalar'),        # lpr = 8, 8 rows per wave
    ('scalar_stride2', 'bf16', 3, 37, 'per_channel', 0, 2, False, 'scalar'),        # lpr = 64, a partial stride
    ('two_stage_tensor', 'bf16', 14336, 4096, 'per_tensor', 0, 8, True, 'two_stage'),
    ('two_stage_tensor', 'f16', 14336, 4096, 'per_tensor', 0, 4, True, 'two_stage'),
    ('two_stage_tensor', 'f32', 4096, 4096, 'per_tensor', 0, 3, True, 'two_stage'),
    ('two_stage_rows', 'bf16', 1024, 32776, 'per_channel', 0, 4, False, 'two_stage'),
    ('two_stage_rows', 'f32', 1024, 32776, 'per_channel', 0, 2, True, 'two_stage'),
    ('two_stage_scalar', 'f16', 1024, 32771, 'per_channel', 0, 3, False, 'two_stage_scalar'),
    ('two_stage_scalar', 'bf16', 1024, 32771, 'per_channel', 0, 8, False, 'two_stage_scalar'),
    ('boundary_G4096', 'bf16', 4096, 32768, 'per_channel', 0, 2, False, 'vector'),
]


def _check_int_dynamic(q, wd, wn, dt, bit, sym, gran, g, rows, tag):
    """fake (fake_quant_weight_dynamic), codes / scales / zeros (real_quant_weight_dynamic), scales / zeros alone
    (get_tensor_qparams) on the sampled weight rows"""
    R, K = wn.shape
    qmin, qmax = Q.int_range(bit, sym)
    gw = R * K if gran == 'per_tensor' else (g or K)
    fq = q.fake_quant_weight_dynamic(wd)
    codes, rs, rz = q.real_quant_weight_dynamic(wd)
    assert fq.dtype == TD[dt] and fq.shape == wd.shape, tag
    assert codes.dtype == code_dtype(bit, sym) and codes.shape == wd.shape, tag
    assert rs.dtype == TD[dt] and (rz is None) == sym, tag
    _, qs, qz, _, _ = q.get_tensor_qparams(wd)
    assert qs.dtype == TD[dt] and qs.numel() == rs.numel() and (qz.dim() == 0) == sym, tag
    if gran == 'per_tensor':
        s, z = Q.minmax_qparams(wn.reshape(1, -1), dt, sym, qmin, qmax)
        s, z = s.reshape(()), z.reshape(())
        if dt != 'f32':
            ref_fake = lut16(wd.cpu(), dt, lambda v: Q.fake_quant_static(v, dt, s, dt, z, dt, qmin, qmax))[rows]
            ref_codes = lut16(wd.cpu(), dt, lambda v: Q.quant_codes(v, dt, s, dt, z, dt, qmin, qmax)[0])[rows]
        else:
            ref_fake, ref_codes, _, _ = int_reference(wn[rows], dt, bit, sym, s, z)
        ref_s, ref_z = s.reshape(1), z.reshape(1)
        got_s, got_z = host(rs).reshape(-1), (None if sym else host(rz).reshape(-1))
        got_qs, got_qz = host(qs).reshape(-1), (None if sym else host(qz).reshape(-1))
    else:
        gpr = K // gw
        ref_fake, ref_codes, ref_s, ref_z = int_reference(wn[rows].reshape(-1, gw), dt, bit, sym)
        ref_fake, ref_codes = ref_fake.reshape(len(rows), K), ref_codes.reshape(len(rows), K)
        got_s = host(rs).reshape(R, gpr)[rows].reshape(-1)
        got_z = None if sym else host(rz).reshape(R, gpr)[rows].reshape(-1)
        got_qs = host(qs).reshape(R, gpr)[rows].reshape(-1)
        got_qz = None if sym else host(qz).reshape(R, gpr)[rows].reshape(-1)
    eq_bits(host(fq[torch.from_numpy(rows).cuda()]), ref_fake, tag + ' fake')
    eq_int(codes[torch.from_numpy(rows).cuda()].cpu().numpy(), ref_codes, tag + ' codes')
    eq_bits(got_s, ref_s.reshape(-1), tag + ' scales')
    eq_bits(got_qs, ref_s.reshape(-1), tag + ' qparams scales')
    if not sym:
        eq_bits(got_z, ref_z.reshape(-1), tag + ' zeros')
        eq_bits(got_qz, ref_z.reshape(-1), tag + ' qparams zeros')


@pytest.mark.parametrize('case', A_CASES, ids=[f'{c[0]}-{c[1]}-{c[2]}x{c[3]}-b{c[6]}{"s" if c[7] else "a"}' for c in A_CASES])
def test_dynamic_integer_quantizer(case):
    name, dt, R, K, gran, g, bit, sym, branch = case
    gw = g or K
    G, gg = (1, R * K) if gran == 'per_tensor' else (R * K // gw, gw)
    w = cpu_weights(R, K, R + K + bit)
    if gran != 'per_tensor':
        plant_int(w, gw, bit, sym)
    else:                               # ties for the tensor's own scale s0: its largest |w| is qmax * s0, in the last element
        qmin, qmax = Q.int_range(bit, sym)
        s0 = 2.0 ** int(np.ceil(np.log2(3.0 / qmax)))
        w[2, :int(qmax - qmin) - 1] = torch.tensor([(m + 0.5) * s0 for m in range(int(qmin) + 1, int(qmax))], dtype=torch.float32)
        w[3, :64] = 0.0
        w[-1, -1] = qmax * s0
        assert float(w.abs().max()) == qmax * s0
    wt, wn = to_dt(w, dt)
    wd = wt.cuda()
    assert dynamic_branch(wd, G, gg, dt) == branch, (name, dynamic_branch(wd, G, gg, dt))
    if name == 'small_passes':
        assert small_passes(G, gg, dt) > 1
    if name.startswith('two_stage_rows'):
        assert gg % K_CHUNK != 0            # a partial last chunk
    q = int_quantizer(bit, sym, gran, g)
    rows = sample_rows(R, 1024, R + K, must=(0, 1, 2, 3, 4, 5, 6, 7, R - 2, R - 1))
    _check_int_dynamic(q, wd, wn, dt, bit, sym, gran, g, rows, f'{name} {dt} {R}x{K} b{bit} sym={sym}')


@pytest.mark.parametrize('dt,bit', [('bf16', 4), ('f16', 8), ('f32', 2)])
def test_dynamic_integer_quantizer_unaligned_view(dt, bit):
    """a contiguous view one element into its storage: the scalar k_quant_rows (per_group 128 at 1024 x 4096)"""
    R, K, g = 1024, 4096, 128
    for sym in (False, True):
        w = plant_int(cpu_weights(R, K, 77 + bit), g, bit, sym)
        wt, wn = to_dt(w, dt)
        flat = torch.empty(R * K + 8, dtype=TD[dt], device='cuda')
        wd = flat[1:1 + R * K].view(R, K)
        wd.copy_(wt.cuda())
        assert dynamic_branch(wd, R * K // g, g, dt) == 'scalar'
        q = int_quantizer(bit, sym, 'per_group', g)
        _check_int_dynamic(q, wd, wn, dt, bit, sym, 'per_group', g, np.arange(R), f'unaligned {dt} b{bit} sym={sym}')


@pytest.mark.parametrize('dt,bit', [('bf16', 4), ('f16', 8), ('bf16', 2)])
def test_per_tensor_asymmetric(dt, bit):
    """_per_tensor_asym_qparams (0-dim fp32 qparams) + k_quant_static with SCALAR_QPARAM at 14336 x 4096"""
    from llmc_amd.compression.quantization import IntegerQuantizer
    R, K = 14336, 4096
    qmin, qmax = Q.int_range(bit, False)
    w = cpu_weights(R, K, 31 + bit)
    w[-1, -1] = 3.0
    w[0, 0] = -1.0
    wt, wn = to_dt(w, dt)
    wd = wt.cuda()
    assert vec_ok(wd, R * K, dt)
    q = IntegerQuantizer(bit, False, 'per_tensor')
    fq = q.fake_quant_weight_dynamic(wd)
    codes, rs, rz = q.real_quant_weight_dynamic(wd)
    s, z = Q.per_tensor_asym_qparams(wn, dt, qmin, qmax)

    ref_fake = lut16(wt, dt, lambda v: _pt_asym(v, dt, s, z, qmin, qmax)[0])
    ref_codes = lut16(wt, dt, lambda v: _pt_asym(v, dt, s, z, qmin, qmax)[1])
    # the restatement above is the oracle's per_tensor_asym_fake_and_codes with the tensor's qparams: pinned on sampled rows
    rows = sample_rows(R, 64, bit, must=(0, R - 1))
    sub = np.concatenate([wn[rows].reshape(-1), [wn.min(), wn.max()]])
    f2, c2, s2, z2 = Q.per_tensor_asym_fake_and_codes(sub, dt, qmin, qmax)
    assert s2 == s and z2 == z
    eq_bits(f2[:-2], ref_fake[rows].reshape(-1), 'restatement')
    tag = f'per_tensor asym {dt} b{bit}'
    eq_bits(host(fq), ref_fake, tag + ' fake')
    eq_int(codes.cpu().numpy(), ref_codes, tag + ' codes')
    assert rs.dtype == torch.float32 and rs.numel() == 1 and rz.numel() == 1
    eq_bits(host(rs).reshape(-1), np.float32([s]), tag + ' scale')
    eq_bits(host(rz).reshape(-1), np.float32([z]), tag + ' zero')


def _pt_asym(v, dt, s, z, qmin, qmax):
    """oracle/quant_ref.py:per_tensor_asym_fake_and_codes after its qparams: 0-dim fp32 s / z, every op rounded to dt"""
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        t = Q.rnd(v / s, dt)
        t = Q.rnd(np.rint(t), dt)
        t = Q.rnd(t + z, dt)
        codes = np.minimum(np.maximum(t, np.float32(qmin)), np.float32(qmax))
        fake = Q.rnd(Q.rnd(codes - z, dt) * s, dt)
    return fake.astype(np.float32), codes.astype(np.int32)


@pytest.mark.parametrize('gran,shape,sym', [('per_token', (4, 2048, 4096), True), ('per_token', (4, 2048, 4096), False),
                                            ('per_tensor', (2, 2048, 14336), True)])
def test_dynamic_activations(gran, shape, sym):
    """fake_quant_act_dynamic, bf16 8 bit: per_token rows of 4096 (small kernel would need g <= 512: vector kernel, lpr = 64),
    per_tensor over 58.7 M elements (two-stage)"""
    from llmc_amd.compression.quantization import IntegerQuantizer
    dt, bit = 'bf16', 8
    qmin, qmax = Q.int_range(bit, sym)
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=gen) * torch.exp(torch.randn(shape[-1], generator=gen))
    x.view(-1, shape[-1])[5, :] = 0.0
    x.view(-1)[-1] = 40.0
    xt, xn = to_dt(x, dt)
    xd = xt.cuda()
    N, K = xn.size // shape[-1], shape[-1]
    G, g = (1, xn.size) if gran == 'per_tensor' else (N, K)
    assert dynamic_branch(xd, G, g, dt) == ('two_stage' if gran == 'per_tensor' else 'vector')
    q = IntegerQuantizer(bit, sym, gran)
    out = q.fake_quant_act_dynamic(xd)
    assert out.shape == xd.shape and out.dtype == xd.dtype
    x2 = xn.reshape(N, K)
    if gran == 'per_tensor':
        s, z = Q.minmax_qparams(xn.reshape(1, -1), dt, sym, qmin, qmax)
        ref = lut16(xt, dt, lambda v: Q.fake_quant_static(v, dt, s.reshape(()), dt, z.reshape(()), dt, qmin, qmax))
        eq_bits(host(out), ref, 'act per_tensor')
        return
    rows = sample_rows(N, 1024, 3, must=(5, N - 1))
    ref, _, _, _ = int_reference(x2[rows], dt, bit, sym)
    eq_bits(host(out).reshape(N, K)[rows], ref, f'act {gran} sym={sym}')


# =============================================================================================================================
# B. k_quant_static with given qparams
def static_reference(w2, wdt, s, sdt, z, zdt, qmin, qmax, fractional=False):
    """fake values and codes of quant.py:699-717 (round_zp=False: round(x / s.clamp_min(1e-9) + z), quant.py:702-707)"""
    if not fractional:
        fake = Q.fake_quant_static(w2, wdt, s, sdt, z, zdt, qmin, qmax)
        codes, _ = Q.quant_codes(w2, wdt, s, sdt, z, zdt, qmin, qmax)
        return fake, codes
    p1 = Q.promote(wdt, sdt)
    p2 = Q.promote(p1, zdt) if zdt is not None else p1
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        sd = np.maximum(s, Q.rnd(np.float32(1e-9), sdt))
        t = Q.rnd(w2 / sd, p1)
        t = Q.rnd(t + z, p2)
        codes = np.minimum(np.maximum(np.rint(t), np.float32(qmin)), np.float32(qmax))
    return Q.rnd(Q.dequant(codes, s, z, p2), wdt), codes


# (id, wdt, gran, bits, sym, scale kind, zero kind, round_zp, unaligned)
#  scale kind: 'f32' [G,1] fp32 | 'dt' [G,1] in the weight dtype | 'scalar' 0-dim fp32;  zero kind: 'int' int32 [G,1] | 'dt' |
#  'f32' | 'scalar' 0-dim fp32 | 'none' (torch.tensor(0.0), symmetric)
B_CASES = [
    ('f32_scales_int_zeros', 'bf16', 'per_group', 4, False, 'f32', 'int', True, False),
    ('f32_scales_int_zeros', 'f16', 'per_channel', 4, False, 'f32', 'int', True, False),
    ('f32_scales_sym', 'f16', 'per_channel', 8, True, 'f32', 'none', True, False),
    ('dt_scales_int_zeros', 'bf16', 'per_channel', 3, False, 'dt', 'int', True, False),
    ('scalar_qparams', 'bf16', 'per_channel', 4, False, 'scalar', 'scalar', True, False),
    ('scalar_qparams', 'f16', 'per_group', 8, True, 'scalar', 'none', True, False),
    ('fractional_zp', 'f16', 'per_group', 4, False, 'dt', 'dt', False, False),
    ('fractional_zp', 'bf16', 'per_channel', 4, False, 'f32', 'f32', False, False),
    ('scalar_kernel', 'bf16', 'per_group', 4, False, 'dt', 'dt', True, True),
    ('scalar_kernel', 'f32', 'per_channel', 3, False, 'f32', 'f32', False, True),
    ('scalar_kernel', 'f16', 'per_group', 8, True, 'f32', 'none', True, True),
]


@pytest.mark.parametrize('case', B_CASES, ids=[f'{c[0]}-{c[1]}-{c[2]}-b{c[3]}' for c in B_CASES])
def test_static_integer_quantizer(case):
    name, dt, gran, bit, sym, skind, zkind, round_zp, unaligned = case
    R, K, g = 4096, 4096, 128
    gw = g if gran == 'per_group' else K
    qmin, qmax = Q.int_range(bit, sym)
    w = plant_int(cpu_weights(R, K, 11 + bit), gw, bit, sym)
    wt, wn = to_dt(w, dt)
    w2 = wn.reshape(-1, gw)
    G = w2.shape[0]
    # qparams of the weight in the scale dtype (fp32 ranges for fp32 scales), then given to the static path
    sdt = {'f32': 'f32', 'dt': dt, 'scalar': 'f32'}[skind]
    s, z = Q.minmax_qparams(w2, sdt, sym, qmin, qmax, round_zp=round_zp)
    if skind == 'scalar':
        s = np.full_like(s, s.max())
        if not sym:
            z = np.full_like(z, np.float32(qmin) - np.rint(w2.min() / s[0, 0]))
    if zkind == 'int':
        z = np.rint(z)
    st = torch.from_numpy(s).to(TD[sdt])
    s_arg = torch.tensor(float(s[0, 0]), dtype=torch.float32) if skind == 'scalar' else st
    zdt = {'int': sdt, 'dt': dt, 'f32': 'f32', 'scalar': dt, 'none': None}[zkind]
    if zkind == 'none':
        z_arg, z_ref = torch.tensor(0.0), None
    elif zkind == 'scalar':
        z_arg, z_ref = torch.tensor(float(z[0, 0]), dtype=torch.float32), z
    elif zkind == 'int':
        z_arg, z_ref = torch.from_numpy(z.astype(np.int32)), z
    else:
        z_arg = torch.from_numpy(z).to(TD[zdt])
        z_ref = z_arg.float().numpy()
    s_ref = s_arg.float().numpy().reshape(-1, 1) if skind != 'scalar' else np.float32(s[0, 0])
    # 0-dim operands keep their fp32 value but do not promote the tensor (the reference's type promotion)
    ref_sdt = dt if skind == 'scalar' else sdt
    rows = sample_rows(R, 1024, bit, must=(0, 1, 2, R - 1))     # weight rows; the groups of a row are its K / gw rows of w2

    def sel(a):
        return a.reshape(R, -1)[rows].reshape(-1, 1) if np.ndim(a) and np.size(a) == G else a

    ref_fake, ref_codes = static_reference(wn[rows].reshape(-1, gw), dt, sel(s_ref), ref_sdt, sel(z_ref), zdt, qmin, qmax,
                                           fractional=not round_zp)
    ref_fake, ref_codes = ref_fake.reshape(-1, K), ref_codes.reshape(-1, K)
    wd = wt.cuda()
    if unaligned:
        flat = torch.empty(R * K + 8, dtype=TD[dt], device='cuda')
        wd = flat[1:1 + R * K].view(R, K)
        wd.copy_(wt.cuda())
    assert vec_ok(wd, gw, dt) == (not unaligned)
    q = int_quantizer(bit, sym, gran, g, round_zp=round_zp)
    shp = (R, K // gw) if gran == 'per_group' else (R, 1)
    args = {'scales': s_arg.cuda() if skind == 'scalar' else st.reshape(shp).cuda(),
            'zeros': z_arg.cuda() if z_arg.dim() == 0 and zkind == 'scalar' else
            (z_arg if zkind == 'none' else z_arg.reshape(shp).cuda()),
            'qmax': torch.tensor(qmax), 'qmin': torch.tensor(qmin)}
    tag = f'static {name} {dt} {gran} b{bit}'
    fq = q.fake_quant_weight_static(wd, dict(args))
    assert fq.dtype == TD[dt]
    eq_bits(host(fq)[rows], ref_fake, tag + ' fake')
    if skind == 'scalar':
        # real_quant_weight_static views the scales as (rows, -1) (quant.py:890-912): a 0-dim scale reaches the codes through
        # quant(), integer values in the promoted float dtype
        t = q.reshape_tensor(wd)
        codes = q.quant(t, args['scales'], args['zeros'], args['qmax'], args['qmin']).reshape(R, K)
        assert codes.dtype == torch.promote_types(TD[dt], torch.float32)
    else:
        codes, _, _ = q.real_quant_weight_static(wd, dict(args))
        assert codes.dtype == code_dtype(bit, sym)
    eq_int(codes.cpu().numpy()[rows], ref_codes, tag + ' codes')
    if gran == 'per_channel' and not unaligned:      # the same arithmetic on a [2, 2048, 4096] activation (per_token rows)
        a = wd.reshape(2, 2048, K)
        qa = int_quantizer(bit, sym, 'per_token', 0, round_zp=round_zp)
        aargs = dict(args)
        if aargs['scales'].dim():
            aargs['scales'] = aargs['scales'].reshape(2, 2048, 1)
        if torch.is_tensor(aargs['zeros']) and aargs['zeros'].dim():
            aargs['zeros'] = aargs['zeros'].reshape(2, 2048, 1)
        fa = qa.fake_quant_act_static(a, aargs)
        eq_bits(host(fa).reshape(R, K)[rows], ref_fake, tag + ' act')


# =============================================================================================================================
# C. calib_algo 'mse'
@pytest.mark.parametrize('dt,R,K,gran,g,bit,sym', [
    ('bf16', 4096, 4096, 'per_channel', 0, 4, False),
    ('f16', 4096, 4096, 'per_channel', 0, 8, True),
    ('bf16', 512, 14336, 'per_channel', 0, 4, True),
    ('f16', 4096, 4096, 'per_group', 128, 4, False),
    ('bf16', 4096, 4096, 'per_group', 128, 4, True),
])
def test_mse_range_search(dt, R, K, gran, g, bit, sym):
    """k_mse_qparams (one wave per row of the [G, g] view, 80 shrink steps) vs Q.mse_range on a seeded sample of rows: rows whose
    searched range equals the oracle's have bit-identical scales, zeros and fake values; >= 97 % of the rows agree (the range is
    a discrete choice decided by fp32 sums of |q - x|^2.4, whose last bits are the implementation's)"""
    from llmc_amd.compression.quantization import IntegerQuantizer
    qmin, qmax = Q.int_range(bit, sym)
    gw = g or K
    w = plant_int(cpu_weights(R, K, 5 * R + bit), gw, bit, sym)
    wt, wn = to_dt(w, dt)
    wd = wt.cuda()
    kw = dict(group_size=g) if g else {}
    q = IntegerQuantizer(bit, sym, gran, calib_algo='mse', **kw)
    t = q.reshape_tensor(wd)
    mn, mx = q.get_tensor_range(t)
    _, s, z, _, _ = q.get_tensor_qparams(wd)
    assert s.dtype == torch.float32 and (sym or z.dtype == torch.float32)
    fq = q.fake_quant_weight_dynamic(wd)
    w2 = wn.reshape(-1, gw)
    G = w2.shape[0]
    n = 256 if g == 0 else 2048
    rows = sample_rows(G, n, G + bit, must=range(0, 5))
    x = w2[rows]
    rmn, rmx = Q.mse_range(x, sym, qmin, qmax)
    same = (host(mn).reshape(-1)[rows] == rmn) & (host(mx).reshape(-1)[rows] == rmx)
    frac = float(same.mean())
    report(f'mse_widths/{dt}/{R}x{K}/{gran}{g or ""}/b{bit}{"s" if sym else "a"}', same_range_fraction=frac, bound=0.97)
    assert frac >= 0.97, frac
    rs, rz = Q.qparams_from_minmax(rmn, rmx, 'f32', sym, qmin, qmax)
    eq_bits(host(s).reshape(-1)[rows][same], rs[same], 'mse scales')
    if not sym:
        eq_bits(host(z).reshape(-1)[rows][same], rz[same], 'mse zeros')
    ref = Q.fake_quant_static(x, dt, rs[:, None], 'f32', None if sym else rz[:, None], None if sym else 'f32', qmin, qmax)
    eq_bits(host(fq).reshape(-1, gw)[rows][same], ref[same], 'mse fake')


# =============================================================================================================================
# D. FloatQuantizer (k_fp8_cast)
def fp8_scale(absmax, dt, sdt, fmt):
    """quant.py:545-553 + 1062: clamp(absmax, 1e-5) / finfo.max in the scales' dtype, a zero scale replaced by 1"""
    a = np.maximum(np.asarray(absmax, dtype=np.float32), Q.rnd(np.float32(1e-5), dt))
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        s = Q.rnd(a / np.float32(FMAX[fmt]), sdt)
    return np.where(s == 0, np.float32(1.0), s).astype(np.float32)


def fp8_rows(x, dt, s, tdt, fmt, sem):
    """float_quant_math.h:float_scaled_exact: t = rnd(rnd(x / s, tdt) + 0, tdt) (tdt: the tensor dtype, promoted by a dimensioned fp32 scale but not by
    a 0-dim one), codes = fp8_encode(t), fake = the fp32 product v * s rounded once to dt"""
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        t = Q.rnd(Q.rnd(x / s, tdt) + np.float32(0.0), tdt)
        b, v = Q.fp8_encode(t, fmt, sem)
        return b, Q.rnd((v * s).astype(np.float32), dt)


def test_fp8_restatement_matches_the_oracle():
    """fp8_scale / fp8_rows (used where the oracle cannot be called as it is: sampled rows of a per-tensor scale, static scales)
    agree with Q.fp8_quant / Q.fp8_fake"""
    gen = np.random.default_rng(0)
    x = (gen.standard_normal((24, 160)) * 0.02).astype(np.float32)
    x[3] = 0.0
    x[4, :5] = [1e-7, -1e-7, 3e-5, 250 * 0.02 / 448, -0.0]
    for dt in ('bf16', 'f16', 'f32'):
        xd = Q.rnd(x, dt)
        for fmt in ('e4m3', 'e5m2'):
            for sem in ('qtorch', 'cast'):
                for w2 in (xd, xd.reshape(1, -1)):
                    b, s, sdt = Q.fp8_quant(w2, dt, fmt, sem)
                    f = Q.fp8_fake(w2, dt, fmt, sem)
                    s2 = fp8_scale(np.abs(w2).max(axis=1, keepdims=True), dt, sdt, fmt)
                    b2, f2 = fp8_rows(w2, dt, s2, dt, fmt, sem)
                    eq_bits(s2, s, 'scale')
                    eq_int(b2, b, f'{dt} {fmt} {sem} codes')
                    eq_bits(f2, f, f'{dt} {fmt} {sem} fake')


def near_tie_values(dt, s, M, tdt=None):
    """values of dt with |x| <= M whose fp32 quotient x / s lies within 4 fp32 ulps of a midpoint of the quotient's dtype"""
    v = patterns16(dt)
    v = v[(np.abs(v) <= M) & (v != 0)]
    with np.errstate(over='ignore', invalid='ignore'):
        qb = (v / np.float32(s)).astype(np.float32).view(np.uint32)
    tdt = tdt or dt
    if tdt == 'bf16':
        d = (qb & 0xffff).astype(np.int64) - 0x8000
    else:
        d = (qb & 0x1fff).astype(np.int64) - 0x1000
        a = (qb & 0x7fffffff).view(np.float32)
        d = np.where((a >= 2.0 ** -14) & (a < 65504), d, 99)
    return v[np.abs(d) <= 4]


def plant_fp8(w, dt, fmt, gran):
    """guard inputs of fp8_fast8 next to ordinary lanes, in the fp32 weight w [R, K] (in place; planted values exact in dt).
    Per row scales: every 32nd element of a planted row is its maximum M, so each group of 32 / 128 and the row share the scale.
    Row 0 all zero; row 1 near-tie quotients (within 4 fp32 ulps of a 16-bit midpoint) for a scale that is not a power of
    two; row 2 the scale 2^-10 with |t| on and beside the subnormal midpoints (k + 1/2) 2^-9, in (240, 448], and -0.0; row 3
    scale 1 with values below the fp16 normal range. per_tensor: the same values for the tensor's scale (its maximum in row 1)."""
    R, K = w.shape
    fm = FMAX[fmt]
    rnd = functools.partial(Q.rnd, dt=dt)
    sub = 2.0 ** -9 if fmt == 'e4m3' else 2.0 ** -16
    tvals = [(k + 0.5) * sub for k in range(8)] + [241.0, 244.0, 247.0, 248.0, 250.0, 255.0, 256.0, 264.0, 300.0, 416.0, 448.0]
    tvals = np.asarray(tvals, dtype=np.float32)
    cols = np.arange(K)
    free = cols[cols % 32 != 0]

    def fill(r, vals, M, every=True):
        base = w[r] * (0.5 * M / float(w[r].abs().max()))
        base[torch.from_numpy(cols[cols % 32 == 0]) if every else 0] = float(M)
        vals = np.asarray(vals, dtype=np.float32)[:len(free)]
        base[torch.from_numpy(free[:len(vals)])] = torch.from_numpy(vals)
        w[r] = base

    def with_ties(M0, sdt):
        """(M, values): M >= M0 in dt whose scale gives near-tie quotients, those first that change the 8-bit code if the quotient
        is rounded from x * (1 / s) (what the guard is for; searched for a while, else plain near ties). The quotient's low bits
        depend on x's significand only, so a scale has a few near ties or none; a bf16 scale has none (a quotient of two 8-bit
        significands is never within 2^-22 of a 9-bit midpoint unless on it, and then one significand would need 9 bits)"""
        if dt == 'f32' or (dt == 'bf16' and sdt != 'f32') or fmt != 'e4m3':     # e5m2 / fp32: no division-free path
            return np.float32(M0), np.zeros(0, np.float32)
        M, first = rnd(np.float32(M0)), None
        for _ in range(256):
            s = fp8_scale(M, dt, sdt, fmt)
            nt = near_tie_values(dt, s, M)
            if len(nt):
                mis = fast_quotient_flips(nt, s)
                if len(mis):
                    return M, np.concatenate([mis, nt[~np.isin(nt, mis)]])
                first = first or (M, nt)
            M = next_up(M)
        assert first is not None, 'no scale with near-tie quotients'
        return first

    def fast_quotient_flips(x, s):
        """x whose code changes when t is rounded from fl32(x * fl32(1 / s)) instead of fl32(x / s)"""
        with np.errstate(all='ignore'):
            t_true = rnd((x / s).astype(np.float32))
            t_fast = rnd((x * (np.float32(1.0) / s)).astype(np.float32))
        d = t_true != t_fast
        flip = np.zeros(d.sum(), bool)
        for sem in ('qtorch', 'cast'):
            flip |= Q.fp8_encode(t_true[d], fmt, sem)[0] != Q.fp8_encode(t_fast[d], fmt, sem)[0]
        return x[d][flip]

    def next_up(M):
        if dt == 'bf16':
            return (np.float32(M).view(np.uint32) + np.uint32(0x10000)).view(np.float32)
        return np.float32(np.nextafter(np.float16(M), np.float16(np.inf)))

    def around(x):
        if dt == 'f32':
            return np.concatenate([x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))])
        lo = rnd(x)
        return np.concatenate([lo, rnd(lo * np.float32(1 + 2.0 ** -7)), rnd(lo * np.float32(1 - 2.0 ** -7))])

    if gran == 'per_tensor':
        M, nt = with_ties(3.0, 'f32')
        s = fp8_scale(M, dt, 'f32', fmt)
        w[0, :K // 2] = 0.0
        fill(1, nt, M, every=False)
        x = around(rnd(np.concatenate([tvals, -tvals]) * s))
        fill(2, np.concatenate([x[np.abs(x) <= M], [-0.0] * 8]), M / 2, every=False)
        w[2, 0] = -0.0
        fill(3, rnd(np.arange(1, 200, dtype=np.float32) * np.float32(2.0 ** -24)), 0.01, every=False)
        return w
    w[0] = 0.0
    M1, nt = with_ties(1.5, dt)
    fill(1, nt, M1)
    M2 = fm * 2.0 ** -10                              # scale exactly 2^-10: t = x * 2^10 without rounding
    x = around((np.concatenate([tvals, -tvals]) * np.float32(2.0 ** -10)).astype(np.float32))
    x = np.concatenate([x, [-0.0] * 8])
    x = x[np.abs(x) <= M2]
    vals = np.empty(len(x) * 2, dtype=np.float32)       # planted lanes alternate with ordinary ones
    vals[0::2] = x
    vals[1::2] = rnd((np.random.default_rng(2).standard_normal(len(x)) * 0.1 * M2).astype(np.float32))
    fill(2, vals, M2)
    fill(3, rnd(np.arange(1, 200, dtype=np.float32) * np.float32(2.0 ** -24)), fm)
    return w


def fp8_quantizer(fmt, gran, sem, g=None):
    from llmc_amd.compression.quantization import FloatQuantizer
    kw = {'per_group': dict(group_size=g), 'per_block': dict(block_size=g)}.get(gran, {})
    return FloatQuantizer(fmt, True, gran, use_qtorch=True, fp8_semantics=sem, **kw)


def fp8_branch(t, g, dt, fmt, sem, fake, G, sdt, no_packed=False):
    """k_fp8_cast's route for a contiguous [G, g] view: 'scalar' loop, 'packed16' (fp8_codes8_bf16_qtorch), 'fast' (fp8_fast8's float
    form, per vector: guards may still send a vector to the general encoder), 'general' (every vector through the general encoder)"""
    if not (g % V16[dt] == 0 and t.data_ptr() % 16 == 0):
        return 'scalar'
    tdt = dt if G == 1 else Q.promote(dt, sdt)
    if V16[dt] != 8 or tdt != dt or fmt != 'e4m3':
        return 'general'
    if dt == 'bf16' and sem == 'qtorch' and not fake and not no_packed:
        return 'packed16'
    return 'fast'


def _fp8_check(wd, wt, wn, dt, fmt, sem, gran, g, rows, tag, static=None, view_shape=None):
    """codes + scales (real_quant_weight_dynamic / _static), fake values (fake_quant_*) of the rows `rows` of the [G, g] view"""
    q = fp8_quantizer(fmt, gran, sem, g)
    x = wd.reshape(view_shape) if view_shape else wd
    R, K = wn.shape
    gw = R * K if gran == 'per_tensor' else (g or K)
    G = R * K // gw
    sdt = 'f32' if gran == 'per_tensor' else dt
    w2 = wn.reshape(G, gw)
    if static is None:
        if view_shape:
            out_f = q.fake_quant_act_dynamic(x)
            bts, s_dev = q._run(q.reshape_tensor(x), False)
            s_dev = s_dev.reshape(-1)
        else:
            out_f = q.fake_quant_weight_dynamic(x)
            bts, s_dev, _ = q.real_quant_weight_dynamic(x)
            bts = bts.view(torch.uint8)
        s = fp8_scale(np.abs(w2).max(axis=1), dt, sdt, fmt)
        assert s_dev.dtype == TD[sdt]
        eq_bits(host(s_dev).reshape(-1), s, tag + ' scales')
        tdt = dt
    else:
        s_arg, s = static
        sd = 'f32' if s_arg.dtype == torch.float32 else dt
        tdt = dt if G == 1 else Q.promote(dt, sd)
        if view_shape:
            out_f = q.fake_quant_act_static(x, {'scales': s_arg})
        else:
            out_f = q.fake_quant_weight_static(x, {'scales': s_arg})
        bts, _, _ = q.real_quant_weight_static(x.reshape(R, K) if view_shape else x, {'scales': s_arg})
        bts = bts.view(torch.uint8)
    s = np.asarray(s, dtype=np.float32).reshape(-1)
    out_f = host(out_f).reshape(G, gw)
    bts = bts.cpu().numpy().reshape(G, gw)
    if G == 1 and dt != 'f32':
        b_ref = lut16(wt, dt, lambda v: fp8_rows(v, dt, s[0], tdt, fmt, sem)[0]).reshape(1, -1)
        f_ref = lut16(wt, dt, lambda v: fp8_rows(v, dt, s[0], tdt, fmt, sem)[1]).reshape(1, -1)
        eq_int(bts, b_ref, tag + ' codes')
        eq_fake8(out_f, f_ref, tag + ' fake')
        return
    if G == 1:                           # fp32 per_tensor: sampled weight rows under the tensor's scale
        wr = wn[rows]
        b_ref, f_ref = fp8_rows(wr, dt, s[0], tdt, fmt, sem)
        eq_int(bts.reshape(R, K)[rows], b_ref, tag + ' codes')
        eq_fake8(out_f.reshape(R, K)[rows], f_ref, tag + ' fake')
        return
    if static is None and tdt == dt:
        b_ref, _, _ = Q.fp8_quant(w2[rows], dt, fmt, sem)
        f_ref = Q.fp8_fake(w2[rows], dt, fmt, sem)
    else:
        b_ref, f_ref = fp8_rows(w2[rows], dt, s[rows][:, None], tdt, fmt, sem)
    eq_int(bts[rows], b_ref, tag + ' codes')
    eq_fake8(out_f[rows], f_ref, tag + ' fake')


@pytest.mark.parametrize('shape', [(14336, 4096), (4096, 14336), (1024, 4096)])
def test_fp8_configs4_call(shape):
    """BASELINE configs[4]: e4m3, qtorch, real, per_tensor, bf16 (fp8_codes8_bf16_qtorch), full tensor; again with
    fp8_no_packed16 = 1 (fp8_fast8's float form), fake values too"""
    from llmc_amd import _ffi
    R, K = shape
    dt, fmt, sem = 'bf16', 'e4m3', 'qtorch'
    w = plant_fp8(cpu_weights(R, K, R ^ K), dt, fmt, 'per_tensor')
    wt, wn = to_dt(w, dt)
    wd = wt.cuda()
    assert fp8_branch(wd, R * K, dt, fmt, sem, False, 1, 'f32') == 'packed16'
    assert fp8_branch(wd, R * K, dt, fmt, sem, False, 1, 'f32', no_packed=True) == 'fast'
    _fp8_check(wd, wt, wn, dt, fmt, sem, 'per_tensor', 0, None, f'configs[4] {shape}')
    with _ffi.option(fp8_no_packed16=1):
        _fp8_check(wd, wt, wn, dt, fmt, sem, 'per_tensor', 0, None, f'configs[4] {shape} float form')


D_GRANS = [('per_tensor', 0), ('per_channel', 0), ('per_group', 128)]


@pytest.mark.parametrize('gran,g', D_GRANS, ids=[f'{a}{b or ""}' for a, b in D_GRANS])
@pytest.mark.parametrize('sem', ['qtorch', 'cast'])
@pytest.mark.parametrize('fmt', ['e4m3', 'e5m2'])
@pytest.mark.parametrize('dt', ['bf16', 'f16', 'f32'])
def test_fp8_quantizer(dt, fmt, sem, gran, g):
    """4096 x 4096 with the guard inputs planted; dynamic, then static with scales at 1/4 of the dynamic ones (|t| up to 1792:
    NaN codes for the cast, 240 for qtorch), in the weight dtype and (per row) in fp32, which promotes the quotient"""
    R, K = 4096, 4096
    w = plant_fp8(cpu_weights(R, K, 3), dt, fmt, 'per_tensor' if gran == 'per_tensor' else 'rows')
    wt, wn = to_dt(w, dt)
    wd = wt.cuda()
    gw = R * K if gran == 'per_tensor' else (g or K)
    G = R * K // gw
    sdt = 'f32' if gran == 'per_tensor' else dt
    want = 'general' if (dt == 'f32' or fmt == 'e5m2') else 'fast'
    assert fp8_branch(wd, gw, dt, fmt, sem, True, G, sdt) == want
    rows = sample_rows(G, 256 if g == 0 else 4096, G, must=range(0, 8 if g == 0 else 8 * K // g))
    tag = f'{dt} {fmt} {sem} {gran}{g or ""}'
    _fp8_check(wd, wt, wn, dt, fmt, sem, gran, g, rows, tag)
    s = fp8_scale(np.abs(wn.reshape(G, gw)).max(axis=1), dt, sdt, fmt) / np.float32(4.0)
    if gran == 'per_tensor':
        s_arg = torch.tensor(float(s[0]), dtype=torch.float32).cuda()
        _fp8_check(wd, wt, wn, dt, fmt, sem, gran, g, rows, tag + ' static', static=(s_arg, s))
        return
    s_dt = torch.from_numpy(s).to(TD[dt])
    _fp8_check(wd, wt, wn, dt, fmt, sem, gran, g, rows, tag + ' static', static=(s_dt.reshape(G, 1).cuda(), s_dt.float().numpy()))
    if dt != 'f32':
        assert fp8_branch(wd, gw, dt, fmt, sem, True, G, 'f32') == 'general'
        _fp8_check(wd, wt, wn, dt, fmt, sem, gran, g, rows, tag + ' static fp32', static=(torch.from_numpy(s).reshape(G, 1).cuda(), s))


@pytest.mark.parametrize('dt,fmt,sem', [('bf16', 'e4m3', 'qtorch'), ('f16', 'e4m3', 'cast'), ('bf16', 'e5m2', 'qtorch')])
def test_fp8_per_token_and_group32(dt, fmt, sem):
    """per_token on a [4, 2048, 4096] activation (dynamic and static), per_group 32 on a 4096 x 4096 weight"""
    R, K = 8192, 4096
    w = plant_fp8(cpu_weights(R, K, 8), dt, fmt, 'rows')
    wt, wn = to_dt(w, dt)
    wd = wt.cuda()
    rows = sample_rows(R, 256, 9, must=range(0, 8))
    tag = f'{dt} {fmt} {sem} per_token'
    _fp8_check(wd, wt, wn, dt, fmt, sem, 'per_token', 0, rows, tag, view_shape=(4, 2048, K))
    s = fp8_scale(np.abs(wn).max(axis=1), dt, dt, fmt) / np.float32(4.0)
    st = torch.from_numpy(s).to(TD[dt])
    _fp8_check(wd, wt, wn, dt, fmt, sem, 'per_token', 0, rows, tag + ' static', static=(st.reshape(4, 2048, 1).cuda(), st.float().numpy()),
               view_shape=(4, 2048, K))
    w2 = wd[:4096]
    rows = sample_rows(4096 * 128, 8192, 10, must=range(0, 8 * 128))
    _fp8_check(w2, wt[:4096], wn[:4096], dt, fmt, sem, 'per_group', 32, rows, f'{dt} {fmt} {sem} per_group32')


@pytest.mark.parametrize('sem', ['qtorch', 'cast'])
def test_fp8_zero_row_f16_scale_is_one(sem):
    """an all-zero fp16 row: clamp(0, 1e-5) / 448 underflows to 0 in fp16, stored and returned as 1 (float_quant_math.h: float_dynamic_scale)"""
    R, K = 4096, 4096
    w = cpu_weights(R, K, 12)
    w[7] = 0.0
    w[4000] = 0.0
    wt, wn = to_dt(w, 'f16')
    q = fp8_quantizer('e4m3', 'per_channel', sem)
    bts, s, _ = q.real_quant_weight_dynamic(wt.cuda())
    sh = host(s).reshape(-1)
    assert sh[7] == 1.0 and sh[4000] == 1.0
    assert int(bts.view(torch.uint8)[7].max()) == 0
    _fp8_check(wt.cuda(), wt, wn, 'f16', 'e4m3', sem, 'per_channel', 0, sample_rows(R, 64, 1, must=(7, 4000)), 'zero row')


@pytest.mark.parametrize('dt,fmt,sem', [('bf16', 'e4m3', 'qtorch'), ('f16', 'e4m3', 'cast'), ('f32', 'e5m2', 'qtorch')])
def test_fp8_scalar_loop(dt, fmt, sem):
    """k_fp8_cast's scalar loop: per_channel K = 4100 (fp32: 4102, not a whole number of 16-B vectors), and a 4096 x 4096 view
    one element into its storage (per_channel, per_tensor)"""
    R, K = 1024, 4100 if dt != 'f32' else 4102
    w = plant_fp8(cpu_weights(R, K, 13), dt, fmt, 'rows')
    wt, wn = to_dt(w, dt)
    wd = wt.cuda()
    assert fp8_branch(wd, K, dt, fmt, sem, False, R, dt) == 'scalar'
    _fp8_check(wd, wt, wn, dt, fmt, sem, 'per_channel', 0, np.arange(R), f'{dt} K=4100')
    R, K = 4096, 4096
    for gran in ('per_channel', 'per_tensor'):
        w = plant_fp8(cpu_weights(R, K, 14), dt, fmt, 'rows' if gran == 'per_channel' else 'per_tensor')
        wt, wn = to_dt(w, dt)
        flat = torch.empty(R * K + 8, dtype=TD[dt], device='cuda')
        wd = flat[1:1 + R * K].view(R, K)
        wd.copy_(wt.cuda())
        G = 1 if gran == 'per_tensor' else R
        assert fp8_branch(wd, R * K // G, dt, fmt, sem, False, G, 'f32' if G == 1 else dt) == 'scalar'
        _fp8_check(wd, wt, wn, dt, fmt, sem, gran, 0, sample_rows(R, 256, 15, must=range(0, 8)), f'{dt} unaligned {gran}')


# =============================================================================================================================
# E. FP8 per_block and the block casts
@pytest.mark.parametrize('sem', ['qtorch', 'cast'])
@pytest.mark.parametrize('dt,shape', [('bf16', (4096, 14336)), ('bf16', (7168, 2112)), ('f32', (1000, 4100))])
def test_fp8_per_block(dt, shape, sem):
    """FloatQuantizer per_block 128 (real and fake), weight_cast_to_fp8 and weight_cast_to_bf16 vs Q.fp8_per_block.
    7168 x 2112: a ragged last block column; 1000 x 4100 fp32: ragged rows and columns, the unvectorised k_fp8_block_dequant"""
    from llmc_amd.compression.quantization.quant import weight_cast_to_bf16, weight_cast_to_fp8
    M, N = shape
    b = 128
    w = cpu_weights(M, N, M + N)
    w[:128, :128] = 0.0
    w[130, 200] = -5.0
    w[-1, -1] = 7.0
    wt, wn = to_dt(w, dt)
    wd = wt.cuda()
    ref_bits, ref_s, ref_fake = Q.fp8_per_block(wn, dt, b, sem)
    q = fp8_quantizer('e4m3', 'per_block', sem, b)
    tag = f'per_block {dt} {shape} {sem}'
    rw, rs, rz = q.real_quant_weight_dynamic(wd)
    assert rz is None and rs.shape == ref_s.shape
    eq_bits(rs.cpu().numpy(), ref_s, tag + ' scales')
    eq_int(rw.view(torch.uint8).cpu().numpy(), ref_bits, tag + ' codes')
    fk = q.fake_quant_weight_dynamic(wd)
    assert fk.dtype == TD[dt]
    eq_bits(host(fk), ref_fake, tag + ' fake')
    w8, s8 = weight_cast_to_fp8(wd, b, fp8_semantics=sem)
    eq_int(w8.view(torch.uint8).cpu().numpy(), ref_bits, tag + ' cast codes')
    eq_bits(s8.cpu().numpy(), ref_s, tag + ' cast scales')
    back = weight_cast_to_bf16(w8, s8, b)
    assert back.dtype == torch.bfloat16
    vec = N % 8 == 0 and b % 8 == 0
    assert vec == (dt != 'f32')
    dec = torch.from_numpy(ref_bits).view(torch.float8_e4m3fn).float().numpy()
    s_full = np.repeat(np.repeat(ref_s, b, axis=0), b, axis=1)[:M, :N]
    eq_bits(host(back), Q.rnd((dec * s_full).astype(np.float32), 'bf16'), tag + ' cast back')


# =============================================================================================================================
# F. packers
def test_pack_lsb_model_width():
    """8-bit codes from int8 (symmetric) and uint8 (asymmetric) containers, 4-bit int32 codes at K = 4100 (a padded last word)"""
    from llmc_amd.compression.quantization import pack_lsb
    R, K = 4096, 14336
    gen = torch.Generator().manual_seed(21)
    c8 = torch.randint(-128, 128, (R, K), generator=gen, dtype=torch.int32)
    c8[0, :256] = torch.arange(-128, 128, dtype=torch.int32)
    i8 = c8.to(torch.int8)
    eq_int(pack_lsb(i8.cuda(), 8).cpu().numpy(), Q.pack_lsb(i8.numpy(), 8), 'int8 codes')
    u8 = (c8 + 128).to(torch.uint8)
    eq_int(pack_lsb(u8.cuda(), 8).cpu().numpy(), Q.pack_lsb(u8.numpy(), 8), 'uint8 codes')
    eq_int(pack_lsb(c8.cuda(), 8).cpu().numpy(), Q.pack_lsb(c8.numpy(), 8), 'int32 8-bit codes')
    c4 = torch.randint(-8, 8, (R, 4100), generator=gen, dtype=torch.int32)
    p4 = pack_lsb(c4.cuda(), 4)
    assert p4.shape == (R, 513)
    eq_int(p4.cpu().numpy(), Q.pack_lsb(c4.numpy(), 4), '4-bit K=4100')
    c4w = torch.randint(-8, 8, (R, K), generator=gen, dtype=torch.int32)
    eq_int(pack_lsb(c4w.cuda(), 4).cpu().numpy(), Q.pack_lsb(c4w.numpy(), 4), '4-bit K=14336')


def test_pack_awq_gemm_model_width():
    """pack_awq_gemm at 4096 x 14336, g = 128, of an asymmetric 4-bit fake-quantized fp16 weight and its qparams"""
    from llmc_amd.compression.quantization import pack_awq_gemm
    R, K, g = 4096, 14336, 128
    w = cpu_weights(R, K, 22).half().cuda()
    q = int_quantizer(4, False, 'per_group', g)
    fq = q.fake_quant_weight_dynamic(w)
    _, s, z = q.real_quant_weight_dynamic(w)
    s, z = s.reshape(R, K // g), z.reshape(R, K // g).to(torch.int32)
    qw, so, qz = pack_awq_gemm(fq, s, z, g)
    rqw, rs, rqz = Q.pack_awq_gemm(host(fq), host(s), z.cpu().numpy(), g)
    eq_int(qw.cpu().numpy(), rqw, 'qweight')
    eq_bits(host(so), rs, 'scales')
    eq_int(qz.cpu().numpy(), rqz, 'qzeros')
