"""AWQ's reductions and elementwise kernels (awq_kernels.hip; llmc_awq_scale_fakequant on k_quant_rows_scaled / k_quant_dynamic_small
of quant_kernels.hip) at model widths.

The goldens of test_awq_gpu.py stop at K = 256, 96 weight rows and 192 tokens; the branches that only run at real sizes are
pinned here: several 512-token chunks of the activation mean, weight rows wider than one 256-thread column step, whole-row
(per-channel) groups up to K = 28672, more than one strided pass of the single-workgroup scale kernel, the large-group and
the unaligned (scalar) scale + fake-quant kernels, the half-empty last k-tile pair of the k-tiled quotient.
References: oracle/awq_ref.py (fp32 numpy with the per-op rounding to the model dtype), or sums in fp64 on the device
where the order of an fp32 reduction is the implementation's."""
import math

import numpy as np
import pytest
import torch

from oracle import awq_ref as A

pytestmark = pytest.mark.gpu

TD = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}
DTS = ['bf16', 'f16', 'f32']
U32 = 2.0 ** -24            # unit roundoff of fp32
TOK_CHUNK = 512             # tokens per partial sum of llmc_awq_act_mean (awq_kernels.hip)
WS_ROWS = 16                # rows per partial sum of llmc_awq_weight_mean (awq_kernels.hip)


def host(t):
    return t.detach().float().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ulps(a, b, dt):
    """distance in units of the last place of dt, for values that are exact in dt (fp32 carriers)"""
    sh = {'bf16': 16, 'f16': 13, 'f32': 0}[dt]
    a = np.ascontiguousarray(a, dtype=np.float32).ravel().view(np.int32).astype(np.int64) >> sh
    b = np.ascontiguousarray(b, dtype=np.float32).ravel().view(np.int32).astype(np.int64) >> sh
    return np.abs(a - b)


def int_q(bit, sym, g):
    from llmc_amd.compression.quantization import IntegerQuantizer
    if g == 0:
        return IntegerQuantizer(bit, bool(sym), 'per_channel')
    return IntegerQuantizer(bit, bool(sym), 'per_group', group_size=g)


def cpu_weights(R, K, seed, dt):
    """seeded weights with outlier columns (every 97th x 20), as the model-shaped tests use"""
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(R, K, generator=gen) * 0.02
    w[:, ::97] *= 20
    return w.to(TD[dt])


def gpu_acts(N, K, seed, dt):
    """seeded activations made on the device (up to 65536 x 4096): per-column scales exp(N(0, 1)), outlier columns x 20"""
    gen = torch.Generator(device='cuda').manual_seed(seed)
    col = torch.exp(torch.randn(K, generator=gen, device='cuda'))
    col[::97] *= 20
    x = torch.empty(N, K, dtype=TD[dt], device='cuda')
    for t0 in range(0, N, 8192):
        t1 = min(N, t0 + 8192)
        x[t0:t1] = (torch.randn(t1 - t0, K, generator=gen, device='cuda') * col).to(TD[dt])
    return x


def abs_colsum64(x):
    """exact column sums of |x| (fp64 holds every partial sum of these fp32-representable terms to 2^-53)"""
    s = torch.zeros(x.shape[1], dtype=torch.float64, device=x.device)
    for t0 in range(0, x.shape[0], 8192):
        s += x[t0:t0 + 8192].double().abs().sum(0)
    return s


# ---------------------------------------------------------------------------------------------------------------------
# llmc_awq_act_mean: sums of TOK_CHUNK tokens, then the partials in order
@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('N,K', [(511, 4096), (512, 4096), (513, 4096), (4133, 14336), (777, 1032), (65536, 4096)])
def test_act_mean_vs_fp64(dt, N, K):
    from llmc_amd.compression.quantization import awq_ops
    x = gpu_acts(N, K, N + K, dt)
    out = awq_ops.act_mean(x)
    mean64 = abs_colsum64(x) / N
    if dt == 'f32':
        # stage 1 adds at most TOK_CHUNK non-negative terms in sequence (TOK_CHUNK - 1 roundings), stage 2 the nchunk
        # partials (nchunk - 1 roundings), the division rounds once: each rounding is a relative error <= u on a partial
        # sum that never exceeds the final sum, so |out - mean| <= (TOK_CHUNK + nchunk - 1) u mean (first order in u)
        nchunk = math.ceil(N / TOK_CHUNK)
        err = (out.double() - mean64).abs()
        assert bool((err <= (TOK_CHUNK + nchunk) * U32 * mean64).all()), float((err / mean64).max())
        return
    ref = mean64.float().to(TD[dt])
    u = ulps(host(out), host(ref), dt)
    assert u.max() <= 1, u.max()
    assert (u > 0).mean() <= 0.02, (u > 0).mean()


# ---------------------------------------------------------------------------------------------------------------------
# llmc_awq_weight_mean: one layer's mean over rows of |w| / group-max(|w|)
def _weight_mean_ref64(w, g):
    """fp32 quotients (a quotient of two fp32 values rounded to fp64 and then to fp32 is the correctly rounded fp32
    quotient), summed exactly in fp64"""
    R, K = w.shape
    a = w.float().abs().reshape(-1, g or K)
    q = (a.double() / a.amax(1, keepdim=True).double()).float().reshape(R, K)
    return q.double().sum(0) / R


def _check_weight_mean(w, g, dt, tag):
    from llmc_amd.compression.quantization import awq_ops
    out = awq_ops.weight_mean(w, g)
    R, K = w.shape
    if dt == 'f32':
        # the sum over a slab of WS_ROWS rows, then the ceil(R / WS_ROWS) slab partials in order, then one division:
        # as for act_mean, (WS_ROWS + nslab) u relative for these non-negative terms
        ref = _weight_mean_ref64(w, g)
        o = out.double()
        nan = torch.isnan(ref)
        assert torch.equal(torch.isnan(o), nan), tag
        err = (o - ref).abs()[~nan]
        bound = (WS_ROWS + math.ceil(R / WS_ROWS)) * U32 * ref[~nan]
        assert bool((err <= bound).all()), (tag, float((err / ref[~nan]).max()))
        return
    ref = A.weight_scale([host(w)], dt, g)
    o = host(out)
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(o), nan, err_msg=tag)
    u = ulps(o[~nan], ref[~nan], dt)
    assert u.max(initial=0) <= 2, (tag, u.max())


def _wm_groups(K):
    return [32, 64, 128, 0] + ([96] if K % 96 == 0 else [])


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('K', [256, 768, 3072, 4096, 8192, 14336, 28672])
def test_weight_mean_vs_oracle(dt, K):
    """groups of 32, 64, 128 (and 96 where it divides K) and whole rows; 1 row, 17 rows (a partial 16-row slab), 1000"""
    rows = (1, 17, 1000) if K in (768, 4096, 14336, 28672) else (1, 17)
    for R in rows:
        w = cpu_weights(R, K, 7 * K + R, dt).cuda()
        for g in _wm_groups(K):
            _check_weight_mean(w, g, dt, (dt, R, K, g))


@pytest.mark.parametrize('dt', DTS)
def test_weight_mean_4096_rows(dt):
    w = cpu_weights(4096, 4096, 4096, dt).cuda()
    for g in (32, 128, 0):
        _check_weight_mean(w, g, dt, (dt, 4096, 4096, g))


@pytest.mark.parametrize('dt', DTS)
def test_weight_mean_other_group_widths(dt):
    """group widths the quantizer accepts that are not 16 B x a power of two: below one 16-B chunk (4), not a whole number
    of chunks in f32 (6), more groups per row than one LDS tile holds (4, 12), a long group of no power-of-two width (1000)"""
    K = 6000
    w = cpu_weights(33, K, 6000, dt).cuda()
    for g in (4, 6, 12, 24, 1000):
        _check_weight_mean(w, g, dt, (dt, 33, K, g))


@pytest.mark.parametrize('dt', DTS)
def test_weight_mean_zero_group_and_unaligned(dt):
    """an all-zero group divides 0 by 0 in the reference: NaN in exactly its columns (per-channel: the whole row, so every
    column); a weight view 1 element into its storage (not 16-B aligned) takes the scalar kernel"""
    R, K = 17, 4096
    w = cpu_weights(R, K, 99, dt).cuda()
    for g in (32, 64, 128, 0):
        wz = w.clone()
        wz[5, K - (g or K):] = 0
        wz[12, (g or K):2 * (g or K)] = 0
        _check_weight_mean(wz, g, dt, (dt, 'zero group', g))
    base = torch.empty(R * K + 1, dtype=TD[dt], device='cuda')
    wu = base[1:].view(R, K)
    wu.copy_(w)
    assert wu.data_ptr() % 16 != 0
    for g in (64, 0):
        _check_weight_mean(wu, g, dt, (dt, 'unaligned', g))


# ---------------------------------------------------------------------------------------------------------------------
def _pow_near_tie(base, e, dt):
    """elements whose exact base^e (fp64) lies within 2 fp32 ulps of a midpoint between two neighbouring dt values"""
    p = np.power(base.astype(np.float64), np.float64(e))
    f = A.rnd(p.astype(np.float32), dt).astype(np.float64)
    man = {'bf16': 7, 'f16': 10}[dt]
    with np.errstate(divide='ignore'):
        ex = np.floor(np.log2(np.maximum(np.abs(p), 1e-30)))
    sp = np.exp2(ex - man)                           # dt spacing in p's binade
    d = np.abs(np.abs(p - f) - sp / 2)               # distance to the midpoint on p's side of f
    return d <= 2 * np.exp2(ex - 23)


# llmc_awq_scales: one 1024-thread workgroup, strided loop over K, max / min over its 16 waves
@pytest.mark.parametrize('dt', ['bf16', 'f16'])
@pytest.mark.parametrize('K', [1000, 4096, 14336, 28672])
def test_awq_scales_vs_oracle(dt, K):
    from llmc_amd.compression.quantization import awq_ops
    rng = np.random.default_rng(K)
    xm = rng.uniform(0.01, 2.0, K).astype(np.float32)
    wm = rng.uniform(0.1, 0.9, K).astype(np.float32)
    last = (K - 1) // 1024 * 1024                 # first element of the last strided pass
    kmax = last + 70                              # wave 1 of that pass: the largest scale at every ratio and version
    kmin = last + (K - 1 - last) // 64 * 64 + 3   # the last wave that has elements there: exact zeros -> the 1e-4 clamp
    assert kmax // 64 != kmin // 64 and kmin < K
    xm[kmax], wm[kmax] = 50.0, 0.05
    xm[kmin:kmin + 3], wm[kmin:kmin + 3] = 0.0, 1.0
    xm, wm = A.rnd(xm, dt), A.rnd(wm, dt)
    xd, wd = torch.from_numpy(xm).to(TD[dt]).cuda(), torch.from_numpy(wm).to(TD[dt]).cuda()
    for ver in ('v1', 'v2'):
        for n in range(20):
            ratio = n / 20
            ref = A.get_scales(xm, wm, ratio, dt, ver)
            out = host(awq_ops.awq_scales(xd, wd, ratio, ver))
            u = ulps(out, ref, dt)
            # pow() of the device libm against the host's: at most one ulp, rarely ...
            tie = _pow_near_tie(xm, A.rnd(np.float32(ratio), dt), dt)
            if ver == 'v1':
                tie |= _pow_near_tie(wm, A.rnd(np.float32(1.0 - ratio), dt), dt)
            assert u[~tie].max() <= 1 and (u > 0).mean() <= 0.03, (ver, n, u[~tie].max(), (u > 0).mean())
            # ... except where a power lies next to a rounding midpoint of dt: the two fp32 pow() results (each within
            # an fp32 ulp of the exact value) may round to neighbouring dt values there, and x^r / w^(1-r) then moves
            # by up to two ulps
            assert u[tie].max(initial=0) <= 2 and tie.mean() <= 0.01, (ver, n, u[tie].max(initial=0), tie.mean())


# ---------------------------------------------------------------------------------------------------------------------
# llmc_awq_scale_fakequant: fakequant(w * s) per row or group
@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('bit', [3, 4, 8])
def test_scale_fakequant_vs_oracle(dt, bit):
    """per-channel rows of 4096 .. 28672 (k_quant_rows_scaled: quant_rows with the column multiplier), groups of 64 and 128
    (k_quant_dynamic_small with it), and a weight view that is not 16-B aligned (the scalar k_quant_rows_scaled): bit-exact.
    The last three are quant_rows' tails: 15 groups of 96 at 4 per wave (sub-groups past the last row), rows of 3
    vectors on 4 lanes (a lane that owns none), and, through the unaligned view, 13 scalar rows of 40 on 64 lanes"""
    from llmc_amd.compression.quantization import awq_ops
    cases = [(24, 4096, 0), (16, 14336, 0), (8, 28672, 0), (40, 4096, 64), (40, 4096, 128),
             (5, 288, 96), (9, 24, 0), (13, 40, 0)]
    for R, K, g in cases:
        w = cpu_weights(R, K, R * K + bit, dt)
        gen = torch.Generator().manual_seed(K + g)
        s = (torch.rand(K, generator=gen) * 1.5 + 0.25)
        s[::61] *= 6
        s = s.to(TD[dt])
        wn, sn = w.float().numpy(), s.float().numpy()
        wd, sd = w.cuda(), s.cuda()
        for sym in (True, False):
            q = int_q(bit, sym, g)
            ref = A.fake_quantize_weight(wn, sn, dt, sym, float(q.qmin), float(q.qmax), g)
            out = awq_ops.scale_fakequant(wd, sd, q)
            np.testing.assert_array_equal(bits(host(out)), bits(ref), err_msg=str((dt, bit, sym, R, K, g)))
            if g == 0 and K in (4096, 40) or g == 128:
                base = torch.empty(R * K + 1, dtype=TD[dt], device='cuda')
                wu = base[1:].view(R, K)
                wu.copy_(wd)
                assert wu.data_ptr() % 16 != 0
                out = awq_ops.scale_fakequant(wu, sd, q)
                np.testing.assert_array_equal(bits(host(out)), bits(ref), err_msg=str((dt, bit, sym, R, K, g, 'unaligned')))


# ---------------------------------------------------------------------------------------------------------------------
# x / s[col], w * s[col], the k-tiled quotient, per-group clamp
def _col_data(N, K, dt, seed):
    x = gpu_acts(N, K, seed, dt)
    gen = torch.Generator(device='cuda').manual_seed(seed + 1)
    s = (torch.rand(K, generator=gen, device='cuda') * 3 + 0.05)
    s[::61] *= 40
    return x, s.to(TD[dt])


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('K', [4096, 14336])
def test_div_mul_cols_bit_exact(dt, K):
    """the fp32 quotient / product rounded once to dt; the exact value is formed in fp64 (an fp32 quotient or product of
    two fp32 values rounded to fp64 and then to fp32 is the correctly rounded one)"""
    from llmc_amd.compression.quantization import awq_ops
    N = 8192 + 37
    x, s = _col_data(N, K, dt, K + 3)
    ref = (x.double() / s.double()).float().to(TD[dt])
    assert torch.equal(awq_ops.div_cols(x, s).view(-1).view(torch.uint8), ref.view(-1).view(torch.uint8))
    w = (x.float() * 0.01).to(TD[dt])            # weight-sized values: no product overflows f16
    ref = (w.double() * s.double()).float().to(TD[dt])
    awq_ops.mul_cols_(w, s)
    assert torch.equal(w.view(-1).view(torch.uint8), ref.view(-1).view(torch.uint8))


@pytest.mark.parametrize('dt', ['bf16', 'f16'])
@pytest.mark.parametrize('K', [4096, 4128, 14336])
def test_div_cols_tiled_is_ktile_pack_of_row_major(dt, K):
    """K = 4128: K % 64 == 32, the grid's last pair of 32-column k-tiles has one tile only"""
    from llmc_amd.compression.quantization import awq_ops
    x, s = _col_data(8192 + 37, K, dt, K + 5)
    a = awq_ops.div_cols(x, s, tiled=True)
    b = awq_ops.ktile_pack(awq_ops.div_cols(x, s))
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('g', [32, 128, 0])
def test_clamp_groups_vs_torch_clamp(dt, g):
    from llmc_amd.compression.quantization import awq_ops
    R, K = 300, 14336
    gw = g or K
    w = cpu_weights(R, K, 300 + g, dt).cuda()
    wg = w.float().reshape(R, K // gw, gw)
    mx = (wg.abs().amax(-1, keepdim=True) * 0.6).to(TD[dt])
    mn = (wg.amin(-1, keepdim=True) * 0.7).to(TD[dt])
    ref = torch.clamp(w.reshape(R, K // gw, gw), min=mn, max=mx).reshape(R, K)
    out = awq_ops.clamp_groups_(w.clone(), mn, mx, g)
    assert torch.equal(out.view(-1).view(torch.uint8), ref.reshape(-1).view(torch.uint8))
    assert not torch.equal(out, w)


# ---------------------------------------------------------------------------------------------------------------------
# per-channel AWQ end to end at Llama widths (these raised NotImplementedError while llmc_awq_weight_mean took only
# groups of 16 B x a power of two <= 64)
def test_search_scale_stacked_per_channel_w8_llama_width():
    """q / k / v-like stack: K = 4096, three layers of 512 rows, 2048 bf16 tokens, the weight quantizer of
    vllm/awq_w8a8.yml (8-bit symmetric per-channel), against the oracle's search"""
    from llmc_amd.compression.quantization.awq_pipeline import search_scale_stacked
    K, T = 4096, 2048
    gen = torch.Generator().manual_seed(4096)
    ws = [(torch.randn(512, K, generator=gen) * 0.02).to(torch.bfloat16) for _ in range(3)]
    col = torch.exp(torch.randn(K, generator=gen))
    col[::97] *= 20
    x = (torch.randn(T, K, generator=gen) * col).to(torch.bfloat16)
    q = int_q(8, True, 0)
    best, losses, n = search_scale_stacked([w.cuda() for w in ws], x.cuda(), q, 'v2', return_losses=True)
    ref_s, ref_l, ref_n = A.search_scale([w.float().numpy() for w in ws], x.float().numpy(), 'bf16', True, float(q.qmin),
                                         float(q.qmax), 0, 'v2')
    srt = np.sort(ref_l)
    assert (srt[1] - srt[0]) / srt[0] > 1e-2        # a clear winner: the argmin is not decided by the 1e-3 tolerance
    np.testing.assert_allclose(losses.cpu().numpy(), ref_l, rtol=1e-3)   # the W8 bound of test_search_matches_reference_golden
    assert n == ref_n
    assert ulps(host(best), ref_s, 'bf16').max() <= 2


@pytest.mark.parametrize('kind', ['int8', 'e4m3'])
def test_get_weight_scale_per_channel_down_proj_width(kind):
    """Awq.get_weight_scale on a down_proj-wide layer (K = 14336; 1024 of its rows) with a per-channel integer quantizer
    (methods/Awq/awq_w_a_mix_bits.yml) and a per-channel e4m3 FloatQuantizer (vllm/fp8/awq_fp8.yml)"""
    from llmc_amd.compression.quantization import FloatQuantizer
    from llmc_amd.compression.quantization.awq import Awq
    w = cpu_weights(1024, 14336, 14336, 'bf16')
    lin = torch.nn.Linear(14336, 1024, bias=False).to(torch.bfloat16)
    lin.weight.data = w.cuda()
    a = Awq.__new__(Awq)
    a.wquantizer = int_q(8, True, 0) if kind == 'int8' else FloatQuantizer('e4m3', True, 'per_channel', use_qtorch=True)
    out = a.get_weight_scale({'down_proj': lin})
    ref = A.weight_scale([w.float().numpy()], 'bf16', 0)
    assert ulps(host(out), ref, 'bf16').max() <= 2


# ---------------------------------------------------------------------------------------------------------------------
def test_get_act_scale_and_get_scales_follow_awq_bs():
    """Awq.get_act_scale / get_scales by name with awq_bs = half the batch: the reference averages the sub-batch means
    (awq.py:74-85), each rounded to the model dtype first"""
    from llmc_amd.compression.quantization import awq_ops
    from llmc_amd.compression.quantization.awq import Awq
    B, T, K, dt = 4, 160, 1024, 'bf16'
    gen = torch.Generator().manual_seed(5)
    col = torch.exp(torch.randn(K, generator=gen))
    x = (torch.randn(B, T, K, generator=gen) * col).to(torch.bfloat16)
    xn = x.float().numpy()
    # restatement of the reference: batch_means of x[i*bs:(i+1)*bs], sum() (0 + m0 + m1, in dt), / len
    bs = B // 2
    m = [A.act_mean(xn[i * bs:(i + 1) * bs], dt) for i in range(B // bs)]
    tot = m[0]
    for mi in m[1:]:
        tot = A.rnd(tot + mi, dt)
    ref = A.rnd(tot / np.float32(len(m)), dt)
    # the whole-batch mean rounds differently often enough for the test to tell the two apart
    assert (A.act_mean(xn, dt) != ref).mean() > 0.05
    a = Awq.__new__(Awq)
    a._bs, a.trans_version = bs, 'v2'
    xd = x.cuda()
    out = host(a.get_act_scale(xd))
    u = ulps(out, ref, dt)
    assert u.max() <= 1 and (u > 0).mean() <= 0.02, (u.max(), (u > 0).mean())
    wm = torch.from_numpy(A.rnd(np.random.default_rng(1).uniform(0.1, 0.9, K).astype(np.float32), dt)).to(torch.bfloat16)
    for ver in ('v1', 'v2'):
        a.trans_version = ver
        sc = host(a.get_scales(None, xd, wm.cuda(), False, 0.4))
        sref = A.get_scales(out, wm.float().numpy(), 0.4, dt, ver)
        u = ulps(sc, sref, dt)
        assert u.max() <= 1 and (u > 0).mean() <= 0.03, (ver, u.max())
        # the same scales as the kernel given the sub-batch mean
        assert np.array_equal(bits(sc), bits(host(awq_ops.awq_scales(torch.from_numpy(out).to(torch.bfloat16).cuda(),
                                                                       wm.cuda(), 0.4, ver))))
