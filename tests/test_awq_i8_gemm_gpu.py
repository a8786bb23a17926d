"""The W4A8 Linear on AutoAWQ's GEMM layout (csrc/awq_i8_gemm.hip) against plain float64 numpy on the unpacked integers:
    ref(m, n) = a_s[m] * sum_g scales[g][n] * S_g(m, n) + bias[n],   S_g the exact integer sum of group g,
    |y - ref| <= u |ref| + (G + 3) 2^-23 (a_s[m] T(m, n) + |bias[n]|),   T = sum_g |scales[g][n] S_g(m, n)|, u = 2^-8 (bf16), 2^-11 (f16).
Derived, not measured: float(S_g) is exact; the kernel rounds once per group (an fma), once per added slice partial (at most G - 1
of them), once for the a_s product and once for the bias sum: at most 2 G + 1 roundings to nearest of 2^-24 each, relative to
partial sums that never exceed a_s T + |bias| — below (G + 3) 2^-23 for any slice order — and then once to the output dtype."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTS = {'f16': torch.float16, 'bf16': torch.bfloat16}
ORDER = (0, 2, 4, 6, 1, 3, 5, 7)
A_TOK = dict(bit=8, symmetric=True, granularity='per_token')
A_STATIC = dict(bit=8, symmetric=True, granularity='per_tensor', static=True)


def unpack(words):
    """int32 [A, C] -> int64 numpy [A, 8 C]: nibble i of a word holds column 8 c + ORDER[i]"""
    w = words.cpu().numpy().astype(np.int64) & 0xffffffff
    out = np.empty(w.shape + (8,), dtype=np.int64)
    for i, c in enumerate(ORDER):
        out[..., c] = (w >> (4 * i)) & 15
    return out.reshape(w.shape[0], -1)


def reference(a8, a_s, qw, qz, sc, g, bias):
    """(ref, a_s T + |bias|) in float64; a_s [M] or [1]"""
    d = unpack(qw) - np.repeat(unpack(qz), g, axis=0)
    a, s = a8.cpu().numpy().astype(np.int64), sc.cpu().double().numpy()
    ref, mag = 0.0, 0.0
    for kg in range(s.shape[0]):
        t = s[kg] * (a[:, kg * g:(kg + 1) * g] @ d[kg * g:(kg + 1) * g]).astype(np.float64)
        ref, mag = ref + t, mag + np.abs(t)
    asd = a_s.cpu().double().numpy().reshape(-1, 1)
    b = 0.0 if bias is None else bias.cpu().double().numpy()
    return asd * ref + b, asd * mag + np.abs(b)


def assert_within_bound(y, ref, mag, G, dt, what):
    u = 2.0 ** -11 if dt == torch.float16 else 2.0 ** -8
    err, bound = np.abs(y.cpu().double().numpy().reshape(ref.shape) - ref), u * np.abs(ref) + (G + 3) * 2.0 ** -23 * mag
    print(f'{what}: max err {err.max():.3e}, max err / bound {(err / np.maximum(bound, 1e-300)).max():.3f}')
    assert (err <= bound).all(), what


@functools.lru_cache(maxsize=None)
def case(M, K, g, R):
    """Random words (all 16 codes), zeros that differ per group and column with 0 and 15 forced in, scales whose neighbours in
    either direction differ by factors of 8 or 64, activation codes over the whole int8 range with -128, -127, 127 forced in"""
    gen = torch.Generator().manual_seed(7 * M + K + R + g)
    qw = torch.randint(0, 2 ** 32, (K, R // 8), generator=gen).to(torch.int32)
    qz = torch.randint(0, 2 ** 32, (K // g, R // 8), generator=gen).to(torch.int32)
    qz[0, 0] = 0x0f0ff0f0
    step = 8.0 ** ((torch.arange(K // g).reshape(-1, 1) + torch.arange(R).reshape(1, -1)) % 3)
    sc = ((torch.rand(K // g, R, generator=gen) * 0.5 + 0.5) * 2.0 ** -8 * step).to(torch.float16)
    a8 = torch.randint(-128, 128, (M, K), generator=gen).to(torch.int8)
    a8[0, :3] = torch.tensor([-128, -127, 127], dtype=torch.int8)
    a_s = torch.rand(M, generator=gen) * 0.05 + 0.001
    bias = torch.randn(R, generator=gen)
    return tuple(t.cuda() for t in (a8, a_s, qw, qz, sc, bias))


@pytest.mark.parametrize('R', [8, 264])
@pytest.mark.parametrize('K,g', [(96, 32), (384, 128), (1024, 128)])
@pytest.mark.parametrize('M', [1, 5, 33, 130])
@pytest.mark.parametrize('dt', list(DTS))
def test_every_rung_within_the_derived_bound(dt, M, K, g, R):
    from llmc_amd.compression.quantization.awq_gemm_ops import awq_i8_gemm
    a8, a_s, qw, qz, sc, bias = case(M, K, g, R)
    for b in (None, bias.to(DTS[dt])):
        ref, mag = reference(a8, a_s, qw, qz, sc, g, b)
        for rung in ('stream', 'tile', None):
            y = awq_i8_gemm(a8, a_s, qw, qz, sc, g, DTS[dt], bias=b, rung=rung)
            assert_within_bound(y, ref, mag, K // g, DTS[dt], f'{dt} {M}x{K}x{R} g{g} bias={b is not None} {rung}')


@pytest.mark.parametrize('rung', ['stream', 'tile'])
def test_per_tensor_scale_and_repeatable_bits(rung):
    from llmc_amd.compression.quantization.awq_gemm_ops import awq_i8_gemm
    a8, a_s, qw, qz, sc, bias = case(33, 1024, 128, 264)
    ref, mag = reference(a8, a_s[:1], qw, qz, sc, 128, None)
    y = awq_i8_gemm(a8, a_s[:1], qw, qz, sc, 128, torch.bfloat16, rung=rung)
    assert_within_bound(y, ref, mag, 8, torch.bfloat16, f'per tensor {rung}')
    assert torch.equal(y.view(torch.int16), awq_i8_gemm(a8, a_s[:1], qw, qz, sc, 128, torch.bfloat16, rung=rung).view(torch.int16))


@pytest.mark.parametrize('g', [16, 48])
def test_refused_group_size_takes_announced_fallback(g, capsys):
    """g % 32 != 0: NotImplementedError from the GEMM; the forward says so once and runs the W4A16 path on the de-quantized codes,
    within that path's bound (tests/test_awq_gemm_gpu.py: K + slices fp32 additions at one ulp each, then the rounding)"""
    from llmc_amd.compression.quantization.awq_gemm_ops import awq_i8_gemm, awq_i8_linear_forward, stream_slices
    from llmc_amd.compression.quantization.i8_linear_ops import i8_act_quant, i8_dequant
    gen = torch.Generator().manual_seed(g)
    K, R = 6 * g, 40
    qw = torch.randint(0, 2 ** 32, (K, R // 8), generator=gen).to(torch.int32).cuda()
    qz = torch.randint(0, 2 ** 32, (6, R // 8), generator=gen).to(torch.int32).cuda()
    sc = (torch.rand(6, R, generator=gen) * 0.1 + 0.01).to(torch.float16).cuda()
    x = torch.randn(3, K, generator=gen).to(torch.bfloat16).cuda()
    codes, a_s = i8_act_quant(x, A_TOK)
    with pytest.raises(NotImplementedError, match='32'):
        awq_i8_gemm(codes, a_s, qw, qz, sc, g)
    y = [awq_i8_linear_forward(x, qw, qz, sc, g, A_TOK) for _ in range(2)]
    assert capsys.readouterr().err.count('awq_i8_linear') == 1 and torch.equal(y[0], y[1])
    xq = i8_dequant(codes, a_s, torch.bfloat16).cpu().double().numpy()
    d = (unpack(qw) - np.repeat(unpack(qz), g, axis=0)).astype(np.float64) * np.repeat(sc.cpu().double().numpy(), g, axis=0)
    wt = torch.from_numpy(d).to(torch.bfloat16).double().numpy()
    truth, n = xq @ wt, (K + stream_slices(3, K, R)) * 2.0 ** -23
    e = n / (1.0 - n) * (np.abs(xq) @ np.abs(wt))
    assert (np.abs(y[0].cpu().double().numpy() - truth) <= e + 2.0 ** -8 * (np.abs(truth) + e)).all()


@pytest.mark.parametrize('act', [A_TOK, A_STATIC, None], ids=['per_token', 'static', 'no_act'])
@pytest.mark.parametrize('cls_name', ['AutoawqRealQuantLinear', 'MlcllmRealQuantLinear'])
def test_module_forward(cls_name, act):
    from llmc_amd.compression.quantization import IntegerQuantizer, module_utils
    from llmc_amd.compression.quantization.awq_gemm_ops import awq_linear_forward
    from llmc_amd.compression.quantization.i8_linear_ops import i8_act_quant
    torch.manual_seed(11)
    lin = torch.nn.Linear(256, 48).to(torch.bfloat16).cuda()
    lin.register_buffer('buf_act_scales_0', torch.tensor(0.03, device='cuda'))
    q = IntegerQuantizer(4, False, 'per_group', group_size=128)
    cfg = {'weight': {'bit': 4, 'group_size': 128, 'pack_version': 'gemm_pack'}}
    m = getattr(module_utils, cls_name).new(lin, lambda mod: q.real_quant_weight_dynamic(mod.weight.data), dict(cfg, act=act) if act else cfg)
    x = torch.randn(2, 3, 256, dtype=torch.bfloat16, device='cuda')
    y = m(x)
    assert y.shape == (2, 3, 48) and y.dtype == torch.bfloat16
    if act is None:
        assert m.act_mode is None and 'input_scale' not in m.state_dict()
        assert torch.equal(y.view(torch.int16), awq_linear_forward(x, m.qweight, m.qzeros, m.scales, 128, m.bias).view(torch.int16))
        return
    assert ('input_scale' in m.state_dict()) == (act is A_STATIC)
    codes, a_s = i8_act_quant(x, act, m.input_scale if act is A_STATIC else None)
    ref, mag = reference(codes.reshape(6, 256), a_s, m.qweight, m.qzeros, m.scales, 128, m.bias)
    assert_within_bound(y, ref, mag, 2, torch.bfloat16, f'{cls_name} {m.act_mode}')
