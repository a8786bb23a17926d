"""The W4A16 Linear on AutoAWQ's GEMM layout (csrc/awq_gemm.hip): every rung bit for bit on inputs whose sums are exact, real
data within the bound of an fp32 accumulation, the de-quantize kernel against two restatements, the module's forward, and the
announced fallback of a group size the kernel refuses."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DTS = {'f16': torch.float16, 'bf16': torch.bfloat16}
ORDER = (0, 2, 4, 6, 1, 3, 5, 7)


def unpack(words):
    """int32 [A, C] -> int64 [A, 8 C] on the CPU: nibble i of a word holds column 8 c + ORDER[i]"""
    w = words.cpu().to(torch.int64) & 0xffffffff
    out = torch.empty(*w.shape, 8, dtype=torch.int64)
    for i, c in enumerate(ORDER):
        out[..., c] = (w >> (4 * i)) & 15
    return out.reshape(w.shape[0], -1)


def w_tilde(qw, qz, sc, g, dt):
    """W~ [K, R] by the stated formula on the CPU: the product is exact in fp64, `.to(dt)` is its one rounding"""
    d = unpack(qw) - unpack(qz).repeat_interleave(g, 0)
    return (d.double() * sc.cpu().double().repeat_interleave(g, 0)).to(dt)


def rungs_for(K):
    from llmc_amd.compression.quantization.awq_gemm_ops import RUNGS
    return [r for r in RUNGS if r != 'tile' or K % 64 == 0] + [None]


def ladder_ms():
    from llmc_amd.compression.quantization.awq_gemm_ops import LADDER
    return sorted({1, 33} | {m for bound, _, _ in LADDER if bound != math.inf for m in (bound, bound + 1)})


@pytest.mark.parametrize('R', [8, 264])
@pytest.mark.parametrize('K,g', [(128, 128), (384, 128), (192, 32)])
@pytest.mark.parametrize('M', ladder_ms())
@pytest.mark.parametrize('with_bias', [False, True])
@pytest.mark.parametrize('dt', list(DTS))
def test_exact_product(dt, with_bias, M, K, g, R):
    """x integers in [-4, 4], all codes and zeros of 0..15 with eight distinct nibbles per word, scales 2^-3..2^0, integer bias:
    |sum| <= 384 * 4 * 15 at a resolution of 2^-3 is 18 bits, so the fp32 accumulation is exact in any order and every rung
    returns the bits of the fp64 product rounded once."""
    from llmc_amd.compression.quantization.awq_gemm_ops import awq_gemm
    gen = torch.Generator().manual_seed(1000 * M + K + R)
    off = torch.randint(0, 16, (K, R // 8), generator=gen)
    qw = sum(((2 * i + off) % 16) << (4 * i) for i in range(8)).to(torch.int32)
    qz = torch.randint(0, 2 ** 32, (K // g, R // 8), generator=gen).to(torch.int32)
    sc = (2.0 ** -torch.randint(0, 4, (K // g, R), generator=gen)).to(torch.float16)
    x = torch.randint(-4, 5, (M, K), generator=gen).to(DTS[dt])
    bias = torch.randint(-8, 9, (R,), generator=gen).to(DTS[dt]) if with_bias else None
    want = x.double() @ w_tilde(qw, qz, sc, g, DTS[dt]).double() + (bias.double() if with_bias else 0.0)
    want = want.to(DTS[dt])
    for rung in rungs_for(K):
        y = awq_gemm(x.cuda(), qw.cuda(), qz.cuda(), sc.cuda(), g, bias.cuda() if with_bias else None, rung=rung)
        assert torch.equal(y.cpu().view(torch.int16), want.view(torch.int16)), rung


@functools.lru_cache(maxsize=None)
def real_case(M, K, R):
    """pack_awq_gemm of a random f16 weight with asymmetric g128 qparams, and a randn activation (fp32, cast per test)"""
    from llmc_amd.compression.quantization import IntegerQuantizer, pack_awq_gemm
    gen = torch.Generator().manual_seed(M + K + R)
    w = (torch.randn(R, K, generator=gen) * 0.05).to(torch.float16).cuda()
    _, s, z = IntegerQuantizer(4, False, 'per_group', group_size=128).real_quant_weight_dynamic(w)
    qw, sc, qz = pack_awq_gemm(w, s, z, 128)
    return qw, qz, sc, torch.randn(M, K, generator=gen)


def assert_within_bound(y, x, wt, bias, slices, dt, what):
    """|y - truth| <= e + u_dt (|truth| + e), e = gamma_n (|x| . |W~| (+ |bias|)), n = K + slices (+ 1 with a bias) fp32 additions
    at one ulp each (tests/divprune_oracle.bound's unit: the matrix pipe's adder is not promised to round to nearest), then the
    one rounding to dt"""
    xd, wd = x.cpu().double(), wt.double()
    truth, mag = xd @ wd, xd.abs() @ wd.abs()
    if bias is not None:
        truth, mag = truth + bias.cpu().double(), mag + bias.cpu().double().abs()
    n = (x.shape[-1] + slices + (bias is not None)) * 2.0 ** -23
    e = n / (1.0 - n) * mag
    bound = e + (2.0 ** -11 if dt == torch.float16 else 2.0 ** -8) * (truth.abs() + e)
    err = (y.cpu().double() - truth).abs()
    print(f'{what}: max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}')
    assert (err <= bound).all(), what


@pytest.mark.parametrize('M,K,R', [(48, 512, 512), (200, 1024, 264)])
@pytest.mark.parametrize('dt', list(DTS))
def test_real_data_within_bound(dt, M, K, R):
    from llmc_amd.compression.quantization.awq_gemm_ops import awq_gemm, stream_slices
    qw, qz, sc, x = real_case(M, K, R)
    x = x.to(DTS[dt]).cuda()
    wt = w_tilde(qw, qz, sc, 128, DTS[dt])
    for rung in rungs_for(K):
        y = awq_gemm(x, qw, qz, sc, 128, rung=rung)
        assert_within_bound(y, x, wt, None, stream_slices(M, K, R), DTS[dt], f'{dt} {M}x{K}x{R} {rung}')
        assert torch.equal(y.view(torch.int16), awq_gemm(x, qw, qz, sc, 128, rung=rung).view(torch.int16)), 'not repeatable'


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float32])
def test_dequant_kernel(dtype):
    """awq_dequant = awq_dequant_composed = the CPU formula, bit for bit: test 2's tensors (R / 8 a multiple of 4 and not) and
    hand-made words with a spilled group maximum (code 16 OR-ed in at nibble 2: a carry into nibble 3)"""
    from llmc_amd.compression.quantization.awq_gemm_ops import awq_dequant, awq_dequant_composed
    spilled = (torch.full((16, 1), 0x76543210) | (16 << 8)).to(torch.int32).cuda()
    hand = (spilled, torch.tensor([[0x01234567], [0x7fedcba9]], dtype=torch.int32).cuda(),
            torch.tensor([[0.5, 0.011, 1.5, 3.0, 0.25, 0.07, 2.0, 1.0]] * 2, dtype=torch.float16).cuda(), 8)
    for qw, qz, sc, g in (real_case(48, 512, 512)[:3] + (128,), real_case(200, 1024, 264)[:3] + (128,), hand):
        got = awq_dequant(qw, qz, sc, g, dtype).cpu()
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        assert torch.equal(got.view(bits), awq_dequant_composed(qw, qz, sc, g, dtype).cpu().view(bits))
        assert torch.equal(got.view(bits), w_tilde(qw, qz, sc, g, dtype).t().contiguous().view(bits))


@pytest.mark.parametrize('with_bias', [False, True])
@pytest.mark.parametrize('cls_name', ['AutoawqRealQuantLinear', 'MlcllmRealQuantLinear'])
def test_module_forward(cls_name, with_bias):
    from llmc_amd.compression.quantization import IntegerQuantizer, module_utils
    from llmc_amd.compression.quantization.awq_gemm_ops import awq_gemm, stream_slices
    torch.manual_seed(7)
    lin = torch.nn.Linear(256, 264, bias=with_bias).to(torch.float16).cuda()
    q = IntegerQuantizer(4, False, 'per_group', group_size=128)
    m = getattr(module_utils, cls_name).new(lin, lambda mod: q.real_quant_weight_dynamic(mod.weight.data),
                                           {'weight': {'bit': 4, 'group_size': 128, 'pack_version': 'gemm_pack'}})
    x = torch.randn(2, 5, 256, dtype=torch.float16, device='cuda')
    y = m(x)
    assert y.shape == (2, 5, 264) and m.group_size == 128
    assert torch.equal(y.view(torch.int16), awq_gemm(x, m.qweight, m.qzeros, m.scales, 128, m.bias).view(torch.int16))
    assert_within_bound(y.reshape(10, 264), x.reshape(10, 256), w_tilde(m.qweight, m.qzeros, m.scales, 128, torch.float16), m.bias,
                        stream_slices(10, 256, 264), torch.float16, f'{cls_name} bias={with_bias}')


def test_refused_group_size_takes_announced_fallback(capsys):
    from llmc_amd.compression.quantization.awq_gemm_ops import awq_dequant, awq_linear_forward
    from llmc_amd.compression.quantization.module_utils import hip_linear
    gen = torch.Generator().manual_seed(5)
    qw = torch.randint(0, 2 ** 32, (64, 5), generator=gen).to(torch.int32).cuda()
    qz = torch.randint(0, 2 ** 32, (8, 5), generator=gen).to(torch.int32).cuda()
    sc = (torch.rand(8, 40, generator=gen) * 0.1 + 0.01).to(torch.float16).cuda()
    x = torch.randn(3, 64, generator=gen).to(torch.bfloat16).cuda()
    y = [awq_linear_forward(x, qw, qz, sc, 8) for _ in range(2)]
    assert capsys.readouterr().err.count('awq_linear') == 1
    want = hip_linear(x, awq_dequant(qw, qz, sc, 8, torch.bfloat16), None)
    assert all(torch.equal(v.view(torch.int16), want.view(torch.int16)) for v in y)
