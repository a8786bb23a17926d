"""The OCP MXFP6 path on the GPU (csrc/mx6_gemm.hip, mx_ops.py, MxFp6RealQuantLinear) against numpy: fp4_oracle's e3m2 grid and
quantizer step, the 24-byte unpack and an fp64 product below. The instruction's summation order is not documented: the exact tests
use operands for which every partial sum in every order is an fp32 number (asserted first) and want the fp64 product rounded once.
Random data: per 128-deep step the kernel adds exact block sums into the fp32 accumulator, K / 128 results plus the start, each
addition losing at most 2^-23 of a partial sum that sum |a b| bounds: |C - C_ref| <= (K / 128 + 1) 2^-23 sum |a b| + half an output
ulp. (Two instructions per step, one per exponent class of A — DESIGN.md K27 — would allow 2 K / 128 + 1; the tighter figure is
asserted and the observed share printed.)"""
import numpy as np
import pytest
import torch

import fp4_oracle as O
import mx_oracle as MX

pytestmark = pytest.mark.gpu

TDT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
RUNGS = ('decode', 'tile128')
WEIGHT = dict(bit='e3m2', symmetric=True, granularity='per_group', group_size=32, quant_type='float-quant', use_qtorch=True,
              float_semantics='ocp', scale_format='e8m0')


def unpack6(packed):
    """dense form [R, 3K/4] -> codes [R, K]: code i of a row at bits 6 i .. 6 i + 5 of the row's little-endian bit stream"""
    bits = np.unpackbits(np.ascontiguousarray(packed, dtype=np.uint8), axis=1, bitorder='little')
    return np.packbits(np.pad(bits.reshape(packed.shape[0], -1, 6), ((0, 0), (0, 0), (0, 2))), axis=2, bitorder='little')[..., 0]


def gemm64(a, a_s, b, b_s):
    """(C, S): the block-scaled product in fp64 (value * 2^(scale - 127) per 32-block, exact) and the same sum over |a b|"""
    sc = lambda c, s: (O.decode(c, 'e3m2').astype(np.float64).reshape(c.shape[0], -1, 32)
                       * np.ldexp(1.0, np.asarray(s).astype(np.int64) - 127)[..., None]).reshape(c.shape)
    A, B = sc(a, a_s), sc(b, b_s)
    return A @ B.T, np.abs(A) @ np.abs(B).T


def exact_in_any_order(a, a_s, b, b_s):
    """every term is a multiple of q[m, n] = 2^-8 2^(min_kb (a_s + b_s) - 254) (e3m2 values are multiples of 2^-4) and
    sum |terms| < 2^24 q: every partial sum in every order is an fp32 number. Returns (holds, worst sum / q)."""
    _, S = gemm64(a, a_s, b, b_s)
    mn = (a_s.astype(np.int64)[:, None, :] + b_s.astype(np.int64)[None, :, :]).min(axis=2)
    ratio = float((S / np.ldexp(2.0 ** -8, mn - 254)).max())
    return ratio < 2.0 ** 24, ratio


def exact_operands(M, N, K, seed):
    """magnitude codes 0 .. 19 (0 .. 3.5: subnormals and both exponent classes of the kernel), random signs, scales 127 / 128:
    a term is at most 3.5^2 2^2 = 12544 quanta, K = 1024 of them stay below 2^24"""
    rng = np.random.default_rng(seed)
    mk = lambda R: ((rng.integers(0, 20, (R, K)) | (rng.integers(0, 2, (R, K)) << 5)).astype(np.uint8),
                    rng.integers(127, 129, (R, K // 32)).astype(np.uint8))
    return (*mk(M), *mk(N))


def bits_of(t):
    t = t.contiguous().cpu()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def run_gemm(a, a_s, b, b_s, dt, bias=None, rung=-1):
    from llmc_amd.compression.quantization.mx_ops import mx6_gemm, mx6_pack
    a, a_s, b, b_s = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (a, a_s, b, b_s))
    return mx6_gemm(mx6_pack(a), a_s, mx6_pack(b), b_s, dtype=TDT[dt], bias=bias, rung=rung)


def check_exact(a, a_s, b, b_s, dts=('f32',), with_bias=False, rung=-1):
    ok, ratio = exact_in_any_order(a, a_s, b, b_s)
    assert ok, f'the fixture is not exact in every order (sum |terms| / quantum = {ratio:.3g} >= 2^24)'
    C, _ = gemm64(a, a_s, b, b_s)
    c32 = C.astype(np.float32)
    assert np.array_equal(c32.astype(np.float64), C)
    for dt in dts:
        for use_bias in ((False, True) if with_bias else (False,)):
            want = torch.from_numpy(c32).to(TDT[dt])
            bias = None
            if use_bias:
                bias = (torch.randint(-64, 65, (b.shape[0],), generator=torch.Generator().manual_seed(5)).float() * 0.25).to(TDT[dt])
                want = (want.float() + bias.float()).to(TDT[dt])
                bias = bias.cuda()
            got = run_gemm(a, a_s, b, b_s, dt, bias, rung)
            bad = bits_of(got) != bits_of(want)
            assert not bad.any(), (dt, use_bias, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got.float().cpu().numpy()[bad][:4])


def bound(S, K, C, dt):
    acc = (K / 128 + 1) * 2.0 ** -23 * S
    return acc + MX.half_ulp(np.abs(C) + acc, dt)


def act_input(M, K, dt, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((M, K)) * np.exp2(rng.integers(-6, 6, (M, K // 32)).repeat(32, axis=1))).astype(np.float32)
    x[0, :32] = rng.uniform(-8, 8, 32)
    x[0, 3], x[0, 5], x[0, 7] = np.nan, 31.0, -30.0                     # absmax 31 -> scale 1: 31 and the tie 30 saturate at 28
    if K >= 96:
        x[0, 32:64] = 0.0
        x[0, 70], x[0, 71] = -np.inf, 0.37
    return O.from_bits16(O.bits16(x, dt), dt)


@pytest.mark.parametrize('dt', ['bf16', 'f16'])
@pytest.mark.parametrize('shape', [(1, 32), (5, 96), (130, 4096)], ids=lambda s: 'x'.join(map(str, s)))
def test_act_quant_is_the_quantizers_route_and_the_oracle(shape, dt):
    from llmc_amd.compression.quantization import FloatQuantizer
    from llmc_amd.compression.quantization.mx_ops import mx6_act_quant, mx6_pack
    M, K = shape
    x = act_input(M, K, dt, seed=K)
    xg = torch.from_numpy(O.bits16(x, dt).view(np.int16).copy()).cuda().view(TDT[dt])
    q = FloatQuantizer('e3m2', True, 'per_group', group_size=32, use_qtorch=True, float_semantics='ocp', scale_format='e8m0')
    want_codes, want_s, _ = q.real_quant_weight_dynamic(xg)
    codes, s = mx6_act_quant(xg)
    assert codes.shape == (M, K // 4 * 3) and s.shape == (M, K // 32)
    assert torch.equal(s, want_s.reshape(s.shape)) and torch.equal(codes, mx6_pack(want_codes.reshape(M, K)))
    # the oracle's quantizer step, given the block scales of the NaN-ignoring absmax (clamp(exponent field - 4, 0, 254))
    am = np.fmax.reduce(np.abs(x.reshape(-1, 32)), axis=1, initial=np.float32(0.0)).astype(np.float32)
    sc = np.where(am == 0, 127, np.clip(((am.view(np.uint32) >> 23) & 0xff).astype(np.int64) - 4, 0, 254)).astype(np.uint8)
    ref = O.run(x.reshape(-1, 32), dt, 'e3m2', 'ocp', 'e8m0', scales=sc)
    assert np.array_equal(s.cpu().numpy().reshape(-1), sc)
    assert np.array_equal(unpack6(codes.cpu().numpy()), ref['codes'].reshape(M, K))
    back = O.decode(unpack6(codes.cpu().numpy()), 'e3m2')[0]
    assert back[3] == 28 and back[5] == 28 and back[7] == -28 and (K < 96 or (back[32:64] == 0).all() and back[70] == -28)


@pytest.mark.parametrize('rung', RUNGS)
def test_operand_map_and_in_block_exactness(rung):
    K, r = 128, RUNGS.index(rung)
    n, k = np.meshgrid(np.arange(16), np.arange(K), indexing='ij')
    b = (1 + (3 * n + 5 * k + n * k) % 31 + ((n + k) % 3 == 0) * 32).astype(np.uint8)     # never zero, both signs
    ones = np.full((16, K // 32), 127, np.uint8)
    for j in (0, 3, 5, 7):
        a = np.zeros((16, K), np.uint8)
        i = np.arange(16)
        a[i, 8 * i + j] = 1 + (5 * i + 3 * j) % 31 + ((i + j) % 2) * 32
        C, _ = gemm64(a, ones, b, ones)
        assert np.array_equal(C, O.decode(a[i, 8 * i + j], 'e3m2').astype(np.float64)[:, None] * O.decode(b[:, 8 * i + j].T, 'e3m2'))
        check_exact(a, ones, b, ones, rung=r)
    # one block holding 28 once and +-0.0625 in the other 31 places, against columns of 28, of 0.0625, and the same mixtures:
    # 784 + 31 * 2^-8 needs 18 bits; an instruction fed the whole block at once returns 810.296875 for 810.3125
    a = np.zeros((16, K), np.uint8)
    b = np.zeros((16, K), np.uint8)
    kk = np.arange(32)
    for i in range(16):
        a[i, 32:64] = np.where(kk == i, 0x1f, 0x01 | (((kk + i) % 2) & (i > 7)) * 32)
    b[0, 32:64], b[1, 32:64], b[2, 32:64], b[3, 32:64] = 0x1f, 0x01, np.where(kk < 16, 0x1f, 0x01), np.where(kk % 2, 0x1f, 0x01)
    b[4:, 32:64] = a[4:, 32:64]
    C, _ = gemm64(a, ones, b, ones)
    assert C[0, 0] == 784 + 31 * 1.75 and C[0, 1] == 1.75 + 31 * 2.0 ** -8 and C[4, 4] == 784 + 31 * 2.0 ** -8
    check_exact(a, ones, b, ones, rung=r)


EXACT = [((1, 16, 128), 'decode'), ((17, 24, 384), 'tile128'), ((129, 130, 256), 'tile128'), ((64, 4096, 640), 'tile128'),
         ((300, 136, 1024), 'tile128'), ((16, 40, 1152), 'decode'), ((5, 130, 2176), 'decode')]


@pytest.mark.parametrize('shape,rung', EXACT, ids=lambda v: v if isinstance(v, str) else 'x'.join(map(str, v)))
def test_exact_data_is_bit_identical(shape, rung):
    from llmc_amd import _ffi
    M, N, K = shape
    assert RUNGS[_ffi.lib().llmc_mx6_gemm_rung(M, N, K)] == rung
    check_exact(*exact_operands(M, N, K, seed=M + N), dts=('bf16', 'f32'), with_bias=True)


def test_random_data_within_the_derived_bound():
    M, N, K = 33, 130, 512
    rng = np.random.default_rng(K)
    a, b = rng.integers(0, 64, (M, K)).astype(np.uint8), rng.integers(0, 64, (N, K)).astype(np.uint8)
    a_s, b_s = rng.integers(119, 136, (M, K // 32)).astype(np.uint8), rng.integers(119, 136, (N, K // 32)).astype(np.uint8)
    C, S = gemm64(a, a_s, b, b_s)
    for dt in ('f32', 'bf16'):
        got = run_gemm(a, a_s, b, b_s, dt).double().cpu().numpy()
        worst = float((np.abs(got - C) / bound(S, K, C, dt)).max())
        print(f'mx6_gemm {(M, N, K)} {dt}: worst |C - C_ref| / bound = {worst:.4f}')
        assert np.isfinite(got).all() and worst <= 1.0, (dt, worst)


class Cfg(dict):
    __getattr__ = dict.get


def test_toy_model_deploys_mxfp6_and_forward_is_the_gemm():
    from llmc_amd.compression.quantization import RTN
    from llmc_amd.compression.quantization.mx_ops import mx6_act_quant, mx6_gemm
    from toy_model import ToyModel
    model = ToyModel(hidden=256, inner=384, n_blocks=2)
    act = {k: v for k, v in WEIGHT.items()}
    algo = RTN(model, Cfg(weight=Cfg(WEIGHT), act=Cfg(act), special=Cfg()), None, None, Cfg())
    algo.deploy('mxfp6_quant', keep_device=True)
    for blk in model.get_blocks():
        for name in ('gate_proj', 'up_proj', 'down_proj'):
            assert type(getattr(blk, name)).__name__ == 'MxFp6RealQuantLinear', name
    m = model.get_blocks()[0].cuda().gate_proj
    K, R = 256, 384
    assert m.weight_packed.shape == (R, K // 4 * 3) and m.weight_scale.shape == (R, K // 32) and m.act_bit == 'e3m2'
    x = (torch.randn(2, 19, K, generator=torch.Generator().manual_seed(3)) * 1.5).to(torch.bfloat16).cuda()
    y = m(x)
    codes, s = mx6_act_quant(x)
    assert torch.equal(y.view(torch.int16), mx6_gemm(codes, s, m.weight_packed, m.weight_scale, torch.bfloat16, m.bias).view(torch.int16))
    C, S = gemm64(unpack6(codes.reshape(-1, K // 4 * 3).cpu().numpy()), s.reshape(-1, K // 32).cpu().numpy(),
                  unpack6(m.weight_packed.cpu().numpy()), m.weight_scale.cpu().numpy())
    assert (np.abs(y.double().cpu().numpy().reshape(-1, R) - C) <= bound(S, K, C, 'bf16')).all()
    with torch.no_grad():
        for blk in model.get_blocks():
            x = blk.cuda()(x)
    assert torch.isfinite(x).all()


@pytest.mark.parametrize('K,with_act', [(96, True), (256, False)])
def test_module_fallback_is_hip_linear_on_the_dequantized_weight(K, with_act):
    from llmc_amd.compression.quantization import FloatQuantizer
    from llmc_amd.compression.quantization.module_utils import MxFp6RealQuantLinear, hip_linear
    from llmc_amd.compression.quantization.quant import dequant_fpx
    torch.manual_seed(0)
    lin = torch.nn.Linear(K, 64).to(torch.bfloat16).cuda()
    wq = FloatQuantizer(**{k: v for k, v in WEIGHT.items() if k != 'quant_type'})
    qc = {'weight': dict(WEIGHT), **({'act': dict(WEIGHT)} if with_act else {})}
    codes, scales, _ = wq.real_quant_weight_dynamic(lin.weight.data)
    m = MxFp6RealQuantLinear.new(lin, lambda mod: (codes, scales, None), qc)
    assert np.array_equal(unpack6(m.weight_packed.cpu().numpy()), codes.reshape(64, K).cpu().numpy())
    x = torch.randn(7, K, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).cuda()
    want = hip_linear(x, dequant_fpx(codes.reshape(64, K), scales, 'e3m2', 32, torch.bfloat16), m.bias)
    assert torch.equal(m(x).view(torch.int16), want.view(torch.int16))
