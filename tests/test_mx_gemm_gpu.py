"""The OCP MX path on the GPU (csrc/mx_gemm.hip: llmc_mx_act_quant, llmc_mx_gemm; mx_ops.py; MxFp4RealQuantLinear) against
the numpy oracle (tests/mx_oracle.py).

The block-scaled matrix instruction's summation order over its 128 products is not documented, so no test assumes one:
  exact data   operands for which every partial sum in every order is an fp32 number (the condition is computed on the CPU and
               asserted BEFORE the comparison): the result must be bit-identical to the fp64 evaluation rounded once
  random data  |C - C_ref| <= K 2^-23 sum |a b| 2^(s_a + s_b - 254) (a truncating fp32 adder in any order) + half an ulp of the
               output dtype at |C_ref| widened by that bound
Test 1 (one-hot activations against an asymmetric weight, one block at a time carrying its own scale) is the probe that
established the instruction's operand and scale lane maps, kept as a regression test.

A finding about the instruction, measured with this file's probe on a kernel that issued ONE instruction per
e4m3 fragment: the products of one 32-block are aligned to the block's largest product and the bits more than 13 binary places
below its leading bit are cut off (256 + 2^-5 exact, 256 + 2^-6 .. 2^-9 came back as 256), and the random-data case
(5, 4096, 128) with e4m3 codes stood at 15.1 times its bound. e2m1 x e2m1 products span 8 binades and never reach the window.
llmc_mx_gemm therefore feeds the instruction one exponent class of the e4m3 codes at a time (three instructions per fragment,
csrc/mx_gemm.hip: mg_e4m3_classes); test_e4m3_alignment_window_probe pins that nothing is cut any more.
"""
import numpy as np
import pytest
import torch

import fp4_oracle as O
import mx_fixtures as FX
import mx_oracle as MX

pytestmark = pytest.mark.gpu

TDT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
BITS = ('e2m1', 'e4m3')


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits_of(t):
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def run_gemm(a, a_s, bit, b, b_s, dt, bias=None):
    """codes one per byte in, the device result out (a torch tensor on the GPU)"""
    from llmc_amd.compression.quantization.mx_ops import mx_gemm
    return mx_gemm(gpu(FX.pack(a, bit)), gpu(a_s), bit, gpu(O.pack_fp4(b)), gpu(b_s), dtype=TDT[dt], bias=bias)


def rounded_once(C, dt, bias=None):
    """the fp64 result (an fp32 number: asserted) rounded once to dt, then the bias added in dt — as a CPU tensor"""
    c32 = C.astype(np.float32)
    assert np.array_equal(c32.astype(np.float64), C)
    y = torch.from_numpy(c32).to(TDT[dt])
    if bias is not None:
        y = (y.float() + bias.cpu().float()).to(TDT[dt])
    return y


def check_exact(a, a_s, bit, b, b_s, dts=('f32',), with_bias=False, what=''):
    ok, ratio = MX.exact_in_any_order(a, a_s, bit, b, b_s)
    assert ok, f'{what}: the fixture is not exact in every order (sum |terms| / quantum = {ratio:.3g} >= 2^24)'
    C, _ = MX.gemm(a, a_s, bit, b, b_s)
    for dt in dts:
        for use_bias in ((False, True) if with_bias else (False,)):
            bias = None
            if use_bias:
                g = torch.Generator().manual_seed(5)
                bias = (torch.randint(-64, 65, (b.shape[0],), generator=g).float() * 0.25).to(TDT[dt]).cuda()
            got = run_gemm(a, a_s, bit, b, b_s, dt, bias)
            want = rounded_once(C, dt, bias)
            bad = bits_of(got) != bits_of(want)
            assert not bad.any(), (what, dt, use_bias, int(bad.sum()), np.argwhere(bad)[:4].tolist(),
                                   got.float().cpu().numpy()[bad][:4], want.float().numpy()[bad][:4])


def codes_of(values, bit):
    """format values -> codes, one per byte"""
    v = np.asarray(values, dtype=np.float32)
    return O.encode(v, 'e2m1') if bit == 'e2m1' else MX.e4m3_encode(v)


# ---- 1. lane and scale maps -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bit', BITS)
@pytest.mark.parametrize('R', [16, 32])
def test_lane_and_scale_maps(bit, R):
    """(R, R, 128): every (row, k) of A in turn carries the only non-zero code of its row — the 128 R one-hot rows stacked along M
    into one launch — against a weight whose code depends on n and k differently; then dense exact operands in which one
    32-block at a time carries a scale of its own, on the A side (stacked along M) and on the B side (stacked along N)."""
    K = 128
    n, k = np.meshgrid(np.arange(R), np.arange(K), indexing='ij')
    b = ((3 * n + 5 * k + n * k + k // 32) % 15 + 1).astype(np.uint8)          # never +0; code 8 (-0) included on purpose
    b_s = np.full((R, K // 32), 127, np.uint8)
    # one-hot: row j of the stacked A holds its only non-zero at k = j // R, so rows j % R = 0 .. R - 1 meet every k (a row of C
    # depends on its own row of A alone: R x 128 one-hot problems in one launch, at every row position of the kernel's tile)
    j = np.arange(K * R)
    a_val = np.zeros((K * R, K), np.float32)
    amp = np.array([0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0], np.float32)[(j * 7 + j // R) % 14]
    if bit == 'e4m3':
        amp = amp * np.float32(2.5)                                            # 1.25 .. 15: three-bit mantissas
    a_val[j, j // R] = amp
    a = codes_of(a_val, bit)
    a_s = np.full((K * R, K // 32), 127, np.uint8)
    check_exact(a, a_s, bit, b, b_s, what='one-hot A')
    # scales, A side: copy c of a dense A has block c of every row at 124 + (row % 7), everything else 127
    a0, _, bd, _ = FX.exact_operands(R, R, K, bit, seed=R)
    a4 = np.tile(a0, (4, 1))
    a4_s = np.full((4 * R, 4), 127, np.uint8)
    for c in range(4):
        a4_s[c * R:(c + 1) * R, c] = 124 + np.arange(R) % 7
    check_exact(a4, a4_s, bit, bd, b_s, what='A-side scales')
    # B side: copy c of the weight (stacked along N) has block c of every column at 131 - (n % 5)
    b4 = np.tile(bd, (4, 1))
    b4_s = np.full((4 * R, 4), 127, np.uint8)
    for c in range(4):
        b4_s[c * R:(c + 1) * R, c] = 131 - np.arange(R) % 5
    check_exact(a0, np.full((R, 4), 127, np.uint8), bit, b4, b4_s, what='B-side scales')


# ---- 2. exact data ----------------------------------------------------------------------------------------------------------------
EXACT_SHAPES = [(1, 16, 128), (17, 48, 256), (33, 80, 384), (129, 129, 1024)]                      # the tile is 128 x 128
EXACT_CASES = [(s, bit) for s in EXACT_SHAPES for bit in BITS] + [((64, 256, 4096), 'e2m1')]       # the e4m3 recipe holds up to K = 1024


@pytest.mark.parametrize('shape,bit', EXACT_CASES, ids=lambda v: v if isinstance(v, str) else 'x'.join(map(str, v)))
def test_exact_data_is_bit_identical(shape, bit):
    M, N, K = shape
    a, a_s, b, b_s = FX.exact_operands(M, N, K, bit, seed=M + N)
    check_exact(a, a_s, bit, b, b_s, dts=('bf16', 'f16', 'f32'), with_bias=True, what=str(shape))


# ---- 3. random data ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bit', BITS)
@pytest.mark.parametrize('shape', [(64, 512, 4096), (5, 4096, 128)], ids=lambda s: 'x'.join(map(str, s)))
def test_random_data_within_the_derived_bound(shape, bit):
    M, N, K = shape
    a, a_s, b, b_s = FX.random_operands(M, N, K, bit, seed=K)
    C, S = MX.gemm(a, a_s, bit, b, b_s)
    acc = MX.truncating_adder_bound(S, K)
    for dt in ('f32', 'bf16'):
        got = run_gemm(a, a_s, bit, b, b_s, dt).double().cpu().numpy()
        tol = acc + MX.half_ulp(np.abs(C) + acc, dt)
        err = np.abs(got - C)
        worst = float((err / tol).max())
        print(f'mx_gemm {bit} {shape} {dt}: worst |C - C_ref| / bound = {worst:.3f}, worst accumulation share '
              f'{float((np.maximum(err - MX.half_ulp(np.abs(C), dt), 0) / acc).max()):.3f}')
        assert np.isfinite(got).all() and worst <= 1.0, (bit, shape, dt, worst)



def test_e4m3_alignment_window_probe():
    """Two-term sums 256 * 1 + 2^e * 1, e = 7 .. -9 (the smallest e4m3 value), both terms exact in fp32 and the exactness condition
    holding with room to spare, the second term in the same 32-block, the next block, the other 64-deep half and the next
    instruction. One instruction per fragment returns 256.0 for e = -6 .. -9 inside the same block (the module docstring);
    the kernel's three exponent classes must give every sum exactly. A dense variant follows: full-range e4m3 codes in one block
    against weights of 1, scales 127, whose sum of at most 32 terms between 2^-9 and 448 is an fp32 number."""
    K = 256
    e = np.arange(7, -10, -1)
    b = np.tile(O.encode(np.ones((1, K), np.float32), 'e2m1'), (16, 1))
    b_s = np.full((16, K // 32), 127, np.uint8)
    for where, k in (('same block', 1), ('next block', 32), ('other 64-deep half', 64), ('next instruction', 128)):
        av = np.zeros((len(e), K), np.float32)
        av[:, 0] = 256.0
        av[:, k] = 2.0 ** e
        a = MX.e4m3_encode(av)
        a_s = np.full((len(e), K // 32), 127, np.uint8)
        assert MX.exact_in_any_order(a, a_s, 'e4m3', b, b_s)[0]
        C, _ = MX.gemm(a, a_s, 'e4m3', b, b_s)
        got = run_gemm(a, a_s, 'e4m3', b, b_s, 'f32').double().cpu().numpy()
        lost = e[got[:, 0] != C[:, 0]]
        print(f'e4m3 256 + 2^e, second term in the {where}: inexact for e = {lost.tolist()}')
        assert np.array_equal(got, C), (where, lost.tolist())
    rng = np.random.default_rng(9)
    a = np.zeros((64, K), np.uint8)
    a[:, 32:64] = rng.integers(0, 256, (64, 32))
    a[(a & 0x7f) == 0x7f] = 0x01
    a_s = np.full((64, K // 32), 127, np.uint8)
    assert MX.exact_in_any_order(a, a_s, 'e4m3', b, b_s)[0]             # 32 * 448 / 2^-9 < 2^24
    check_exact(a, a_s, 'e4m3', b, b_s, what='full-range codes in one block')


# ---- 4 / 5. the activation quantizer --------------------------------------------------------------------------------------------
ACT_SHAPES = [(3, 128), (257, 4096), (8, 14336)]


def act_input(M, K, dt, seed):
    """fp32 container of dt values with the special blocks in front: all zero, an exact power-of-two absmax, dt subnormals, the
    e2m1 rounding ties after scaling, scaled values in (448, 512), a NaN and an infinity among ordinary values"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((M, K)) * np.exp2(rng.integers(-6, 6, (M, K // 32)).repeat(32, axis=1))).astype(np.float32)
    x[0, 0:32] = 0.0
    x[0, 32:64] = np.where(np.arange(32) % 3 == 0, 4.0, 0.37)                                  # absmax 2^2
    sub = 2.0 ** -133 if dt == 'bf16' else 2.0 ** -24
    x[0, 64:96] = sub * np.arange(32)
    ties = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0, 7.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0], np.float32)
    x[0, 96:128] = np.tile(ties, 2) * 8.0                                                      # absmax 56 -> e2m1 scale 8
    if K >= 256:
        x[1, 0:32] = np.linspace(256.0, 511.0, 32) * 2.0 ** -3                                 # e4m3 scale 2^-3: (448, 512) saturates
        x[1, 32:64] = rng.standard_normal(32)
        x[1, 40], x[1, 41], x[1, 42] = np.nan, -np.inf, -0.0
        x[1, 64:96] = rng.standard_normal(32)
        x[1, 70] = np.inf
        x[1, 96:128] = -np.float32(np.nan)
    return O.from_bits16(O.bits16(x, dt), dt)


def to_gpu16(x, dt):
    return torch.from_numpy(O.bits16(x, dt).view(np.int16).copy()).cuda().view(TDT[dt])


@pytest.mark.parametrize('dt', ['bf16', 'f16'])
@pytest.mark.parametrize('shape', ACT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_act_quant_e2m1_is_the_quantizers_route(shape, dt):
    from llmc_amd.compression.quantization import FloatQuantizer
    from llmc_amd.compression.quantization.mx_ops import mx_act_quant
    x = act_input(*shape, dt, seed=shape[1])
    xg = to_gpu16(x, dt)
    q = FloatQuantizer('e2m1', True, 'per_group', group_size=32, use_qtorch=True, float_semantics='ocp', scale_format='e8m0')
    want_codes, want_s, _ = q.real_quant_weight_dynamic(xg)
    codes, s = mx_act_quant(xg, 'e2m1')
    assert codes.shape == (shape[0], shape[1] // 2) and s.shape == (shape[0], shape[1] // 32)
    assert torch.equal(s, want_s.reshape(s.shape)) and torch.equal(codes, want_codes)
    oc, osc = MX.act_quant(x, 'e2m1')                                                          # and the restated rules agree
    assert np.array_equal(s.cpu().numpy(), osc) and np.array_equal(codes.cpu().numpy(), oc)


@pytest.mark.parametrize('dt', ['bf16', 'f16'])
@pytest.mark.parametrize('shape', ACT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_act_quant_e4m3_is_the_oracle(shape, dt):
    from llmc_amd.compression.quantization.mx_ops import mx_act_quant, mx_dequant
    x = act_input(*shape, dt, seed=shape[1] + 1)
    xg = to_gpu16(x, dt)
    codes, s = mx_act_quant(xg, 'e4m3')
    oc, osc = MX.act_quant(x, 'e4m3')
    assert np.array_equal(s.cpu().numpy(), osc)
    bad = codes.cpu().numpy() != oc
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist(), x[bad][:4], codes.cpu().numpy()[bad][:4], oc[bad][:4])
    if shape[1] >= 256:
        sat = MX.scaled(oc[1:2, :32], osc[1:2, :1], 'e4m3')[0]
        assert (sat[x[1, :32] * 8 > 448] == 448 / 8).all() and (x[1, :32] * 8 > 448).sum() > 3
    back = mx_dequant(codes, s, 'e4m3', torch.float32).cpu().numpy()
    ok = ~np.isnan(back)
    with np.errstate(over='ignore'):                                  # an infinity's block scale: 448 * 2^120 is inf in fp32, on both sides
        assert np.array_equal(back[ok], MX.scaled(oc, osc, 'e4m3').astype(np.float32)[ok])


# ---- 6. the module ---------------------------------------------------------------------------------------------------------------
class Cfg(dict):
    __getattr__ = dict.get


WEIGHT = dict(bit='e2m1', symmetric=True, granularity='per_group', group_size=32, quant_type='float-quant', use_qtorch=True,
              float_semantics='ocp', scale_format='e8m0')
ACT = {'e2m1': dict(bit='e2m1', symmetric=True, granularity='per_group', group_size=32, quant_type='float-quant', use_qtorch=True,
                    float_semantics='ocp', scale_format='e8m0'),
       'e4m3': dict(bit='e4m3', symmetric=True, granularity='per_token', quant_type='float-quant', use_qtorch=True)}


def make_module(K, R, act_bit, bias=True, seed=0):
    from llmc_amd.compression.quantization import FloatQuantizer
    from llmc_amd.compression.quantization.module_utils import MxFp4RealQuantLinear
    torch.manual_seed(seed)
    lin = torch.nn.Linear(K, R, bias=bias).to(torch.bfloat16).cuda()
    wq = FloatQuantizer(**{k: v for k, v in WEIGHT.items() if k != 'quant_type'})
    qc = {'weight': dict(WEIGHT)}
    if act_bit:
        qc['act'] = dict(ACT[act_bit])
    return lin, MxFp4RealQuantLinear.new(lin, lambda m: wq.real_quant_weight_dynamic(m.weight.data), qc)


@pytest.mark.parametrize('act_bit', BITS)
@pytest.mark.parametrize('K,R', [(256, 96), (4096, 128)])
def test_module_forward(K, R, act_bit):
    from llmc_amd.compression.quantization.module_utils import MxFp4RealQuantLinear
    from llmc_amd.compression.quantization.mx_ops import mx_act_quant, mx_gemm
    lin, m = make_module(K, R, act_bit)
    assert m.weight_packed.shape == (R, K // 2) and m.weight_scale.shape == (R, K // 32) and m.weight_scale.dtype == torch.uint8
    assert (m.in_features, m.out_features, m.act_bit) == (K, R, act_bit) and 'MxFp4RealQuantLinear' in repr(m)
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(2, 19, K, generator=g) * 1.5).to(torch.bfloat16).cuda()
    y = m(x)
    assert y.shape == (2, 19, R) and y.dtype == torch.bfloat16
    codes, s = mx_act_quant(x, act_bit)
    assert torch.equal(y.view(torch.int16), mx_gemm(codes, s, act_bit, m.weight_packed, m.weight_scale, torch.bfloat16, m.bias).view(torch.int16))
    # within the derived bound of dequant(act) @ dequant(weight)^T in fp64, bias added after the rounding
    ac = codes.reshape(-1, codes.shape[-1]).cpu().numpy()
    ac = MX.unpack_fp4(ac) if act_bit == 'e2m1' else ac
    C, S = MX.gemm(ac, s.reshape(-1, K // 32).cpu().numpy(), act_bit, MX.unpack_fp4(m.weight_packed.cpu().numpy()), m.weight_scale.cpu().numpy())
    acc = MX.truncating_adder_bound(S, K)
    nb = mx_gemm(codes, s, act_bit, m.weight_packed, m.weight_scale, torch.bfloat16, None).double().cpu().numpy().reshape(-1, R)
    assert (np.abs(nb - C) <= acc + MX.half_ulp(np.abs(C) + acc, 'bf16')).all()
    want = (torch.from_numpy(nb).to(torch.bfloat16).float() + m.bias.cpu().float()).to(torch.bfloat16)
    assert torch.equal(y.reshape(-1, R).cpu().view(torch.int16), want.view(torch.int16))
    # state_dict round trip
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    assert set(sd) == {'weight_packed', 'weight_scale', 'bias'}
    m2 = MxFp4RealQuantLinear(torch.zeros_like(m.weight_packed), torch.zeros_like(m.bias), torch.zeros_like(m.weight_scale), act_bit)
    m2.in_features, m2.out_features = K, R
    m2.load_state_dict(sd)
    assert torch.equal(m2(x).view(torch.int16), y.view(torch.int16))


@pytest.mark.parametrize('K,act_bit', [(96, 'e2m1'), (256, None)])
def test_module_fallback_is_hip_linear_on_the_dequantized_weight(K, act_bit):
    from llmc_amd.compression.quantization.module_utils import hip_linear
    from llmc_amd.compression.quantization.quant import dequant_fpx
    lin, m = make_module(K, 64, act_bit)
    x = torch.randn(7, K, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).cuda()
    want = hip_linear(x, dequant_fpx(m.weight_packed, m.weight_scale, 'e2m1', 32, torch.bfloat16), m.bias)
    assert torch.equal(m(x).view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize('act_bit', BITS)
def test_toy_model_deploys_mxfp4(act_bit):
    from llmc_amd.compression.quantization import RTN
    from toy_model import ToyModel
    model = ToyModel(hidden=256, inner=384, n_blocks=2)
    algo = RTN(model, Cfg(weight=Cfg(WEIGHT), act=Cfg(ACT[act_bit]), special=Cfg()), None, None, Cfg())
    algo.deploy('mxfp4_quant', keep_device=True)
    for b in model.get_blocks():
        for name in ('gate_proj', 'up_proj', 'down_proj'):
            assert type(getattr(b, name)).__name__ == 'MxFp4RealQuantLinear', name
    x = torch.randn(2, 33, 256, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).cuda()
    with torch.no_grad():
        for b in model.get_blocks():
            x = b.cuda()(x)
    assert torch.isfinite(x).all()
