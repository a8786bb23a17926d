"""The QUIK real-quant Linear on the GPU (csrc/quik_gemm.hip): the activation split against the existing quantizer on the gathered
copy (bit for bit), the GEMM on each rung against float64 (bit for bit on exact inputs, within the stated bound on real ones),
the module, QUIK.deploy('quik_quant') and the composed fallback."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CONFIGS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_mixed_configs.json')
DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(64, 0), (64, 32), (192, 32), (448, 64), (4096, 256)]               # (Ki, Fp)
RUNG_M = [('decode', 1), ('decode', 16), ('decode', 17), ('decode', 64), ('tile128', 1), ('tile128', 65), ('tile128', 129)]
A_CFG = dict(bit=8, symmetric=True, granularity='per_token')


def _bits(t):
    return t.contiguous().view(torch.int16)


def _ids(K, F, seed):
    order = torch.randperm(K, generator=torch.Generator().manual_seed(seed))
    return order[:K - F].to(DEV), order[K - F:].to(DEV)


@pytest.mark.parametrize('M', [1, 3, 65])
@pytest.mark.parametrize('K,F', [(64, 0), (64, 24), (320, 0), (320, 24), (4096, 0), (4096, 24), (4096, 256)])
@pytest.mark.parametrize('dtype', DTYPES)
def test_split_equals_the_quantizer_on_the_gathered_copy(dtype, K, F, M):
    from llmc_amd.compression.quantization import IntegerQuantizer, quik_ops as QK
    g = torch.Generator().manual_seed(K + F + M)
    x = torch.randn(M, K, generator=g).to(dtype).to(DEV)
    int_ids, fp_ids = _ids(K, F, 1)
    if F:
        x[0, fp_ids[0]] = 1000.0                     # the row's largest |x| is an outlier: the scale must ignore it
    if M > 1:
        x[1] = 0                                     # a row of zeros
    n_int = K - F
    Ki, Fp = QK.padded(n_int, F)
    col_map = torch.empty(K, dtype=torch.int32, device=DEV)
    col_map[int_ids] = torch.arange(n_int, dtype=torch.int32, device=DEV)
    col_map[fp_ids] = Ki + torch.arange(F, dtype=torch.int32, device=DEV)
    codes, scales, a_fp = QK.quik_act_split(x, col_map, Ki, Fp)
    want_c, want_s, _ = IntegerQuantizer(8, True, 'per_token').real_quant_weight_dynamic(x.index_select(1, int_ids))
    assert codes.dtype == torch.int8 and tuple(codes.shape) == (M, Ki) and tuple(a_fp.shape) == (M, Fp) and a_fp.dtype == dtype
    assert torch.equal(codes[:, :n_int], want_c) and not codes[:, n_int:].any()
    assert scales.dtype == torch.float32 and torch.equal(scales.reshape(-1), want_s.float().reshape(-1))
    assert torch.equal(_bits(a_fp[:, :F]), _bits(x.index_select(1, fp_ids))) and not _bits(a_fp[:, F:]).any()


def _operands(M, N, Ki, Fp, dtype, exact, seed):
    g = torch.Generator().manual_seed(seed)
    if exact:      # codes and outliers in {-1, 0, 1}, scales powers of two: every partial sum is a small integer, exact in fp32
        a8, w8 = torch.randint(-1, 2, (M, Ki), generator=g), torch.randint(-1, 2, (N, Ki), generator=g)
        a_fp, w_fp = torch.randint(-1, 2, (M, Fp), generator=g).float(), torch.randint(-1, 2, (N, Fp), generator=g).float()
        a_s, w_s = 2.0 ** torch.randint(-2, 2, (M,), generator=g), 2.0 ** torch.randint(-2, 3, (N,), generator=g)
    else:
        a8, w8 = torch.randint(-128, 128, (M, Ki), generator=g), torch.randint(-128, 128, (N, Ki), generator=g)
        a_fp, w_fp = torch.randn(M, Fp, generator=g), torch.randn(N, Fp, generator=g)
        a_s, w_s = torch.rand(M, generator=g) * 0.05 + 1e-3, torch.rand(N, generator=g) * 0.02 + 1e-3
    a_fp, w_fp = a_fp.to(dtype), w_fp.to(dtype)
    i64 = (a8.double().numpy() @ w8.double().numpy().T) * a_s.double().numpy()[:, None] * w_s.double().numpy()[None, :]
    f64 = a_fp.double().numpy() @ w_fp.double().numpy().T
    fabs = a_fp.double().abs().numpy() @ w_fp.double().abs().numpy().T
    dev = [t.to(DEV) for t in (a8.to(torch.int8), a_s, a_fp, w8.to(torch.int8), w_s, w_fp)]
    return dev, i64, f64, fabs


@pytest.mark.parametrize('Ki,Fp', SHAPES)
@pytest.mark.parametrize('rung,M', RUNG_M)
@pytest.mark.parametrize('dtype', DTYPES)
def test_gemm_exact_inputs_equal_float64_bit_for_bit(dtype, rung, M, Ki, Fp):
    from llmc_amd.compression.quantization import quik_ops as QK
    for N in (16, 48, 144):
        ops, i64, f64, _ = _operands(M, N, Ki, Fp, dtype, True, M + N + Ki)
        bias = torch.randint(-4, 5, (N,), generator=torch.Generator().manual_seed(N)).to(dtype)
        want = torch.from_numpy(i64 + f64).to(dtype)
        got = QK.quik_gemm(*ops, dtype=dtype, rung=rung)
        assert torch.equal(_bits(got.cpu()), _bits(want)), (N, 'no bias')
        got = QK.quik_gemm(*ops, dtype=dtype, bias=bias.to(DEV), rung=rung)
        assert torch.equal(_bits(got.cpu()), _bits((want.float() + bias.float()).to(dtype))), (N, 'bias')


def _within_bound(got, i64, f64, fabs, Fp, dtype):
    """|y - y64| <= u_out |y64| + 2 (Fp + 4) 2^-24 (|int part| + sum |a_fp| |w_fp|): one unit of the output format, three fp32
    roundings of the scaled integer plus Fp accumulations, twice for an instruction that truncates where an add would round"""
    y64 = i64 + f64
    u_out = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -10
    bound = u_out * np.abs(y64) + 2 * (Fp + 4) * 2.0 ** -24 * (np.abs(i64) + fabs)
    err = np.abs(got.double().cpu().numpy() - y64)
    return bool((err <= bound).all()), float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize('Ki,Fp', [(64, 0), (64, 32), (4096, 256)])
@pytest.mark.parametrize('rung,M', [('decode', 1), ('decode', 64), ('tile128', 1), ('tile128', 129)])
@pytest.mark.parametrize('dtype', DTYPES)
def test_gemm_real_inputs_within_the_rounding_bound(dtype, rung, M, Ki, Fp):
    from llmc_amd.compression.quantization import quik_ops as QK
    for N in (16, 144):
        ops, i64, f64, fabs = _operands(M, N, Ki, Fp, dtype, False, M + N + Ki)
        ok, worst = _within_bound(QK.quik_gemm(*ops, dtype=dtype, rung=rung), i64, f64, fabs, Fp, dtype)
        print(f'{rung} M={M} N={N} Ki={Ki} Fp={Fp} {dtype}: worst error / bound = {worst:.3f}')
        assert ok, (N, worst)


def _module():
    """QuikRealQuantLinear.new on a 256 -> 48 bf16 Linear, F = 32 outlier columns chosen like QUIK does from a scale table"""
    from llmc_amd.compression.quantization import IntegerQuantizer
    from llmc_amd.compression.quantization.module_utils import QuikRealQuantLinear
    from llmc_amd.compression.quantization.quik import choose_indices
    g = torch.Generator().manual_seed(5)
    lin = torch.nn.Linear(256, 48, bias=False, dtype=torch.bfloat16).to(DEV)
    lin.weight.data = torch.randn(48, 256, generator=g).to(torch.bfloat16).to(DEV)
    int_ids, fp_ids = choose_indices(torch.rand(256, generator=g).to(DEV), 32)
    lin.register_buffer('buf_int_ids', int_ids)
    lin.register_buffer('buf_fp_ids', fp_ids)
    wq = IntegerQuantizer(8, True, 'per_channel')
    cfg = {'weight': dict(bit=8, symmetric=True, granularity='per_channel'), 'act': A_CFG}
    return QuikRealQuantLinear.new(lin, lambda m: wq.real_quant_weight_dynamic(m.weight.data.index_select(1, m.buf_int_ids)), cfg), g


def test_module_forward_against_float64_of_its_own_tensors():
    from llmc_amd.compression.quantization import i8_linear_ops as I8
    m, g = _module()
    assert tuple(m.weight.shape) == (48, 256) and tuple(m.weight_fp.shape) == (48, 32)      # n_int = 224 -> Ki = 256
    x = torch.randn(2, 5, 256, generator=g).to(torch.bfloat16).to(DEV)
    y = m(x)
    assert y.shape == (2, 5, 48) and y.dtype == torch.bfloat16
    codes, a_s = I8.i8_act_quant(x.reshape(10, 256).index_select(1, m.int_ids.long()), A_CFG)
    a_fp = x.reshape(10, 256).index_select(1, m.fp_ids.long()).double().cpu().numpy()
    w_fp = m.weight_fp.double().cpu().numpy()
    i64 = (codes.double().cpu().numpy() @ m.weight[:, :224].double().cpu().numpy().T) * a_s.double().cpu().numpy() \
        * m.weight_scale.double().cpu().numpy().T
    ok, worst = _within_bound(y.reshape(10, 48), i64, a_fp @ w_fp.T, np.abs(a_fp) @ np.abs(w_fp).T, 32, torch.bfloat16)
    assert ok, worst


def test_composed_fallback_equals_the_kernels_on_exact_inputs():
    """integer activations whose row maximum is 127 (scale 1: the codes are the values), weights in {-1, 0, 1}, scales powers of
    two: both routes round one exact sum once"""
    from llmc_amd.compression.quantization import quik_ops as QK
    m, g = _module()
    m.weight.copy_(torch.randint(-1, 2, (48, 256), generator=g).to(torch.int8))
    m.weight[:, 224:] = 0
    m.weight_scale.copy_((2.0 ** torch.randint(-2, 3, (48, 1), generator=g)))
    m.weight_fp.copy_(torch.randint(-1, 2, (48, 32), generator=g).to(torch.bfloat16))
    x = torch.randint(-3, 4, (7, 256), generator=g).to(torch.bfloat16).to(DEV)
    x[:, m.int_ids[0].long()] = 127
    got, want = QK.quik_linear_forward(x, m), QK.quik_linear_composed(x, m)
    assert got.dtype == want.dtype and torch.equal(_bits(got), _bits(want)) and got.float().abs().max() > 8


def test_quik_deploys_the_toy_model_to_modules_whose_forward_runs():
    import llmc_amd.compression.quantization as Q
    from toy_model import ToyModel, calib_input
    cfg = json.load(open(CONFIGS))['methods/QUIK/quik_w_a.yml']
    cfg['quant']['special'] = dict(cfg['quant']['special'], fp_features=32)
    model = ToyModel(hidden=256, inner=384, n_blocks=2)
    inp = calib_input(model, n_seq=4, seq=16)
    algo = Q.QUIK(model, dict(cfg['quant']), inp, None, {'calib': cfg['calib'], 'model': cfg['model'], 'quant': cfg['quant']})
    algo.run_block_loop()
    model.get_model().to(DEV)
    algo.deploy('quik_quant', keep_device=True)
    mods = [getattr(b, n) for b in model.get_blocks() for n in ('gate_proj', 'up_proj', 'down_proj')]
    assert all(type(m).__name__ == 'QuikRealQuantLinear' and m.act_mode == 'dynamic_per_token' for m in mods)
    assert all(m.fp_ids.numel() == 32 and m.weight.shape[1] == -(-(m.in_features - 32) // 64) * 64 for m in mods)
    h = inp['data'][0].to(DEV)
    with torch.no_grad():
        for b in model.get_blocks():
            h = b(h)
    assert h.shape == (1, 16, 256) and torch.isfinite(h.float()).all()
