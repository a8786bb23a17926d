"""The plain FP8 Linear on the GPU (csrc/fp8_linear.hip: llmc_fp8_scaled_gemm; fp8_linear_ops.py; VllmRealQuantLinear.forward)
against the numpy oracle (tests/fp8_linear_oracle.py) and a torch composition on the GPU.

  exact data   codes from {0, +-0.5, +-1, +-1.5, +-2}, power-of-two scales: every partial sum in every order is an fp32 number
               (asserted before the comparison), so C must equal the float64 result rounded once, bit for bit, on every rung,
               and the same call twice must return the same bits (the decode rung adds its K slices in a fixed order)
  random data  |C - E| <= c_acc(K) P + 2 2^-24 |E| + u_out |E| (+ u_out |E + bias|), the bound derived in the oracle's header
               from the matrix instruction's accumulation, against the oracle and against
               (a8.float() @ b8.float().T) * a_s * b_s computed by torch on the GPU
Shapes cross the edges of every rung: M 1 / 17 / 64 (decode rung with 1, 2 and 4 row tiles) and 65 / 257 (tile rung, one
and three row tiles with a ragged last one); N 16 / 130 / 256 / 513 (one decode workgroup, ragged and whole column tiles);
K 128 / 384 / 1152 (fewer K blocks than the decode rung has waves, an odd count, more than one per wave). Every rung also runs
every shape it takes by name, whatever the ladder would choose.
"""
import numpy as np
import pytest
import torch

import fp8_linear_oracle as O

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
TDT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
MS, NS, KS = (1, 17, 64, 65, 257), (16, 130, 256, 513), (128, 384, 1152)
W_CH = dict(bit='e4m3', symmetric=True, granularity='per_channel', quant_type='float-quant', use_qtorch=True)
W_T = dict(W_CH, granularity='per_tensor')
A_TOK = dict(bit='e4m3', symmetric=True, granularity='per_token', quant_type='float-quant', use_qtorch=True)
A_STATIC = dict(bit='e4m3', symmetric=True, granularity='per_tensor', quant_type='float-quant', use_qtorch=True, static=True)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits_of(t):
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def rungs_for(M):
    """None: the library's ladder; then every rung that takes M rows, by name"""
    return (None, 'decode', 'tile128') if M <= 64 else (None, 'tile128')


def gemm(a, a_s, b, b_s, dt, bias=None, rung=None):
    from llmc_amd.compression.quantization.fp8_linear_ops import fp8_scaled_gemm
    return fp8_scaled_gemm(a, a_s, b, b_s, dtype=TDT[dt], bias=bias, rung=rung)


def rounded_once(E, dt, bias=None):
    """the float64 result (an fp32 number: asserted) rounded once to dt, then the bias added in dt — a CPU tensor"""
    c32 = E.astype(np.float32)
    assert np.array_equal(c32.astype(np.float64), E)
    y = torch.from_numpy(c32).to(TDT[dt])
    if bias is not None:
        y = (y.float() + bias.cpu().float()).to(TDT[dt])
    return y


def exact_bias(N, dt):
    g = torch.Generator().manual_seed(5)
    return (torch.randint(-64, 65, (N,), generator=g).float() * 0.25).to(TDT[dt]).cuda()


# ---- exact data ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', MS)
def test_exact_data_is_bit_exact_on_every_rung(M):
    for N in NS:
        for K in KS:
            a, a_s, b, b_s = O.exact_case(M, N, K, seed=1000 * M + N + K)
            ok, ratio = O.exact_in_any_order(a, b)
            assert ok, ratio
            S = O.decode_e4m3fn(a) @ O.decode_e4m3fn(b).T
            ad, bd = gpu(a), gpu(b)
            first = True
            for per_token in (True, False):
                for per_channel in (True, False):
                    sa, sb = (a_s if per_token else a_s[:1]), (b_s if per_channel else b_s[:1])
                    E = S * O._col(sa, M)[:, None] * O._col(sb, N)[None, :]
                    sad, sbd = gpu(sa), gpu(sb)
                    full = per_token and per_channel
                    for dt in ('f32', 'bf16', 'f16'):
                        if dt != 'f32' and per_token != per_channel:
                            continue                          # the 16-bit outputs take the two pure pairings
                        for with_bias in (False, True):
                            bias = exact_bias(N, dt) if with_bias else None
                            want = bits_of(rounded_once(E, dt, bias))
                            for rung in (rungs_for(M) if full and dt == 'f32' else (None,)):
                                got = gemm(ad, sad, bd, sbd, dt, bias, rung)
                                bad = bits_of(got) != want
                                assert not bad.any(), ((M, N, K), dt, per_token, per_channel, with_bias, rung, int(bad.sum()),
                                                       np.argwhere(bad)[:4].tolist(), got.float().cpu().numpy()[bad][:4],
                                                       rounded_once(E, dt, bias).float().numpy()[bad][:4])
                                if first:                     # the same call again: the same bits
                                    again = gemm(ad, sad, bd, sbd, dt, bias, rung)
                                    assert np.array_equal(bits_of(again), bits_of(got)), ((M, N, K), rung)
                            first = False


def test_one_hot_rows_against_an_asymmetric_weight():
    """A = I (as e4m3 ones) against a weight whose every element differs: C is the weight's transpose, so a swapped row / column
    map or a wrong k order inside a lane's bytes cannot hide. Both instruction shapes: the decode rung and the tile rung."""
    K = 128
    vals = O.decode_e4m3fn(np.arange(0x08, 0x78, dtype=np.uint8))                 # 112 distinct normal numbers
    for M, N, rungs in ((64, 130, ('decode', 'tile128')), (129, 130, ('tile128',))):
        a = np.zeros((M, K), np.float64)
        a[np.arange(M), (np.arange(M) * 7 + 3) % K] = 1.0
        idx = (np.arange(N)[:, None] * 5 + np.arange(K)[None, :] * 3) % vals.size
        bvals = vals[idx] * np.where((np.arange(N)[:, None] + np.arange(K)[None, :]) % 3 == 0, -1.0, 1.0)
        ac, bc = O.encode_exact(a), O.encode_exact(bvals)
        one = np.ones(1, np.float32)
        E, _ = O.gemm(ac, one, bc, one)
        assert np.array_equal(E, bvals[:, (np.arange(M) * 7 + 3) % K].T)
        for rung in rungs:
            got = gemm(gpu(ac), gpu(one), gpu(bc), gpu(one), 'f32', None, rung).cpu().numpy().astype(np.float64)
            assert np.array_equal(got, E), (M, N, rung, np.argwhere(got != E)[:6].tolist())


def test_what_the_instruction_keeps():
    """The part of the measured accumulation behaviour the bound's derivation relies on (oracle header), kept as a
    regression test: a product 13 binary places below the leading bit of the largest product of its own group of 8 survives
    (256 + 2^-5), and products of different groups meet at fp32 width (256 + 2^-15). (What lies deeper inside a group is cut
    off; the bound allows for it, nothing asserts it.)"""
    one = gpu(np.ones(1, np.float32))
    for rung, M in (('decode', 16), ('tile128', 32)):
        for pos, j in ((1, 5), (9, 15), (17, 15), (100, 15)):
            a, b = np.zeros((M, 128)), np.zeros((16, 128))
            a[:, 0] = b[:, 0] = 16.0
            a[:, pos], b[:, pos] = 2.0 ** -(j // 2), 2.0 ** -(j - j // 2)
            got = gemm(gpu(O.encode_exact(a)), one, gpu(O.encode_exact(b)), one, 'f32', None, rung).double().cpu().numpy()
            assert (got == 256.0 + 2.0 ** -j).all(), (rung, pos, j, float(got[0, 0] - 256.0))


# ---- random data ---------------------------------------------------------------------------------------------------------
def check_random(M, N, K, seed):
    a, a_s, b, b_s = O.random_case(M, N, K, seed)
    ad, bd = gpu(a), gpu(b)
    S = O.decode_e4m3fn(a) @ O.decode_e4m3fn(b).T
    Sabs = np.abs(O.decode_e4m3fn(a)) @ np.abs(O.decode_e4m3fn(b)).T
    g = torch.Generator().manual_seed(seed)
    for per_row, with_bias in ((True, True), (False, False)):
        sa, sb = (a_s, b_s) if per_row else (a_s[:1], b_s[:1])
        sc = O._col(sa, M)[:, None] * O._col(sb, N)[None, :]
        E, P = S * sc, Sabs * sc
        sad, sbd = gpu(sa), gpu(sb)
        # the second opinion: torch's own fp32 product of the decoded codes, scaled in the kernel's order, on the GPU
        T = ((ad.view(FP8).float() @ bd.view(FP8).float().T) * sad.reshape(-1, 1)) * sbd.reshape(1, -1)
        for dt in ('f32', 'bf16'):
            bias = (torch.randn(N, generator=g) * float(np.abs(E).mean())).to(TDT[dt]).cuda() if with_bias else None
            bnp = None if bias is None else bias.float().cpu().numpy().astype(np.float64)
            bound = O.bound(E, P, K, dt, bnp)
            want = O.expected(E, bnp)
            want_t = T.double().cpu().numpy() + (0.0 if bnp is None else bnp[None, :])
            for rung in rungs_for(M):
                got = gemm(ad, sad, bd, sbd, dt, bias, rung).double().cpu().numpy()
                for ref, name in ((want, 'oracle'), (want_t, 'torch composition')):
                    r = np.abs(got - ref) / bound
                    print(f'fp8_scaled_gemm {(M, N, K)} {dt} per_row={per_row} rung={rung} vs {name}: max |C - ref| / bound = {r.max():.4f}')
                    assert (r <= 1.0).all(), ((M, N, K), dt, per_row, rung, name, float(r.max()), np.argwhere(r > 1)[:4].tolist())


@pytest.mark.parametrize('M', MS)
def test_random_data_within_the_oracles_bound(M):
    for N in NS:
        for K in KS:
            check_random(M, N, K, seed=7 * M + N + K)


@pytest.mark.parametrize('M,N', [(1, 513), (64, 130), (257, 256)])
def test_random_data_at_model_depth(M, N):
    check_random(M, N, 4096, seed=M)


# ---- return codes and the fallback ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [192, 64])
def test_unsupported_depth_is_enotsup_and_the_linear_still_runs(K, capfd):
    from llmc_amd import _ffi
    from llmc_amd.compression.quantization import fp8_linear_ops as F8
    from llmc_amd.compression.quantization.quant import FloatQuantizer
    M, N = 5, 48
    g = torch.Generator().manual_seed(K)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).cuda()
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).cuda()
    wq = FloatQuantizer(**{k: v for k, v in W_CH.items() if k != 'quant_type'})
    w8, w_s, _ = wq.real_quant_weight_dynamic(w)
    codes, a_s = F8.fp8_act_quant(x, A_TOK)
    # the raw entry: LLMC_ENOTSUP, and nothing is launched (C keeps its fill)
    c = torch.full((M, N), 7.0, dtype=torch.bfloat16, device='cuda')
    ws32 = w_s.reshape(-1).float().contiguous()
    as32 = a_s.reshape(-1).contiguous()
    rc = _ffi.lib().llmc_fp8_scaled_gemm(_ffi.ptr(codes), _ffi.ptr(as32), M, _ffi.ptr(w8), _ffi.ptr(ws32), N, M, N, K,
                                         _ffi.dt(torch.bfloat16), None, _ffi.ptr(c), _ffi.stream())
    torch.cuda.synchronize()
    assert rc == -95 and '128' in _ffi.last_error() and bool((c == 7.0).all())
    with pytest.raises(NotImplementedError):
        F8.fp8_scaled_gemm(codes, a_s, w8, w_s)
    # the Linear: said once, and the composition's numbers. The fallback multiplies the two de-quantized operands in bf16: each
    # operand element carries one bf16 rounding (u = 2^-8) of code * scale, the 16-bit GEMM accumulates in fp32 and rounds once.
    #   |y - E| <= d + u (|E| + d),  d = ((1 + u)^2 - 1) P + c_acc(K) (1 + u)^2 P
    # and the composition T it is compared with is itself an fp32 product: c_acc(K) P more.
    F8._FALLBACK_SEEN.clear()
    capfd.readouterr()
    y = F8.fp8_linear_forward(x, w8, w_s, A_TOK, None, None)
    y2 = F8.fp8_linear_forward(x, w8, w_s, A_TOK, None, None)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert err.count('[llmc_amd] fp8_linear') == 1 and '128' in err, err
    assert torch.equal(y, y2) and y.dtype == torch.bfloat16 and tuple(y.shape) == (M, N)
    A, B = codes.float(), w8.float()
    sc = a_s.reshape(-1, 1) * w_s.float().reshape(1, -1)
    T = ((A @ B.T) * a_s.reshape(-1, 1)) * w_s.float().reshape(1, -1)
    P = (A.abs() @ B.abs().T) * sc
    u = 2.0 ** -8
    d = ((1 + u) ** 2 - 1) * P + O.c_acc(K) * (1 + u) ** 2 * P
    bound = d + u * (T.abs() + d) + O.c_acc(K) * P
    r = ((y.float() - T).abs() / bound).max().item()
    print(f'fp8_linear_forward fallback K={K}: max |y - T| / bound = {r:.4f}')
    assert r <= 1.0


# ---- layer level ---------------------------------------------------------------------------------------------------------
def _layer(in_f, out_f, bias, seed):
    g = torch.Generator().manual_seed(seed)
    lin = torch.nn.Linear(in_f, out_f, bias=bias)
    lin.weight.data = torch.randn(out_f, in_f, generator=g) * 0.05
    if bias:
        lin.bias.data = torch.randn(out_f, generator=g) * 0.1
    lin = lin.to(torch.bfloat16).cuda()
    x = (torch.randn(2, 9, in_f, generator=g) * torch.exp(0.5 * torch.randn(in_f, generator=g))).to(torch.bfloat16).cuda()
    return lin, x


@pytest.mark.parametrize('cls_name', ['VllmRealQuantLinear', 'SglRealQuantLinear'])
@pytest.mark.parametrize('in_f,out_f,bias', [(256, 130, True), (384, 16, False)])
def test_layer_forward(cls_name, in_f, out_f, bias):
    from llmc_amd.compression.quantization import fp8_linear_ops as F8
    from llmc_amd.compression.quantization import module_utils as MU
    from llmc_amd.compression.quantization.quant import FloatQuantizer
    cls = getattr(MU, cls_name)
    lin, x = _layer(in_f, out_f, bias, seed=in_f)

    def quantizer(cfg):
        return FloatQuantizer(**{k: v for k, v in cfg.items() if k != 'quant_type'})

    # per-channel weight, dynamic per-token activation
    wq, aq = quantizer(W_CH), quantizer(A_TOK)
    m = cls.new(lin, lambda mod: wq.real_quant_weight_dynamic(mod.weight.data), {'weight': W_CH, 'act': A_TOK, 'quant_type': 'float-quant'})
    assert m.weight.dtype == FP8 and tuple(m.weight_scale.shape) == (out_f, 1) and m.act_mode == 'dynamic_per_token'
    y = m(x)
    codes, a_s = F8.fp8_act_quant(x, A_TOK)
    assert codes.dtype == FP8 and codes.shape == x.shape and a_s.dtype == torch.float32 and tuple(a_s.shape) == (2, 9, 1)
    want = F8.fp8_scaled_gemm(codes, a_s, m.weight, m.weight_scale, dtype=x.dtype, bias=m.bias)
    assert y.dtype == x.dtype and tuple(y.shape) == (2, 9, out_f) and torch.equal(y.view(torch.int16), want.view(torch.int16))
    # decode(code) * scale is the fake-quant activation, bit for bit
    fake = aq.fake_quant_act_dynamic(x)
    assert torch.equal(F8.fp8_dequant(codes, a_s, x.dtype).view(torch.int16), fake.view(torch.int16))

    # per-tensor weight, static per-tensor activation
    wq, aq = quantizer(W_T), quantizer(A_STATIC)
    lin.register_buffer('buf_act_scales_0', (x.float().abs().max() / 448.0).reshape(()))
    m = cls.new(lin, lambda mod: wq.real_quant_weight_dynamic(mod.weight.data), {'weight': W_T, 'act': A_STATIC, 'quant_type': 'float-quant'})
    assert m.weight_scale.numel() == 1 and m.input_scale.numel() == 1 and m.act_mode == 'static_per_tensor'
    y = m(x)
    codes, a_s = F8.fp8_act_quant(x, A_STATIC, m.input_scale)
    assert tuple(a_s.shape) == (1,) and torch.equal(a_s.reshape(()), m.input_scale.float().reshape(()))
    want = F8.fp8_scaled_gemm(codes, a_s, m.weight, m.weight_scale, dtype=x.dtype, bias=m.bias)
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))
    fake = aq.fake_quant_act_static(x, {'scales': m.input_scale})
    assert torch.equal(F8.fp8_dequant(codes, a_s, x.dtype).view(torch.int16), fake.view(torch.int16))

    # weight-only: the de-quantized weight through the 16-bit GEMM
    wq = quantizer(W_CH)
    m = cls.new(lin, lambda mod: wq.real_quant_weight_dynamic(mod.weight.data), {'weight': W_CH})
    assert m.act_mode is None
    want = MU.hip_linear(x, F8.fp8_dequant(m.weight, m.weight_scale, x.dtype), m.bias)
    assert torch.equal(m(x).view(torch.int16), want.view(torch.int16))


# ---- block loop ----------------------------------------------------------------------------------------------------------
class Cfg(dict):
    __getattr__ = dict.get


def test_rtn_fp8_deployed_model_runs_within_the_per_layer_bounds():
    """RTN with the rtn_fp8 quant section (per-channel e4m3 weights, dynamic per-token e4m3 activations), deploy('vllm_quant'),
    then the model runs. Every deployed Linear is compared, on the input it actually received in that run, with the torch
    composition of the same codes: ((a8.float() @ w8.float().T) * a_s) * w_s. Feeding both the same input is what makes the
    per-layer bound rigorous (two runs that drift apart layer by layer have no bound that follows from the formats); a block's
    output is its input plus its last Linear's output, so the layer bounds are the model's. The composition is an fp32 product
    itself: its own c_acc(K) P is added to the oracle's bound."""
    import llmc_amd.compression.quantization as Q
    from llmc_amd.compression.quantization import fp8_linear_ops as F8
    from toy_model import ToyModel, calib_input
    model = ToyModel()
    inp = calib_input(model)
    config = Cfg(calib=Cfg(seq_len=64), model=Cfg(type='Toy'))
    qc = Cfg(method='RTN', weight=Cfg(W_CH), act=Cfg(A_TOK), quant_type='float-quant')
    algo = Q.RTN(model, qc, inp, None, config)
    algo.run_block_loop()
    algo.deploy('vllm_quant', keep_device=True)
    seen = []
    hooks = []
    for blk in model.get_blocks():
        blk.cuda()
        for name in ('gate_proj', 'up_proj', 'down_proj'):
            m = getattr(blk, name)
            assert type(m).__name__ == 'VllmRealQuantLinear' and m.weight.dtype == FP8 and m.act_mode == 'dynamic_per_token'
            hooks.append(m.register_forward_hook(lambda mod, args, out, name=name: seen.append((name, mod, args[0].detach().clone(), out.detach().clone()))))
    x = inp['data'][0].cuda()
    with torch.no_grad():
        for blk in model.get_blocks():
            x = blk(x)
    for h in hooks:
        h.remove()
    assert len(seen) == 6 and bool(torch.isfinite(x).all())
    u = 2.0 ** -8
    for name, m, xin, out in seen:
        K = xin.shape[-1]
        codes, a_s = F8.fp8_act_quant(xin, m.act_cfg)
        A, B = codes.reshape(-1, K).float(), m.weight.float()
        w_s = m.weight_scale.float().reshape(1, -1)
        T = ((A @ B.T) * a_s.reshape(-1, 1)) * w_s
        P = (A.abs() @ B.abs().T) * a_s.reshape(-1, 1) * w_s
        bound = 2 * O.c_acc(K) * P + (2.0 ** -23 + u) * T.abs()
        r = ((out.reshape(-1, out.shape[-1]).float() - T).abs() / bound).max().item()
        print(f'deployed {name} K={K}: max |y - T| / bound = {r:.4f}')
        assert r <= 1.0, (name, r)
