"""The W8A8 integer Linear on the GPU (csrc/i8_linear.hip: llmc_i8_scaled_gemm; i8_linear_ops.py; VllmRealQuantLinear.forward)
against the arithmetic in numpy: the int64 product, one conversion to fp32, the two scale products in fp32 in the kernel's order,
one rounding, the bias in the output dtype. The int32 accumulator is exact, so every comparison is bit for bit on arbitrary data.
Shapes cross the edges of every rung: M 1 / 17 / 64 (decode rungs with 1, 2 and 4 row tiles) and 65 / 257 (tile rung, one and
three row tiles, the last ragged); N 16 / 130 / 513; K 16 (less than one instruction's depth), 208 (3 x 64 + 16: a ragged chunk
and a ragged 128-byte stage) and 1152 (more K blocks than the decode rung has waves)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TDT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
MS, NS, KS = (1, 17, 64, 65, 257), (16, 130, 513), (16, 208, 1152)
W_CH = dict(bit=8, symmetric=True, granularity='per_channel', group_size=-1)
W_T = dict(bit=8, symmetric=True, granularity='per_tensor')
A_TOK = dict(bit=8, symmetric=True, granularity='per_token')
A_STATIC = dict(bit=8, symmetric=True, granularity='per_tensor', static=True, calib_algo='static_minmax')


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits_of(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def rungs_for(M):
    """None: the library's ladder; then every rung that takes M rows, by name"""
    return (None, 'decode', 'decode_split', 'tile128') if M <= 64 else (None, 'tile128')


def gemm(a, a_s, b, b_s, dt, bias=None, rung=None):
    from llmc_amd.compression.quantization.i8_linear_ops import i8_scaled_gemm
    return i8_scaled_gemm(a, a_s, b, b_s, dtype=TDT[dt], bias=bias, rung=rung)


def reference(a, b, sa, sb, dt, bias=None):
    """a [M, K], b [N, K] int8; sa [M] or [1], sb [N] or [1] float32; bias a CPU tensor of dt -> a CPU tensor of dt"""
    acc = a.astype(np.int64) @ b.astype(np.int64).T
    f = acc.astype(np.float32)
    y = (f * sa.astype(np.float32).reshape(-1, 1)) * sb.astype(np.float32).reshape(1, -1)
    assert y.dtype == np.float32
    y = torch.from_numpy(y).to(TDT[dt])
    return y if bias is None else y + bias


def assert_same(got, want, what):
    bad = bits_of(got) != bits_of(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got.float().cpu().numpy()[bad][:4], want.float().numpy()[bad][:4])


@pytest.mark.parametrize('M', MS)
def test_random_codes_are_bit_exact_on_every_rung(M):
    rng = np.random.default_rng(M)
    for N in NS:
        for K in KS:
            a = rng.integers(-128, 128, (M, K), dtype=np.int8)
            b = rng.integers(-128, 128, (N, K), dtype=np.int8)
            sa = np.exp(rng.normal(size=M)).astype(np.float32) * 0.01
            sb = np.exp(rng.normal(size=N)).astype(np.float32) * 0.002
            ad, bd = gpu(a), gpu(b)
            for dt in ('f32', 'bf16', 'f16'):
                for per_token, per_channel in ((True, True), (False, False), (True, False), (False, True)):
                    if dt != 'f32' and per_token != per_channel:
                        continue                              # the 16-bit outputs take the two pure pairings
                    s1, s2 = (sa if per_token else sa[:1]), (sb if per_channel else sb[:1])
                    for with_bias in (False, True):
                        bias = torch.from_numpy(rng.normal(size=N).astype(np.float32)).to(TDT[dt]) if with_bias else None
                        want = reference(a, b, s1, s2, dt, bias)
                        for rung in rungs_for(M):
                            what = ((M, N, K), dt, per_token, per_channel, with_bias, rung)
                            got = gemm(ad, gpu(s1), bd, gpu(s2), dt, None if bias is None else bias.cuda(), rung)
                            assert_same(got, want, what)
                    for rung in rungs_for(M):                 # the same call again: the same bits
                        again = [gemm(ad, gpu(s1), bd, gpu(s2), dt, None, rung) for _ in range(2)]
                        assert_same(again[0], again[1].cpu(), ((M, N, K), dt, rung, 'not repeatable'))


@pytest.mark.parametrize('M', [3, 65])
def test_saturated_sums_are_converted_round_to_nearest_even(M):
    """All codes 127 but one 126 per row of A: every sum is 127 * 127 * 1151 + 126 * 127 = 18580481, above 2^24 and odd, so it lies
    halfway between two fp32 numbers and only round-to-nearest-even gives 18580480."""
    N, K = 130, 1152
    a, b = np.full((M, K), 127, np.int8), np.full((N, K), 127, np.int8)
    a[np.arange(M), (np.arange(M) * 37 + 5) % K] = 126
    one = np.ones(1, np.float32)
    want = reference(a, b, one, one, 'f32')
    assert (want.numpy() == 18580480.0).all()
    for rung in rungs_for(M):
        assert_same(gemm(gpu(a), gpu(one), gpu(b), gpu(one), 'f32', None, rung), want, (M, rung))


def test_one_hot_rows_against_a_weight_of_distinct_elements():
    """A has one 1 per row, at a k of its own; every element of a row of the weight differs from the others (3 k mod 256 is
    injective for k < 128), so C[m, n] = b[n, k(m)] and a wrong lane -> k map or a swapped row / column map cannot hide. Both
    instruction shapes: the decode rungs and the tile rung."""
    K = 128
    for M, N in ((64, 130), (129, 130)):
        pos = (np.arange(M) * 7 + 3) % K
        a = np.zeros((M, K), np.int8)
        a[np.arange(M), pos] = 1
        b = (((np.arange(N)[:, None] * 5 + np.arange(K)[None, :] * 3) % 256) - 128).astype(np.int8)
        one = np.ones(1, np.float32)
        for rung in rungs_for(M)[1:]:
            got = gemm(gpu(a), gpu(one), gpu(b), gpu(one), 'f32', None, rung).cpu().numpy()
            assert np.array_equal(got, b[:, pos].T.astype(np.float32)), (M, N, rung, np.argwhere(got != b[:, pos].T)[:6].tolist())


def test_return_codes_and_the_fallback(capfd):
    from llmc_amd import _ffi
    from llmc_amd.compression.quantization import i8_linear_ops as I8
    from llmc_amd.compression.quantization.module_utils import hip_linear
    L, bf16 = _ffi.lib(), _ffi.dt(torch.bfloat16)
    one = torch.ones(1, device='cuda')

    def raw(M, N, K, rung, ws_bytes):
        a, b = torch.ones(M, K, dtype=torch.int8, device='cuda'), torch.ones(N, K, dtype=torch.int8, device='cuda')
        c = torch.full((M, N), 7.0, dtype=torch.bfloat16, device='cuda')
        ws = _ffi.workspace(max(ws_bytes, 4), 'cuda')
        rc = L.llmc_i8_scaled_gemm_on_rung(_ffi.ptr(a), _ffi.ptr(one), 1, _ffi.ptr(b), _ffi.ptr(one), 1, M, N, K, bf16, None, _ffi.ptr(c),
                                           _ffi.ptr(ws), ws_bytes, rung, _ffi.stream())
        torch.cuda.synchronize()
        return rc, _ffi.last_error(), c

    for K, word in ((24, '16'), (131072, '65536')):           # the depth rules: LLMC_ENOTSUP, nothing is launched (C keeps its fill)
        for rung in (-1, 0, 1):
            rc, msg, c = raw(2, 16, K, rung, 0)
            assert rc == -95 and word in msg and bool((c == 7.0).all()), (K, rung, rc, msg)
    need = L.llmc_i8_scaled_gemm_ws_bytes(5, 48, 1152)
    assert need >= 2 * 5 * 48 * 4
    rc, msg, c = raw(5, 48, 1152, 2, need - 4)                # a short workspace: LLMC_EINVAL
    assert rc == -22 and 'workspace' in msg and bool((c == 7.0).all())
    rc, _, c = raw(5, 48, 1152, 2, need)
    assert rc == 0 and bool((c == 1152.0).all())
    # the Linear at a depth the GEMM refuses: said once, and the numbers of the composition it names
    g = torch.Generator().manual_seed(24)
    x = torch.randn(5, 24, generator=g).to(torch.bfloat16).cuda()
    w8 = torch.randint(-128, 128, (48, 24), generator=g, dtype=torch.int8).cuda()
    w_s = (torch.rand(48, 1, generator=g) * 0.01 + 0.001).to(torch.bfloat16).cuda()
    I8._FALLBACK_SEEN.clear()
    capfd.readouterr()
    y = [I8.i8_linear_forward(x, w8, w_s, A_TOK, None, None) for _ in range(2)]
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert err.count('[llmc_amd] i8_linear') == 1 and '16' in err, err
    codes, a_s = I8.i8_act_quant(x, A_TOK)
    want = hip_linear(I8.i8_dequant(codes, a_s, x.dtype), I8.i8_dequant(w8, w_s, x.dtype), None)
    assert_same(y[0], want.cpu(), 'fallback')
    assert_same(y[1], want.cpu(), 'fallback, second call')


def layer_reference(m, codes, a_s, dtype):
    K = codes.shape[-1]
    y = reference(codes.reshape(-1, K).cpu().numpy(), m.weight.cpu().numpy(), a_s.reshape(-1).cpu().numpy(),
                  m.weight_scale.float().reshape(-1).cpu().numpy(), {v: k for k, v in TDT.items()}[dtype],
                  None if m.bias is None else m.bias.cpu())
    return y.reshape(*codes.shape[:-1], -1)


@pytest.mark.parametrize('cls_name', ['VllmRealQuantLinear', 'SglRealQuantLinear'])
@pytest.mark.parametrize('in_f,out_f,bias', [(256, 130, True), (208, 16, False)])
def test_layer_forward(cls_name, in_f, out_f, bias):
    from llmc_amd.compression.quantization import i8_linear_ops as I8
    from llmc_amd.compression.quantization import module_utils as MU
    from llmc_amd.compression.quantization.quant import IntegerQuantizer
    cls = getattr(MU, cls_name)
    g = torch.Generator().manual_seed(in_f)
    lin = torch.nn.Linear(in_f, out_f, bias=bias)
    lin.weight.data = torch.randn(out_f, in_f, generator=g) * 0.05
    lin = lin.to(torch.bfloat16).cuda()
    x = (torch.randn(2, 9, in_f, generator=g) * torch.exp(0.5 * torch.randn(in_f, generator=g))).to(torch.bfloat16).cuda()
    for w_cfg, a_cfg, mode in ((W_CH, A_TOK, 'dynamic_per_token'), (W_T, A_STATIC, 'static_per_tensor')):
        wq, aq = IntegerQuantizer(**w_cfg), IntegerQuantizer(**a_cfg)
        if mode == 'static_per_tensor':
            lin.register_buffer('buf_act_scales_0', (x.float().abs().max() / 127.0).reshape(()))
        m = cls.new(lin, lambda mod: wq.real_quant_weight_dynamic(mod.weight.data), {'weight': w_cfg, 'act': a_cfg})
        assert m.weight.dtype == torch.int8 and m.act_mode == mode and m.weight_scale.numel() == (out_f if w_cfg is W_CH else 1)
        y = m(x)
        codes, a_s = I8.i8_act_quant(x, a_cfg, m.input_scale if mode == 'static_per_tensor' else None)
        assert codes.dtype == torch.int8 and codes.shape == x.shape and a_s.dtype == torch.float32
        assert tuple(a_s.shape) == ((2, 9, 1) if mode == 'dynamic_per_token' else (1,))
        assert y.dtype == x.dtype and tuple(y.shape) == (2, 9, out_f)
        assert_same(y, I8.i8_scaled_gemm(codes, a_s, m.weight, m.weight_scale, dtype=x.dtype, bias=m.bias).cpu(), (mode, 'forward vs its parts'))
        assert_same(y, layer_reference(m, codes, a_s, x.dtype), (mode, 'forward vs numpy'))
        # code * scale is the fake-quant activation (equal as numbers: an integer code has no negative zero)
        if mode == 'dynamic_per_token':
            fake = aq.fake_quant_act_dynamic(x)
        else:
            fake = aq.fake_quant_act_static(x, {'scales': lin.buf_act_scales_0, 'zeros': torch.tensor(0.0), 'qmax': aq.qmax, 'qmin': aq.qmin})
        deq = I8.i8_dequant(codes, a_s, x.dtype)
        assert torch.equal(deq, fake) and torch.equal(deq.view(torch.int16)[fake != 0], fake.view(torch.int16)[fake != 0])


class Cfg(dict):
    __getattr__ = dict.get


def test_rtn_w8a8_deployed_model_runs_bit_exactly():
    """RTN with the rtn_w8a8 quant section, deploy('vllm_quant'), then the model runs. Every deployed Linear is compared, on the
    input it actually received in that run, with the numpy arithmetic."""
    import llmc_amd.compression.quantization as Q
    from llmc_amd.compression.quantization import i8_linear_ops as I8
    from toy_model import ToyModel, calib_input
    model = ToyModel()
    inp = calib_input(model)
    qc = Cfg(method='RTN', weight=Cfg(W_CH), act=Cfg(A_TOK))
    algo = Q.RTN(model, qc, inp, None, Cfg(calib=Cfg(seq_len=64), model=Cfg(type='Toy')))
    algo.run_block_loop()
    algo.deploy('vllm_quant', keep_device=True)
    seen, hooks = [], []
    for blk in model.get_blocks():
        blk.cuda()
        for name in ('gate_proj', 'up_proj', 'down_proj'):
            m = getattr(blk, name)
            assert type(m).__name__ == 'VllmRealQuantLinear' and m.weight.dtype == torch.int8 and m.act_mode == 'dynamic_per_token'
            hooks.append(m.register_forward_hook(lambda mod, args, out: seen.append((mod, args[0].detach().clone(), out.detach().clone()))))
    x = inp['data'][0].cuda()
    with torch.no_grad():
        for blk in model.get_blocks():
            x = blk(x)
    for h in hooks:
        h.remove()
    assert len(seen) == 6 and bool(torch.isfinite(x).all())
    for m, xin, out in seen:
        codes, a_s = I8.i8_act_quant(xin, m.act_cfg)
        assert_same(out, layer_reference(m, codes, a_s, xin.dtype), tuple(m.weight.shape))
