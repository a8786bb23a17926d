"""NaiveQuantKVCache / KiviQuantKVCache on the GPU (llmc_amd/compression/quantization/kvquant.py, llmc_kv_cache_update): the
reference's bits on every step of tests/golden/kvquant.npz, and tests/kvquant_oracle.py's (pinned to those goldens by
test_kvquant_oracle.py) at the shapes where the kernel takes another route: several groups per row, rows wider than a sub-wave,
row counts that do not fill a wave's row sets, growth of the store, several new rows, strided input, clamped scales, keys
alone. What the kernel refuses runs composed and must equal the same sequence of the quantizer's public calls."""
import copy

import numpy as np
import pytest
import torch

import kvquant_oracle as KO
from conftest import load_golden

pytestmark = pytest.mark.gpu

G = load_golden('kvquant')
NAMES = [str(n) for n in G['names']]
TDT = {'bf16': torch.bfloat16, 'f16': torch.float16}


def dev_tensor(bits, dt):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(TDT[dt]).cuda()


def bits_of(t):
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32)
    return t.view(torch.int16).numpy().view(np.uint16)


def make_cache(method, initial_capacity=4, **cfg):
    from llmc_amd.compression.quantization import kvquant  # noqa: F401
    from llmc_amd.utils.registry_factory import KV_REGISTRY
    quant_type = cfg.pop('quant_type', 'int-quant')
    return KV_REGISTRY[method](quant_type, dict(cfg, method=method), 1, initial_capacity=initial_capacity)


def cfg_of(meta):
    bit, sym, gran, group, B, H, T0, D, steps, kivi, resid = (int(x) for x in meta)
    cfg = dict(bit=bit, symmetric=bool(sym), granularity=KO.GRAN[gran])
    if gran == 1:
        cfg['group_size'] = group
    if kivi:
        cfg['residual_length'] = resid
    return ('Kivi' if kivi else 'Naive'), cfg


def check_quantized(cache, want, dt, what, from_golden):
    """cache.quantized(0, .) against the reference's dict: `want` holds bit patterns (goldens) or float32 values (oracle)."""
    for t, is_key in (('k', True), ('v', False)):
        d = cache.quantized(0, is_key)
        q, s, z = d['q_tensor'], d['scales'], d['zeros']
        wq, ws, wz = (want[t + '_q'], want[t + '_scales'], want[t + '_zeros']) if from_golden else \
            (want[t]['q_tensor'], want[t]['scales'], want[t]['zeros'])
        assert q.dtype == TDT[dt] and tuple(q.shape) == tuple(wq.shape), (what, t, q.dtype, q.shape)
        assert np.array_equal(q.float().cpu().numpy(), np.asarray(wq, np.float32)), (what, t, 'codes')
        for name, got, w in (('scales', s, ws), ('zeros', z, wz)):
            if not from_golden:
                w = KO.to_bits(w, 'f32' if np.ndim(w) == 0 else dt)       # the oracle's only 0-dim qparam here: a symmetric zero
            assert tuple(got.shape) == tuple(w.shape), (what, t, name, got.shape, w.shape)
            assert got.dtype == (torch.float32 if w.dtype == np.uint32 else TDT[dt]), (what, t, name, got.dtype)
            assert np.array_equal(bits_of(got), w), (what, t, name)


@pytest.mark.parametrize('name', NAMES)
def test_every_step_of_the_goldens_bit_for_bit(name):
    dt = KO.case_dt(name)
    method, cfg = cfg_of(G[name + '/meta'])
    cache = make_cache(method, **cfg)
    for s, st in enumerate(KO.golden_steps(G, name)):
        k, v = cache.update(dev_tensor(st['k_in'], dt), dev_tensor(st['v_in'], dt), 0, {})
        assert k.dtype == v.dtype == TDT[dt] and tuple(k.shape) == st['k_out'].shape
        assert np.array_equal(bits_of(k), st['k_out']), (s, 'k_out')
        assert np.array_equal(bits_of(v), st['v_out']), (s, 'v_out')
        check_quantized(cache, st, dt, (name, s), True)
        assert cache.get_seq_length() == int(G[name + '/meta'][6]) + s
    # the kernel ran wherever it can: a quiet fall-back to the composed path would pass the comparison too
    assert cache._layers[0].fused is (cfg['granularity'] != 'per_tensor')


def states(gen, B, H, n, D, dt, strided=False):
    if strided:         # what attention hands over: [B, T, H, D].transpose(1, 2)
        x = torch.randn(B, n, H, D, generator=gen) * torch.exp(0.7 * torch.randn(1, 1, H, D, generator=gen))
        return x.to(TDT[dt]).cuda().transpose(1, 2)
    x = torch.randn(B, H, n, D, generator=gen) * torch.exp(0.7 * torch.randn(1, H, 1, D, generator=gen))
    return x.to(TDT[dt]).cuda()


def run_against_oracle(dt, method, cfg, B, H, D, new_rows, seed, initial_capacity=4, strided=False, edit=None, fused=True):
    gen = torch.Generator().manual_seed(seed)
    cache = make_cache(method, initial_capacity=initial_capacity, **cfg)
    oracle = KO.OracleKVCache(dt, cfg['bit'], cfg['symmetric'], cfg['granularity'], cfg.get('group_size'), method,
                              cfg.get('residual_length', 128))
    for s, n in enumerate(new_rows):
        k, v = states(gen, B, H, n, D, dt, strided), states(gen, B, H, n, D, dt, strided)
        if edit is not None:
            edit(s, k, v)
        ko, vo = cache.update(k, v, 0, {})
        wk, wv = oracle.update(k.float().cpu().numpy(), v.float().cpu().numpy())
        assert tuple(ko.shape) == wk.shape and ko.dtype == TDT[dt]
        assert np.array_equal(bits_of(ko), KO.to_bits(wk, dt)), (s, 'k_out')
        assert np.array_equal(bits_of(vo), KO.to_bits(wv, dt)), (s, 'v_out')
        check_quantized(cache, {'k': oracle.k, 'v': oracle.v}, dt, s, False)
    assert cache._layers[0].fused is fused
    return cache


A4 = dict(bit=4, symmetric=False, granularity='per_group')


@pytest.mark.parametrize('dt', ['bf16', 'f16'])
@pytest.mark.parametrize('group', [128, 64, 32])
def test_d128_with_one_two_and_four_groups_per_row(dt, group):
    run_against_oracle(dt, 'Naive', dict(A4, group_size=group), 1, 2, 128, [5, 1, 1, 1], seed=group)


@pytest.mark.parametrize('dt', ['bf16', 'f16'])
def test_d256_per_token(dt):
    run_against_oracle(dt, 'Naive', dict(bit=8, symmetric=True, granularity='per_token'), 1, 2, 256, [6, 1, 1], seed=7)


@pytest.mark.parametrize('T0', [1, 7])
@pytest.mark.parametrize('sym', [True, False])
def test_three_heads_ragged_row_counts_growth_and_three_new_rows(T0, sym):
    # B * H = 3 and T0 = 1 / 7: the row count is no multiple of the rows of a wave; initial_capacity 4 doubles mid-sequence
    # (T0 = 1: at 5 and 9 rows; T0 = 7: at the prefill and at 9); the third step appends 3 rows at once
    cache = run_against_oracle('bf16', 'Naive', dict(bit=8, symmetric=sym, granularity='per_token'), 1, 3, 64,
                               [T0, 1, 3, 1, 1, 1, 1, 1], seed=11 + T0, initial_capacity=4)
    assert cache._layers[0].k.cap == 16 and cache._layers[0].T == T0 + 9


def test_kivi_flushes_growth_and_group_quantization():
    cache = run_against_oracle('bf16', 'Kivi', dict(A4, group_size=32, residual_length=3), 2, 2, 64, [3, 1, 1, 1, 1, 2, 1, 1],
                               seed=5, initial_capacity=4)
    assert cache._layers[0].T == 3 + 3 + 4 and cache._layers[0].k.cap == 16     # flushes at the 4th and 7th update


@pytest.mark.parametrize('method', ['Naive', 'Kivi'])
def test_the_strided_view_of_attention_equals_its_contiguous_copy(method):
    cfg = dict(bit=8, symmetric=False, granularity='per_token', residual_length=2)
    a = run_against_oracle('bf16', method, dict(cfg), 2, 2, 64, [5, 1, 1, 1], seed=3, strided=True)
    gen = torch.Generator().manual_seed(3)
    b = make_cache(method, **cfg)
    for n in [5, 1, 1, 1]:
        k, v = states(gen, 2, 2, n, 64, 'bf16', True), states(gen, 2, 2, n, 64, 'bf16', True)
        assert not k.is_contiguous() or n == 1
        kb, vb = b.update(k.contiguous(), v.contiguous(), 0, {})
    for is_key in (True, False):
        da, db = a.quantized(0, is_key), b.quantized(0, is_key)
        assert all(torch.equal(da[x], db[x]) for x in ('q_tensor', 'scales', 'zeros'))


@pytest.mark.parametrize('dt', ['bf16', 'f16'])
@pytest.mark.parametrize('sym', [True, False])
def test_a_constant_row_and_an_all_zero_row(dt, sym):
    def edit(s, k, v):
        if s == 0:
            k[0, 0, 1, :] = 0.0173          # max == min: the asymmetric scale is clamp(1e-5) / (qmax - qmin)
            k[0, 1, 0, :] = 0.0             # all zero: both scales clamped
            v[0, 1, 2, :] = -3.0
        else:
            v[0, 0, 0, :] = 0.0
    run_against_oracle(dt, 'Naive', dict(bit=8, symmetric=sym, granularity='per_token'), 1, 2, 64, [4, 1, 1], seed=13, edit=edit)
    run_against_oracle(dt, 'Naive', dict(bit=4, symmetric=sym, granularity='per_group', group_size=32), 1, 2, 64, [4, 1, 1],
                       seed=14, edit=edit)


def test_keys_and_values_of_one_update_equal_two_keys_only_updates():
    cfg = dict(A4, group_size=32)
    both, ks, vs = make_cache('Naive', **cfg), make_cache('Naive', **cfg), make_cache('Naive', **cfg)
    gen = torch.Generator().manual_seed(17)
    for n in [5, 1, 1, 1, 1]:
        k, v = states(gen, 1, 2, n, 64, 'bf16'), states(gen, 1, 2, n, 64, 'bf16')
        ko, vo = both.update(k, v, 0, {})
        k1, none1 = ks.update(k, None, 0, {})
        v1, none2 = vs.update(v, None, 0, {})
        assert none1 is None and none2 is None
        assert torch.equal(ko.view(torch.int16), k1.view(torch.int16)) and torch.equal(vo.view(torch.int16), v1.view(torch.int16))
    for x in ('q_tensor', 'scales', 'zeros'):
        assert torch.equal(both.quantized(0, True)[x], ks.quantized(0, True)[x])
        assert torch.equal(both.quantized(0, False)[x], vs.quantized(0, True)[x])


# ---- what the kernel refuses runs composed ------------------------------------------------------------------------------------------
def composed_sequence(q, steps, int_quant):
    """The reference's Naive update (kvquant.py:44-87, 136-186) as calls of the quantizer's public methods."""
    def quantize(t):
        shape = t.shape
        t = q.reshape_tensor(t)
        scales, zeros, qmax, qmin = q.get_qparams(q.get_tensor_range(t, {}), t.device)
        codes = q.quant(t, scales, zeros, qmax, qmin)
        if int_quant:
            codes = codes.to(torch.result_type(t, scales))
        return q.restore_tensor(codes, shape), scales, zeros

    def dequantize(codes, scales, zeros):
        shape = codes.shape
        return q.restore_tensor(q.dequant(q.reshape_tensor(codes), scales, zeros), shape)

    store, outs = None, []
    for k in steps:
        if store is None:
            store = quantize(k.contiguous())
            outs.append(dequantize(*store))
        else:
            outs.append(torch.cat([dequantize(*store), k], dim=-2))
            store = quantize(outs[-1].contiguous())
    return outs, store


@pytest.mark.parametrize('case', ['d80', 'round_zp_false', 'e4m3'])
def test_the_composed_path_equals_the_same_sequence_of_public_quantizer_calls(case):
    D = 80 if case == 'd80' else 64
    cfg = {'d80': dict(bit=8, symmetric=False, granularity='per_token'),
           'round_zp_false': dict(bit=8, symmetric=False, granularity='per_token', round_zp=False),
           'e4m3': dict(bit='e4m3', symmetric=True, granularity='per_token', use_qtorch=True, quant_type='float-quant')}[case]
    if case == 'd80':          # the integer arithmetic has an oracle at any width
        run_against_oracle('bf16', 'Naive', dict(cfg), 1, 2, 80, [5, 1, 1], seed=19, fused=False)
    cache = make_cache('Naive', **dict(cfg))
    gen = torch.Generator().manual_seed(23)
    ks = [states(gen, 1, 2, n, D, 'bf16') for n in (5, 1, 1)]
    vs = [states(gen, 1, 2, n, D, 'bf16') for n in (5, 1, 1)]
    got = [cache.update(k, v, 0, {}) for k, v in zip(ks, vs)]
    assert cache._layers[0].fused is False
    for is_key, xs in ((True, ks), (False, vs)):
        outs, store = composed_sequence(cache.kvquantizer, xs, case != 'e4m3')
        for s, o in enumerate(outs):
            g = got[s][0 if is_key else 1]
            assert g.dtype == o.dtype and torch.equal(g, o), (case, is_key, s)
        d = cache.quantized(0, is_key)
        assert torch.equal(d['q_tensor'], store[0]) and torch.equal(d['scales'], store[1])
        assert torch.equal(d['zeros'].cpu(), store[2].cpu())


def test_refusals_of_the_kernel_leave_the_store_untouched():
    """LLMC_EINVAL / LLMC_ENOTSUP are answered before anything is launched."""
    from llmc_amd import _ffi
    L = _ffi.lib()
    codes = torch.zeros(2, 8, 64, dtype=torch.uint8, device='cuda')
    sc = torch.ones(2, 8, 1, dtype=torch.bfloat16, device='cuda')
    zr = torch.zeros(2, 8, 1, dtype=torch.bfloat16, device='cuda')
    new = torch.ones(1, 2, 1, 64, dtype=torch.bfloat16, device='cuda')
    out = torch.empty(1, 2, 5, 64, dtype=torch.bfloat16, device='cuda')

    def call(T_old=4, n_new=1, cap=8, D=64, g=64, sym=0, round_zp=1, qmin=0.0, qmax=255.0, flags=_ffi.KV_REQUANT, zeros=zr,
             strides=(128, 64, 64)):
        return L.llmc_kv_cache_update(_ffi.BF16, 1, 2, T_old, n_new, cap, D, g, sym, round_zp, qmin, qmax, flags, _ffi.ptr(codes),
                                      _ffi.ptr(sc), _ffi.ptr(zeros), _ffi.ptr(new), _ffi.ptr(out), 0, 0, 0, 0, 0, *strides,
                                      _ffi.stream())
    assert call(cap=4) == -22                                   # REQUANT writes row 4 of a store of 4
    assert call(flags=_ffi.KV_NEW_FAKE) == -22                  # NEW_FAKE needs REQUANT
    assert call(zeros=None) == -22 and call(sym=1) == -22       # zeros exactly when asymmetric
    assert call(g=48) == -22                                    # D % g
    assert call(round_zp=0) == -95
    assert call(qmax=65535.0) == -95                            # bit > 8
    assert call(D=48, g=48, strides=(96, 48, 48)) == -95        # 6 lanes: not a power of two
    assert call(strides=(128, 64, 36)) == -95                   # rows not 16-byte aligned
    torch.cuda.synchronize()
    assert int(codes.sum()) == 0 and bool((sc == 1).all())


# ---- one decoder layer through the hook -------------------------------------------------------------------------------------------
class OracleBackedCache:
    """update() of the CPU oracle behind the cache interface an attention module calls."""

    def __init__(self, dt, **cfg):
        self.dt = dt
        self.oracle = KO.OracleKVCache(dt, cfg['bit'], cfg['symmetric'], cfg['granularity'], cfg.get('group_size'))

    def get_seq_length(self, layer_idx=0):
        return self.oracle.seen

    def update(self, key_states, value_states, layer_idx, *args, **kwargs):
        k, v = self.oracle.update(key_states.float().cpu().numpy(), value_states.float().cpu().numpy())
        back = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(key_states.dtype).to(key_states.device)  # noqa: E731
        return back(k), back(v)


def test_a_llama_decoder_layer_through_the_hook_equals_an_oracle_backed_cache():
    import llmc_amd.compression.quantization as Q
    from toy_model import ToyModel, calib_input
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import LlamaDecoderLayer, LlamaRotaryEmbedding

    config = LlamaConfig(hidden_size=128, num_attention_heads=2, num_key_value_heads=2, intermediate_size=256,
                         num_hidden_layers=1, vocab_size=32, max_position_embeddings=64)
    config._attn_implementation = 'eager'
    torch.manual_seed(0)
    layer = LlamaDecoderLayer(config, 0).to(torch.bfloat16).cuda().eval()
    rotary = LlamaRotaryEmbedding(config).cuda()
    kv = dict(method='Naive', bit=8, symmetric=True, granularity='per_token')
    runs = []
    for oracle_backed in (False, True):
        model = ToyModel()
        algo = Q.RTN(model, {'method': 'RTN', 'weight': dict(bit=8, symmetric=True, granularity='per_channel'), 'kvcache': dict(kv)},
                     calib_input(model), None, {})
        if oracle_backed:
            algo.kv_module = OracleBackedCache('bf16', **kv)
        blk = copy.deepcopy(layer)
        algo.register_kv_cache(blk)
        gen = torch.Generator().manual_seed(29)
        outs, pos = [], 0
        for n in (5, 1, 1):
            x = torch.randn(1, n, 128, generator=gen).to(torch.bfloat16).cuda()
            position_ids = torch.arange(pos, pos + n, device='cuda').unsqueeze(0)
            with torch.no_grad():
                y = blk(x, position_ids=position_ids, position_embeddings=rotary(x, position_ids), use_cache=True)
            outs.append(y[0] if isinstance(y, tuple) else y)
            pos += n
        runs.append(outs)
        if not oracle_backed:
            assert algo.kv_module._layers[0].fused and algo.kv_module._layers[0].T == 7
    for a, b in zip(*runs):
        assert a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))
