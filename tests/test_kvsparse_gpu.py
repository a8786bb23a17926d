"""SinkKVCache on the GPU (llmc_amd/compression/sparsification/kvsparse.py, llmc_kv_sink_update): the reference's bits on every
step of tests/golden/kvsparse.npz, and tests/kvsparse_oracle.py's (pinned to those goldens by test_kvsparse_oracle.py) at the
shapes where the kernel takes another route: rows of 8 and 16 vector pairs, columns behind the rotated ones, rows that are no
whole vectors (composed), several (b, h), windows that fill no block, no sink and almost only sink, several new rows, strided
input, a model-width window and one whose items pass the grid cap. Every step's output is compared before the next update: the
fused path returns views that live until the second following update."""
import copy

import numpy as np
import pytest
import torch

import kvsparse_oracle as SO
from conftest import load_golden

pytestmark = pytest.mark.gpu

G = load_golden('kvsparse')
NAMES = [str(n) for n in G['names']]
TDT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
EINVAL, ENOTSUP = -22, -95


def new_cache(W, sink):
    from llmc_amd.compression.sparsification.kvsparse import SinkKVCache
    return SinkKVCache(1, W, sink)


@pytest.mark.parametrize('name', NAMES)
def test_every_step_of_the_goldens_bit_for_bit(name):
    m = SO.case_meta(G, name)
    cache = new_cache(m['W'], m['sink'])
    SO.run_golden_case(G, name, cache, 'cuda')
    # the kernel ran: a quiet fall-back to the composed path would pass the comparison too
    assert cache._layers[0].fused is True


def rope_table(positions, width, dt):
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, width, 2, dtype=torch.float32) / width))
    emb = torch.outer(torch.arange(positions, dtype=torch.float32), inv_freq)
    emb = torch.cat((emb, emb), dim=-1)
    return emb.cos().to(TDT[dt]), emb.sin().to(TDT[dt])


def states(gen, B, H, n, D, dt, strided):
    if strided:         # what attention hands over: [B, T, H, D].transpose(1, 2)
        return torch.randn(B, n, H, D, generator=gen).to(TDT[dt]).cuda().transpose(1, 2)
    return torch.randn(B, H, n, D, generator=gen).to(TDT[dt]).cuda()


def run_against_oracle(dt, B, H, D, W, sink, new_rows, seed, fused=True, rope=True, partial=None, strided=False):
    gen = torch.Generator().manual_seed(seed)
    cache, oracle = new_cache(W, sink), SO.OracleSinkCache(dt, W, sink)
    width = partial or D
    cos, sin = rope_table(max(sum(new_rows), W), width, dt)
    at = 0
    for s, n in enumerate(new_rows):
        k, v = states(gen, B, H, n, D, dt, strided), states(gen, B, H, n, D, dt, strided)
        kw, okw = {}, {}
        if rope:
            c, sn = cos[at:at + n][None].expand(B, -1, -1), sin[at:at + n][None].expand(B, -1, -1)
            kw = {'cos': c.cuda(), 'sin': sn.cuda()}
            okw = {'cos': c.float().numpy(), 'sin': sn.float().numpy()}
            if partial:
                kw['partial_rotation_size'] = partial
                okw['partial'] = partial
        ko, vo = cache.update(k, v, 0, kw)
        wk, wv = oracle.update(k.float().cpu().numpy(), v.float().cpu().numpy(), **okw)
        assert tuple(ko.shape) == tuple(vo.shape) == wk.shape and ko.dtype == vo.dtype == TDT[dt], (s, ko.shape, wk.shape)
        assert np.array_equal(SO.torch_bits(ko), SO.to_bits(wk, dt)), (s, 'keys')
        assert np.array_equal(SO.torch_bits(vo), SO.to_bits(wv, dt)), (s, 'values')
        assert cache.get_seq_length() == oracle.rows
        at += n
    assert cache._layers[0].fused is fused
    return cache


# growing, the n + len == W shift that drops nothing, then shifts by 1, 2 and 1 rows (two rerotation tables)
def steps_for(W):
    return (W - 3, 1, 1, 1, 1, 2, 1)


@pytest.mark.parametrize('dt', ['bf16', 'f16'])
@pytest.mark.parametrize('D', [64, 128])
def test_d64_and_d128(dt, D):
    run_against_oracle(dt, 1, 2, D, 16, 4, steps_for(16), 1)


@pytest.mark.parametrize('D, dt, fused', [(80, 'bf16', True), (80, 'f16', True), (80, 'f32', True), (72, 'bf16', False),
                                          (72, 'f16', False), (72, 'f32', True)])
def test_d80_and_d72_take_the_path_the_kernels_refusals_imply(D, dt, fused):
    """The kernel takes rot / 2 that is whole 16-byte vectors. D = 80: 40 elements, five vectors of a 16-bit dtype, ten of fp32:
    fused. D = 72: 36 elements, four and a half vectors of a 16-bit dtype (refused at the first shift, the layer goes on composed),
    nine of fp32 (fused). The bits are the oracle's either way."""
    run_against_oracle(dt, 1, 2, D, 16, 4, steps_for(16), 2, fused=fused)


def test_d72_without_rope_is_copied_by_the_kernel():
    run_against_oracle('bf16', 1, 2, 72, 16, 4, steps_for(16), 3, rope=False)


def test_columns_behind_the_rotated_ones_pass():
    run_against_oracle('bf16', 1, 2, 128, 16, 4, steps_for(16), 4, partial=64)
    run_against_oracle('f32', 1, 2, 24, 16, 4, steps_for(16), 4, partial=8)


def test_six_heads_over_two_batches():
    run_against_oracle('bf16', 2, 3, 64, 16, 4, steps_for(16), 5)


def test_a_window_of_67_rows():
    run_against_oracle('f16', 1, 2, 64, 67, 4, steps_for(67), 6)


def test_no_sink_and_almost_only_sink():
    run_against_oracle('bf16', 1, 2, 64, 16, 0, steps_for(16), 7)
    run_against_oracle('bf16', 1, 2, 64, 16, 14, (13, 1, 1, 1, 1, 1), 7)          # one kept row: only n = 1 fits


def test_three_new_rows_and_a_prompt_longer_than_the_window():
    run_against_oracle('bf16', 1, 2, 64, 16, 4, (5, 3, 3, 3, 3, 3, 3), 8)
    run_against_oracle('bf16', 1, 2, 64, 16, 4, (21, 3, 1, 2), 8)


def test_the_strided_view_of_attention_is_read_in_place():
    run_against_oracle('bf16', 2, 2, 64, 16, 4, steps_for(16), 9, strided=True)
    run_against_oracle('f32', 1, 3, 32, 16, 4, steps_for(16), 9, strided=True)


def test_a_model_width_window():
    run_against_oracle('bf16', 1, 8, 128, 1024, 4, (1021, 1, 1, 1, 1, 2), 10)


@pytest.mark.parametrize('cap', [0, 16])
def test_a_window_whose_items_pass_the_grid_cap(cap):
    """W = 4096, B * H = 2, D = 128 in bf16: 65536 vector pairs per tensor. With the built-in cap (8 blocks of 256 lanes per CU
    over keys and values) one pass covers them; kv_sink_max_grid = 16 makes every lane grid-stride 16 times."""
    from llmc_amd import _ffi
    with _ffi.option(kv_sink_max_grid=cap):
        run_against_oracle('bf16', 1, 2, 128, 4096, 4, (4093, 1, 1, 1, 2), 11)


def test_refusals_of_the_kernel_leave_the_destination_untouched():
    """LLMC_EINVAL / LLMC_ENOTSUP are answered before anything is launched."""
    from llmc_amd import _ffi
    L = _ffi.lib()
    mk = lambda cap: torch.full((2, cap, 64), 7.0, dtype=torch.bfloat16, device='cuda')      # noqa: E731
    ks, kd, vs, vd = mk(8), mk(8), mk(8), mk(8)
    new = torch.ones(1, 2, 1, 64, dtype=torch.bfloat16, device='cuda')
    tab = torch.ones(5, 64, dtype=torch.bfloat16, device='cuda')
    P = _ffi.ptr

    def call(dt=_ffi.BF16, D=64, n_sink=2, keep_from=3, n_keep=5, n_new=1, src_cap=8, dst_cap=8, row0=0, rot=64, cos=P(tab),
             sin=P(tab), k_src=P(ks), k_dst=P(kd), k_new=P(new), v_src=P(vs), v_dst=P(vd), v_new=P(new), strides=(128, 64, 64)):
        return L.llmc_kv_sink_update(dt, 1, 2, D, n_sink, keep_from, n_keep, n_new, src_cap, dst_cap, row0, rot, cos, sin, k_src,
                                     k_dst, k_new, v_src, v_dst, v_new, *strides, _ffi.stream())
    assert call(dt=7) == EINVAL and 'dtype' in _ffi.last_error()
    assert call(k_dst=0) == EINVAL and call(k_src=0) == EINVAL and call(v_new=0) == EINVAL and call(sin=0) == EINVAL      # nulls
    assert call(rot=66) == EINVAL and call(rot=63) == EINVAL and call(rot=0) == EINVAL
    assert call(keep_from=4) == EINVAL and 'beyond' in _ffi.last_error()               # 4 + 5 rows of a source of 8
    assert call(dst_cap=7) == EINVAL and call(row0=1) == EINVAL and 'capacity' in _ffi.last_error()
    assert call(k_src=P(kd)) == EINVAL and 'in place' in _ffi.last_error()             # src == dst while rows move
    assert call(n_sink=0, n_keep=0, n_new=0) == EINVAL and call(n_keep=-1) == EINVAL
    assert call(rot=8) == ENOTSUP and 'rot / 2' in _ffi.last_error()                    # half a vector
    assert call(D=68, rot=64) == ENOTSUP                                                # a row of 8.5 vectors
    assert call(strides=(128, 64, 36)) == ENOTSUP and call(strides=(128, 68, 64)) == ENOTSUP
    assert call(k_new=P(new) + 2, v_new=P(new) + 2) == ENOTSUP and call(k_dst=P(kd) + 8) == ENOTSUP
    assert call(cos=P(tab) + 4) == ENOTSUP
    assert L.llmc_kv_sink_update(_ffi.BF16, 1 << 20, 1 << 10, 64, 0, 0, 0, 1, 0, 8, 0, 0, 0, 0, 0, P(kd), P(new), 0, P(vd), P(new),
                                 0, 0, 64, _ffi.stream()) == ENOTSUP and 'too large' in _ffi.last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in (ks, kd, vs, vd))
    # the same call with nothing wrong runs, and in place when nothing moves
    assert call() == 0
    assert call(n_sink=0, n_keep=0, keep_from=0, k_src=P(kd), v_src=P(vd), row0=7, cos=0, sin=0) == 0
    torch.cuda.synchronize()
    # sink rows copied; kept keys 7 * 1 + (-7, 7) * 1; values copied; the new row behind them
    assert bool((kd[:, :2] == 7).all()) and bool((kd[:, 2:7, :32] == 0).all()) and bool((kd[:, 2:7, 32:] == 14).all())
    assert bool((kd[:, 7] == 1).all()) and bool((vd[:, :7] == 7).all()) and bool((vd[:, 7] == 1).all())


# ---- one decoder layer through the hook -------------------------------------------------------------------------------------------
class OracleBackedCache:
    """update() of the CPU oracle behind the cache interface an attention module calls."""

    def __init__(self, dt, W, sink):
        self.dt = dt
        self.oracle = SO.OracleSinkCache(dt, W, sink)

    def get_seq_length(self, layer_idx=0):
        return self.oracle.rows

    def update(self, key_states, value_states, layer_idx, *args, **kwargs):
        k, v = self.oracle.update(key_states.float().cpu().numpy(), value_states.float().cpu().numpy())
        back = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(key_states.dtype).to(key_states.device)  # noqa: E731
        return back(k), back(v)


def test_a_llama_decoder_layer_through_dense_equals_an_oracle_backed_cache():
    import llmc_amd.compression.sparsification as S
    from toy_model import ToyModel, calib_input
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import LlamaDecoderLayer, LlamaRotaryEmbedding

    config = LlamaConfig(hidden_size=128, num_attention_heads=2, num_key_value_heads=2, intermediate_size=256,
                         num_hidden_layers=1, vocab_size=32, max_position_embeddings=64)
    config._attn_implementation = 'eager'
    torch.manual_seed(0)
    layer = LlamaDecoderLayer(config, 0).to(torch.bfloat16).cuda().eval()
    rotary = LlamaRotaryEmbedding(config).cuda()
    sparse = {'method': 'Dense', 'kvcache': {'method': 'SinkKV', 'window_length': 8, 'num_sink_tokens': 2}}
    runs = []
    for oracle_backed in (False, True):
        model = ToyModel()
        algo = S.Dense(model, copy.deepcopy(sparse), calib_input(model), None, {})
        if oracle_backed:
            algo.kv_module = OracleBackedCache('bf16', 8, 2)
        blk = copy.deepcopy(layer)
        algo.register_kv_cache(blk)
        gen = torch.Generator().manual_seed(29)
        outs, pos = [], 0
        for n in (5, 1, 1, 1, 1, 1):
            x = torch.randn(1, n, 128, generator=gen).to(torch.bfloat16).cuda()
            position_ids = torch.arange(pos, pos + n, device='cuda').unsqueeze(0)
            with torch.no_grad():
                y = blk(x, position_ids=position_ids, position_embeddings=rotary(x, position_ids), use_cache=True)
            outs.append((y[0] if isinstance(y, tuple) else y).clone())
            pos += n
        runs.append(outs)
        if not oracle_backed:
            assert algo.kv_module._layers[0].fused and algo.kv_module.get_seq_length() == 8
    for a, b in zip(*runs):
        assert a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))
