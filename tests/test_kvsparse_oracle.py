"""tests/kvsparse_oracle.py and the composed path of SinkKVCache (llmc_amd/compression/sparsification/kvsparse.py, on CPU tensors)
equal the reference's SinkKVCache as recorded in tests/golden/kvsparse.npz (tools/make_golden_kvsparse.py) bit for bit: what every
update() returned, on every step."""
import numpy as np
import pytest

import kvsparse_oracle as SO
from conftest import load_golden

G = load_golden('kvsparse')
NAMES = [str(n) for n in G['names']]


def test_the_goldens_cover_what_they_should():
    assert NAMES == ['main_bf16', 'main_f16', 'main_f32', 'prompt11_bf16', 'norope_bf16', 'partial16_bf16', 'cos2d_bf16', 'b2_bf16']
    assert [int(r) for r in G['main_bf16/rows']] == [5, 6, 7, 8, 8, 8, 8]          # growing, the shift that drops nothing, shifts
    assert [int(r) for r in G['prompt11_bf16/rows']] == [11, 8, 8]                   # stored whole, cut by the first decode step
    assert SO.case_meta(G, 'partial16_bf16')['partial'] == 16 and SO.case_meta(G, 'cos2d_bf16')['cos_dims'] == 2
    assert SO.case_meta(G, 'norope_bf16')['cos_dims'] == 0 and SO.case_meta(G, 'b2_bf16')['B'] == 2
    # a key kept over three shifts carries three roundings: one rotation of the original by the total shift gives other bits, so
    # the goldens can tell step-wise rerotation from a single one. The row appended at step 3 (place 7) ends at place 3.
    steps = list(SO.golden_steps(G, 'main_bf16'))
    cos, sin = (SO.as_f32(G['main_bf16/' + t].reshape(-1, 32), 'bf16') for t in ('cos', 'sin'))
    from oracle import quant_ref as Q
    r = lambda a: Q.rnd(a, 'bf16')          # noqa: E731
    cos_d, sin_d = r(cos[7] * cos[3] + sin[7] * sin[3]), r((-sin[7]) * cos[3] + cos[7] * sin[3])
    k0 = SO.as_f32(steps[3]['k_in'], 'bf16')[:, :, 0]
    once = r(r(k0 * cos_d) + r(np.concatenate([-k0[..., 16:], k0[..., :16]], -1) * sin_d))
    stepwise = steps[6]['k_out'][:, :, 3]
    assert int((SO.to_bits(once, 'bf16') != stepwise).sum()) > 0


@pytest.mark.parametrize('name', NAMES)
def test_oracle_equals_the_reference_on_every_step(name):
    m = SO.case_meta(G, name)
    dt = m['dt']
    oracle = SO.OracleSinkCache(dt, m['W'], m['sink'])
    for s, st in enumerate(SO.golden_steps(G, name)):
        cos = sin = None
        if st['cos'] is not None:
            cos, sin = SO.as_f32(st['cos'], dt), SO.as_f32(st['sin'], dt)
        k, v = oracle.update(SO.as_f32(st['k_in'], dt), SO.as_f32(st['v_in'], dt), cos, sin, m['partial'])
        assert k.shape == st['k_out'].shape and oracle.rows == st['rows']
        assert np.array_equal(SO.to_bits(k, dt), st['k_out']), (name, s, 'keys')
        assert np.array_equal(SO.to_bits(v, dt), st['v_out']), (name, s, 'values')


@pytest.mark.parametrize('name', NAMES)
def test_the_composed_path_on_cpu_tensors_equals_the_reference_on_every_step(name):
    from llmc_amd.compression.sparsification.kvsparse import SinkKVCache
    m = SO.case_meta(G, name)
    cache = SinkKVCache(1, m['W'], m['sink'])
    SO.run_golden_case(G, name, cache)
    assert cache._layers[0].fused is False and cache.get_max_cache_shape() == m['W']
    cache._reset_states()
    assert cache.get_seq_length() == 0 and not cache._layers
