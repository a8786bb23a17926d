"""tests/kvquant_oracle.py equals the reference's NaiveQuantKVCache / KiviQuantKVCache as recorded in tests/golden/kvquant.npz
(tools/make_golden_kvquant.py) bit for bit: what every update() returned and the codes and qparams it left, on every step."""
import numpy as np
import pytest

import kvquant_oracle as KO
from conftest import load_golden

G = load_golden('kvquant')
NAMES = [str(n) for n in G['names']]


def same_bits(got, want_bits, dt, what):
    """`got`: float32 values; `want_bits`: recorded bit patterns (uint32 where the reference holds fp32)."""
    got_bits = KO.to_bits(got, 'f32' if want_bits.dtype == np.uint32 else dt)
    assert got_bits.shape == want_bits.shape, (what, got_bits.shape, want_bits.shape)
    assert np.array_equal(got_bits, want_bits), (what, int((got_bits != want_bits).sum()))


def test_the_goldens_cover_what_they_should():
    assert len(NAMES) == 14
    assert sum(n.startswith('kivi_') for n in NAMES) == 2 and sum('_b2_d128' in n for n in NAMES) == 2
    rows = [int(r) for r in G['kivi_bf16_w4asym_g32/rows']]
    assert rows == [5, 5, 5, 5, 9, 9, 9, 9, 13]          # two flushes
    # a stored code re-derived from its own dequantized value is not always the same code: the goldens can tell a cache that
    # skips the requantization from one that does it
    changed = 0
    for name in NAMES:
        if '_bf16_' not in name or name.startswith('kivi_'):
            continue
        prev = None
        for st in KO.golden_steps(G, name):
            if prev is not None:
                changed += int((st['k_q'][:, :, :prev.shape[2]] != prev).sum())
            prev = st['k_q']
    assert changed > 0


@pytest.mark.parametrize('name', NAMES)
def test_oracle_equals_the_reference_on_every_step(name):
    dt = KO.case_dt(name)
    cache = KO.from_meta(dt, G[name + '/meta'])
    for s, st in enumerate(KO.golden_steps(G, name)):
        k, v = cache.update(KO.as_f32(st['k_in'], dt), KO.as_f32(st['v_in'], dt))
        same_bits(k, st['k_out'], dt, (s, 'k_out'))
        same_bits(v, st['v_out'], dt, (s, 'v_out'))
        for t, is_key in (('k', True), ('v', False)):
            d = cache.quantized(is_key)
            assert d['q_tensor'].shape == st[t + '_q'].shape
            assert np.array_equal(d['q_tensor'], st[t + '_q'].astype(np.float32)), (s, t, 'codes')
            same_bits(d['scales'], st[t + '_scales'], dt, (s, t, 'scales'))
            same_bits(d['zeros'], st[t + '_zeros'], dt, (s, t, 'zeros'))
