"""tests/fp4_oracle.py against the reference's own output (tests/golden/fp4.npz, written by tools/make_golden_fp4.py) and the
properties of the two grids. No GPU."""
import numpy as np
import pytest

import fp4_oracle as O
from oracle import quant_ref as Q

E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def cases(golden):
    g = golden('fp4')
    return g, [str(n) for n in g['names']]


def rows_of(g, n):
    """(x as the [G, g] view the quantizer reduces over, dt, bit, meta)"""
    dt, bit, gran = str(g[n + '/dt']), str(g[n + '/bit']), str(g[n + '/gran'])
    gs = int(g[n + '/meta'][3])
    x = O.from_bits16(g[n + '/x_bits'], dt)
    if gran == 'per_group':
        x2 = x.reshape(-1, gs)
    elif gran == 'per_tensor':
        x2 = x.reshape(1, -1)
    else:
        x2 = x.reshape(-1, x.shape[-1])
    return x, x2, dt, bit


def test_oracle_reproduces_every_golden_array(golden):
    g, names = cases(golden)
    assert len(names) == 8
    for n in names:
        x, x2, dt, bit = rows_of(g, n)
        kind = str(g[n + '/kind'])
        sdt = {'torch.bfloat16': 'bf16', 'torch.float16': 'f16', 'torch.float32': 'f32'}[str(g[n + '/scales_dtype'])]
        if kind == 'act_static':
            assert sdt == 'f32'
            r = O.run(x2, dt, bit, scales=g[n + '/scales'], sdt=sdt)
        else:
            assert sdt == dt, n                     # the integer qmax never promotes, per_tensor included
            r = O.run(x2, dt, bit)
            assert np.array_equal(r['scales_raw'].reshape(-1).view(np.uint32), g[n + '/scales'].view(np.uint32)), n
        assert np.array_equal(O.bits16(r['fake'], dt).reshape(-1), g[n + '/fake_bits'].reshape(-1)), n
        assert np.array_equal(r['values'].reshape(-1).view(np.uint32), g[n + '/q'].reshape(-1).view(np.uint32)), n
        if n + '/static_scales' in g.files:
            rs = O.run(x2, dt, bit, scales=g[n + '/static_scales'], sdt=dt)
            assert np.array_equal(O.bits16(rs['fake'], dt).reshape(-1), g[n + '/static_fake_bits'].reshape(-1)), n


def test_the_zero_row_case_keeps_a_representable_scale(golden):
    """An all-zero row: absmax.clamp(1e-5) / 6 = 1.67e-6 is still an fp16 subnormal (the FP8 formats' / 448 underflows to 0 and
    becomes 1, quant.py:1062; the narrow formats' does not), and the row quantizes to zeros. The 0 -> 1 rule itself is pinned
    on given scales."""
    g, _ = cases(golden)
    s = g['e2m1_g128_f16_zero_row/scales']
    expect = Q.rnd(Q.rnd(np.float32(1e-5), 'f16') / np.float32(6.0), 'f16')
    assert (s == expect).sum() == 3 and expect > 0 and (s != 0).all()
    x, x2, dt, bit = rows_of(g, 'e2m1_g128_f16_zero_row')
    r = O.run(x2, dt, bit, scales=np.zeros((x2.shape[0], 1), np.float32), sdt=dt)
    r1 = O.run(x2, dt, bit, scales=np.ones((x2.shape[0], 1), np.float32), sdt=dt)
    assert (r['scales'] == 1).all() and np.array_equal(r['fake'], r1['fake'])


def test_value_sets():
    sweep = np.linspace(-40, 40, 160001).astype(np.float32)
    q = np.unique(np.abs(O.quantize(sweep, 'e2m1', 'qtorch')))
    assert q.tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0]                 # 11 signed levels: the top exponent code is infinity's
    assert len(np.unique(O.quantize(sweep, 'e2m1', 'qtorch'))) == 11
    assert np.abs(O.quantize(sweep, 'e3m2', 'qtorch')).max() == 14.0
    o = np.unique(O.quantize(sweep, 'e2m1', 'ocp'))
    assert len(o) == 15 and np.unique(np.abs(o)).tolist() == E2M1
    o6 = np.unique(O.quantize(sweep, 'e3m2', 'ocp'))
    assert len(o6) == 63 and o6.max() == 28.0 and np.unique(np.abs(o6))[1] == 0.0625
    assert O.ocp_values('e2m1').tolist() == E2M1
    # every qtorch result is a member of the OCP grid
    assert set(np.unique(np.abs(O.quantize(sweep, 'e3m2', 'qtorch'))).tolist()) <= set(O.ocp_values('e3m2').tolist())


@pytest.mark.parametrize('bit,n', [('e2m1', 16), ('e3m2', 64)])
def test_encode_decode_round_trip(bit, n):
    codes = np.arange(n, dtype=np.uint8)
    v = O.decode(codes, bit)
    assert np.array_equal(O.encode(v, bit), codes)
    assert np.signbit(v[n // 2]) and v[n // 2] == 0                     # the sign bit alone is -0
    assert v[n // 2 - 1] == O.FORMATS[bit][2] and v[n - 1] == -O.FORMATS[bit][2]
    assert np.array_equal(O.quantize(v, bit, 'ocp').view(np.uint32), v.view(np.uint32))      # grid points are fixed points


def test_ties():
    t = np.array([0.25, 2.5, 5.0, -0.25, -2.5, 0.75, 1.75, 3.5], np.float32)
    assert O.quantize(t, 'e2m1', 'ocp').tolist() == [0.0, 2.0, 4.0, -0.0, -2.0, 1.0, 2.0, 4.0]     # to the even code
    assert np.signbit(O.quantize(t, 'e2m1', 'ocp')[3])
    assert O.quantize(t[:2], 'e2m1', 'qtorch').tolist() == [0.5, 3.0]                          # away from zero
    assert O.quantize(np.array([5.0, 1e9, -np.inf], np.float32), 'e2m1', 'qtorch').tolist() == [3.0, 3.0, -3.0]
    sat = O.quantize(np.array([7.0, np.inf, -np.inf, np.nan, -np.nan], np.float32), 'e2m1', 'ocp')
    assert sat[:3].tolist() == [6.0, 6.0, -6.0] and abs(sat[3]) == 6.0 and sat[3] == -sat[4]


def test_e8m0_rule():
    a = np.array([0.0, 1.0, 4.0, 3.999, 6.0, 0.75, 2.0 ** -130, 2.0 ** 127], np.float32)
    c = O.e8m0_codes(a, 'e2m1')
    assert c.tolist() == [127, 125, 127, 126, 127, 124, 0, 252]
    assert O.e8m0_values(np.array([127, 0, 254])).tolist() == [1.0, 2.0 ** -127, 2.0 ** 127]
    assert O.e8m0_codes(np.array([16.0, 28.0, 15.9]), 'e3m2').tolist() == [127, 127, 126]


def test_packing():
    c = np.array([[1, 2, 0xf, 0], [7, 8, 9, 0xa]], np.uint8)
    assert O.pack_fp4(c).tolist() == [[0x21, 0x0f], [0x87, 0xa9]]


def test_qtorch_path_is_the_oracle_function_unchanged():
    x = np.random.default_rng(0).standard_normal(1000).astype(np.float32) * 3
    assert np.array_equal(O.quantize(x, 'e2m1', 'qtorch'), Q.qtorch_float_quantize(x, 2, 1))
