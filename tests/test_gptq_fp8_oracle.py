"""tests/gptq_fp8_oracle.py (the numpy restatement the GPU tests check large shapes against) reproduces the reference's GPTQ
with a FloatQuantizer, bit for bit, on every case of tests/golden/gptq_fp8.npz (tools/make_golden_gptq_fp8.py): tmp, losses,
group scales and the running W. No GPU."""
import numpy as np
import pytest

from conftest import load_golden

import gptq_fp8_oracle as O
from gptq_fp8_oracle import bits

GOLD = load_golden('gptq_fp8')
CASES = [str(n) for n in GOLD['names']]


def case_inputs(case):
    return O.case_inputs(GOLD, case)


def test_the_golden_has_the_cases_the_loop_must_cover():
    metas = {c: GOLD[c + '/meta'] for c in CASES}
    bit = {c: str(GOLD[c + '/bit']) for c in CASES}
    assert {bit[c] for c in CASES} == {'e4m3', 'e5m2'}
    assert any(m[2] == 0 and m[3] == 1 for m in metas.values())                    # per_channel with actorder (the shipped file)
    assert any(m[2] > 0 and m[4] == 1 for m in metas.values())                     # static groups
    assert any(m[2] in (16, 32, 64) and m[4] == 0 for m in metas.values())         # groups that start mid-block
    assert any(m[6] % 128 for m in metas.values())                                 # a partial last block
    assert any((GOLD[c + '/rtn_scales'] == 0).any() for c in CASES)                # a scale that underflowed to 0
    assert 'e5m2_g128_noact_dyn_bf16_outliers' in CASES                            # the case that reaches e5m2's saturation


@pytest.mark.parametrize('case', CASES)
def test_oracle_reproduces_the_reference(case):
    p = case + '/'
    Wp, U, fmt, gs, static_groups, col_group, scales = case_inputs(case)
    r = O.weight_transform(Wp, U, fmt, gs, static_groups, col_group, scales)
    np.testing.assert_array_equal(bits(r['tmp']), bits(GOLD[p + 'tmp']), err_msg=case + ' tmp')
    np.testing.assert_array_equal(bits(r['losses']), bits(GOLD[p + 'losses']), err_msg=case + ' losses')
    np.testing.assert_array_equal(bits(r['W']), bits(GOLD[p + 'W_after']), err_msg=case + ' running W')
    sc = r['scales']
    if scales is not None:
        sc = np.where(sc == 0, np.float32(1.0), sc)        # quant.py:1062 acts in place on the qparams the loop holds
    np.testing.assert_array_equal(bits(sc), bits(GOLD[p + 'g_scales']), err_msg=case + ' group scales')
    # the saturation arm is exercised against the reference: e4m3's in every case (the scale maps the range to +-448, the grid
    # ends at 240: every |w / s| >= 248 lands there); e5m2's only beyond the range its scale was taken from (|w / s| >= 61440
    # rounds past 57344), which the outlier case reaches through its strong upper factor
    if fmt == 'e4m3':
        assert r['t_absmax'] >= 248.0
    if case == 'e5m2_g128_noact_dyn_bf16_outliers':
        assert r['t_absmax'] >= 61440.0


def test_rows_are_independent():
    case = CASES[2]
    Wp, U, fmt, gs, static_groups, col_group, scales = case_inputs(case)
    rows = [1, 5, 14]
    r = O.weight_transform(Wp[rows], U, fmt, gs, static_groups, col_group, None if scales is None else scales[rows])
    np.testing.assert_array_equal(bits(r['tmp']), bits(GOLD[case + '/tmp'][rows]))
    np.testing.assert_array_equal(bits(r['scales']), bits(GOLD[case + '/g_scales'][rows]))
