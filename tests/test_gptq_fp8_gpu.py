"""GPTQ's column loop on FP8 grids (llmc_gptq_quantize_fp8_cols: FloatQuantizer e4m3 / e5m2 with qtorch rounding) on MI355X.
Every comparison is bit for bit.

1. The reference's own GPTQ (tests/golden/gptq_fp8.npz) through gptq_ops.gptq_quantize and through the class's per-layer flow
   (layer_transform_reference: weight_transform, update_model_qparams, w_qdq, w_q), on the default in-block path and with the
   generic path forced.
2. Shapes past the golden against tests/gptq_fp8_oracle.py (pinned to the reference by tests/test_gptq_fp8_oracle.py) on 64
   seeded rows: every launch form of the loop (512- and 1024-thread workgroups, the rider launch), both formats on the fast and
   on the generic in-block path.
3. Fast and generic path give the same tensors, with inputs that make single waves fall back.
4. The class on a toy model with the shipped gptq_fp8.yml: every deployed weight lies on the e4m3 grid qtorch rounds to.
"""
import contextlib
import copy
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from llmc_amd import _ffi
from oracle import quant_ref as Q

import gptq_fp8_oracle as O
from gptq_fp8_oracle import bits

pytestmark = pytest.mark.gpu
TD = {'f16': torch.float16, 'bf16': torch.bfloat16}
GOLD = load_golden('gptq_fp8')
CASES = [str(n) for n in GOLD['names']]


def host(t):
    return t.detach().float().cpu().numpy()


def generic_path(on):
    return _ffi.option(gptq_generic=1) if on else contextlib.nullcontext()


def run_loop(W, U, fmt, gs, static_groups, col_group, scales):
    """gptq_ops.gptq_quantize on numpy inputs -> (tmp, losses, scales) on the device"""
    from llmc_amd.compression.quantization.gptq_ops import gptq_quantize
    Wd = torch.from_numpy(np.ascontiguousarray(W, dtype=np.float32)).cuda()
    Ud = U if torch.is_tensor(U) else torch.from_numpy(U).cuda()
    cg = None if col_group is None else torch.from_numpy(col_group).cuda()
    sc = None if scales is None else torch.from_numpy(np.ascontiguousarray(scales, dtype=np.float32)).cuda()
    tmp, losses, s, z = gptq_quantize(Wd, Ud, True, 0.0, 0.0, gs, static_groups, cg, sc, None, fp8=fmt)
    assert z is None
    return tmp, losses, s


# =========================================================================================================================
# 1. the reference's GPTQ (golden)
@pytest.mark.parametrize('generic', [False, True], ids=['default', 'generic'])
@pytest.mark.parametrize('case', CASES)
def test_golden_through_gptq_quantize(case, generic):
    p = case + '/'
    Wp, U, fmt, gs, static_groups, col_group, scales = O.case_inputs(GOLD, case)
    with generic_path(generic):
        tmp, losses, s = run_loop(Wp, U, fmt, gs, static_groups, col_group, scales)
    np.testing.assert_array_equal(bits(host(tmp)), bits(GOLD[p + 'tmp']), err_msg=case + ' tmp')
    np.testing.assert_array_equal(bits(host(losses)), bits(GOLD[p + 'losses']), err_msg=case + ' losses')
    if scales is None:
        np.testing.assert_array_equal(bits(host(s)), bits(GOLD[p + 'g_scales']), err_msg=case + ' group scales')


def _golden_gptq(case):
    """A GPTQ object for a golden case without the model plumbing. Its Hessian is not part of the fixture: hessian_sorting and
    the factorisation hand out the golden's permutation, prepared weight and synthetic upper factor; everything else of the
    per-layer flow (qparam setup, weight_transform, the buffers, update_model_qparams) is the class's own."""
    from llmc_amd.compression.quantization import FloatQuantizer
    from llmc_amd.compression.quantization.gptq import GPTQ
    p = case + '/'
    Wp, U, fmt, gs, static_groups, _, _ = O.case_inputs(GOLD, case)
    actorder = bool(GOLD[p + 'meta'][3])
    dt = str(GOLD[p + 'dt'])
    R, K = Wp.shape
    perm = torch.from_numpy(GOLD[p + 'perm']).cuda()
    Wp_d, U_d = torch.from_numpy(Wp).cuda(), torch.from_numpy(U).cuda()

    class GoldenGPTQ(GPTQ):
        def hessian_sorting(self, name):
            self.perm = perm

        def process_hessian_and_weights(self, layer, name):
            if not self.ready():                       # gptq.py:143-148
                if self.wquantizer.granularity == 'per_group':
                    self.groups = []
                    self.search_group_qparams(layer)
                else:
                    self.search_layer_qparams(layer)
            if self.actorder:                          # gptq.py:150-156
                self.invperm = torch.argsort(self.perm)
                layer.register_buffer('buf_perm', self.perm)
                layer.register_buffer('buf_invperm', self.invperm)
            return Wp_d.clone(), U_d

    kw = dict(group_size=gs) if gs else {}
    wq = FloatQuantizer(fmt, True, 'per_group' if gs else 'per_channel', use_qtorch=True, **kw)
    a = GoldenGPTQ.__new__(GoldenGPTQ)
    a.wquantizer, a.static_groups, a.actorder, a.blocksize, a.owq, a.percdamp = wq, static_groups, actorder, 128, False, 0.01
    a.model_dtype = TD[dt]
    a.need_perm = bool(gs) and not static_groups and actorder
    a.layers_cache = {'fc': {'columns': K}}
    layer = torch.nn.Linear(K, R, bias=False).to(TD[dt]).cuda()
    layer.weight.data = torch.from_numpy(O.from_bits16(GOLD[p + 'W0_bits'], dt).reshape(R, K)).to(TD[dt]).cuda()
    # collect_block_qparams (base_blockwise_quantization.py:338-365)
    _, s0, z0, qmax, qmin = wq.get_tensor_qparams(layer.weight.data)
    layer.register_buffer('buf_scales', s0.detach())
    layer.register_buffer('buf_zeros', z0.detach())
    layer.register_buffer('buf_qmax', torch.as_tensor(qmax).cuda())
    layer.register_buffer('buf_qmin', torch.as_tensor(qmin).cuda())
    return a, wq, layer


@pytest.mark.parametrize('generic', [False, True], ids=['default', 'generic'])
@pytest.mark.parametrize('case', CASES)
def test_golden_through_the_class(case, generic):
    p = case + '/'
    a, wq, layer = _golden_gptq(case)
    gs, static_groups = int(GOLD[p + 'meta'][2]), bool(GOLD[p + 'meta'][4])
    dt = str(GOLD[p + 'dt'])
    R, K = layer.weight.shape
    assert str(layer.buf_scales.dtype) == str(GOLD[p + 'rtn_scales_dtype']), case
    np.testing.assert_array_equal(bits(host(layer.buf_scales).reshape(-1)), bits(GOLD[p + 'rtn_scales']), err_msg=case + ' RTN')
    with generic_path(generic):
        a.layer_transform_reference(layer, 'fc')
    assert layer.weight.dtype == torch.float32
    np.testing.assert_array_equal(bits(host(layer.weight)), bits(GOLD[p + 'final_w']), err_msg=case + ' final_w')
    # the qparams the loop leaves behind: groups / qparams with the reference's 0-dim zero, buf_scales as the reference leaves it
    if gs:
        gsc = torch.cat([q['scale'].reshape(R, 1).float() for q in a.groups], 1)
        assert all(q['zero'].dim() == 0 and float(q['zero']) == 0.0 for q in a.groups)
        assert all(float(q['qmax']) == float(wq.qmax) and float(q['qmin']) == float(wq.qmin) for q in a.groups)
    else:
        gsc = a.qparams['scale'].reshape(R, 1).float()
        assert a.qparams['zero'].dim() == 0 and float(a.qparams['zero']) == 0.0
    np.testing.assert_array_equal(bits(host(gsc)), bits(GOLD[p + 'g_scales']), err_msg=case + ' group scales')
    assert str(layer.buf_scales.dtype) == str(GOLD[p + 'buf_scales_dtype']), case
    np.testing.assert_array_equal(bits(host(layer.buf_scales).reshape(-1)), bits(GOLD[p + 'buf_scales']),
                                  err_msg=case + ' buf_scales')
    fq = a.w_qdq(layer, wq)
    assert str(fq.dtype) == str(GOLD[p + 'w_qdq_dtype']), case
    np.testing.assert_array_equal(bits(host(fq)), bits(O.from_bits16(GOLD[p + 'w_qdq_bits'], dt).reshape(R, K)),
                                  err_msg=case + ' w_qdq')
    if (p + 'w_q_bytes') in GOLD.files:
        cw, cs, cz = a.w_q(layer, wq)
        assert cz is None and str(cw.dtype) == str(GOLD[p + 'w_q_dtype']) and str(cs.dtype) == str(GOLD[p + 'w_q_scales_dtype'])
        np.testing.assert_array_equal(cw.view(torch.uint8).cpu().numpy(), GOLD[p + 'w_q_bytes'], err_msg=case + ' w_q weight')
        assert tuple(cs.shape) == GOLD[p + 'w_q_scales'].shape
        np.testing.assert_array_equal(bits(host(cs)), bits(GOLD[p + 'w_q_scales']), err_msg=case + ' w_q scales')
    else:
        assert a.need_perm


# =========================================================================================================================
# 2. shapes past the golden, against the numpy oracle
def upper(K, seed, amp):
    """An upper factor of exact dyadic values: off-diagonal entries in [-amp, amp] (amp a power of two), diagonal in [0.5, 1.45].
    With amp = 1/8 the in-block feedback moves a weight by several percent of its value."""
    i = np.arange(K, dtype=np.int64)[:, None]
    j = np.arange(K, dtype=np.int64)[None, :]
    h = (i * 2654435761 + j * 40503 + seed * 7919) % 65521
    off = ((h % 257) - 128).astype(np.float32) * np.float32(amp / 128.0)
    diag = np.float32(0.5) + (i % 61).astype(np.float32) / np.float32(64.0)
    return np.where(j > i, off, np.where(j == i, diag, np.float32(0.0))).astype(np.float32)


def weights(R, K, seed):
    """bf16-valued weights with outlier columns, a zero row, a constant row, a row of large values, a -0 and a tiny value"""
    rs = np.random.RandomState(seed)
    W = (rs.standard_normal((R, K)) * 0.02).astype(np.float32)
    W[:, rs.choice(K, max(1, K // 64), replace=False)] *= 20
    W[0, :] = 0.0
    W[1, :128] = 0.0173
    W[2, :128] *= 3000.0
    W[5, 7] = -0.0
    W[6, 9] = 1e-30
    return Q.rnd(W, 'bf16')


def static_scales(W, fmt, gs):
    """the RTN scales a bf16 layer would hold (max(|w|).clamp(1e-5) / qmax, every op rounded to bf16), [R, ng]; row 3's are 0,
    as an fp16 scale that underflowed would be; row 4's are half of that: its largest weights lie beyond the format's range
    (e5m2 saturates only there: |w / s| >= 61440)"""
    R, K = W.shape
    qmax = O.FORMATS[fmt][2]
    g = W.reshape(R, -1, gs) if gs else W.reshape(R, 1, K)
    s, _ = Q.qparams_from_minmax(g.min(-1), g.max(-1), 'bf16', True, -qmax, qmax)
    s[3] = 0.0
    s[4] *= np.float32(0.5)
    return s


_ORACLE = {}


def oracle_rows(key, W, U, fmt, gs, static_groups, col_group, scales, rows):
    """computed once per (shape, configuration), shared by the tests that need it"""
    if key not in _ORACLE:
        _ORACLE[key] = O.weight_transform(W[rows], U, fmt, gs, static_groups, col_group, None if scales is None else scales[rows])
    return _ORACLE[key]


def check_rows(tag, tmp, losses, s, ref, rows, dynamic):
    ri = torch.from_numpy(rows).cuda()
    np.testing.assert_array_equal(bits(host(tmp[ri])), bits(ref['tmp']), err_msg=tag + ' tmp')
    np.testing.assert_array_equal(bits(host(losses[ri])), bits(ref['losses']), err_msg=tag + ' losses')
    if dynamic:
        np.testing.assert_array_equal(bits(host(s[ri])), bits(ref['scales']), err_msg=tag + ' scales')


# (R, K, fmt, group_size, static_groups, generic forced). R = 48: not a multiple of the 32 rows of a 512-thread workgroup, five
# blocks (one outer group and a far update); R = 16384: 1024-thread workgroups. Dynamic groups of 32 start mid-block and always
# take the generic in-block path; per_channel / static groups / dynamic g128 take the fast path unless the generic one is forced.
SHAPES = [
    (48, 640, 'e5m2', 0, False, False),
    (48, 640, 'e4m3', 128, False, False),
    (48, 640, 'e5m2', 32, False, False),
    (48, 640, 'e4m3', 64, True, False),
    (48, 640, 'e4m3', 0, False, True),
    (48, 640, 'e5m2', 0, False, True),
    (16384, 256, 'e5m2', 128, False, False),
    (16384, 256, 'e4m3', 0, False, False),
    (16384, 256, 'e4m3', 0, False, True),
]


@pytest.mark.parametrize('R,K,fmt,gs,static_groups,generic', SHAPES)
def test_shapes_match_the_oracle(R, K, fmt, gs, static_groups, generic):
    W, U = weights(R, K, R + K), upper(K, R + K, 1.0 / 8)
    dynamic = bool(gs) and not static_groups
    scales = None if dynamic else static_scales(W, fmt, gs)
    col_group = None
    if static_groups:
        col_group = (np.random.RandomState(K).permutation(K) // gs).astype(np.int32)      # actorder: any processing order
    rows = np.arange(R) if R <= 64 else np.sort(np.concatenate([np.arange(8), np.random.RandomState(R).choice(
        np.arange(8, R), 56, replace=False)]))
    with generic_path(generic):
        tmp, losses, s = run_loop(W, U, fmt, gs, static_groups, col_group, scales)
    ref = oracle_rows((R, K, fmt, gs, static_groups), W, U, fmt, gs, static_groups, col_group, scales, rows)
    check_rows(f'{R}x{K} {fmt} g{gs} static={static_groups} generic={generic}', tmp, losses, s, ref, rows, dynamic)
    # the inputs do what they were made for: the format's saturation is reached (e4m3: the scale maps the range to +-448 while
    # the grid ends at 240; e5m2 with given scales: row 4)
    assert ref['t_absmax'] >= (248.0 if fmt == 'e4m3' else 0.0 if dynamic else 61440.0)


def test_rider_launch_matches_plain_launches_and_the_oracle():
    """R = 4096, K = 1536 per_channel: the in-block kernel of the second and third outer group carries tiles of the first
    group's far update (k_gptq_block_riders). With riders and without: identical tensors, and the oracle's on 64 rows."""
    R, K, fmt = 4096, 1536, 'e4m3'
    L = _ffi.lib()
    plan = np.zeros((256, 12), np.int32)
    with _ffi.helper_streams(False):
        n = L.llmc_test_gptq_rider_plan(R, K, K, 0, 0, plan.ctypes.data, 256)
    assert n > 0 and (plan[:n][plan[:n, 0] == 0][:, 6] >= 0).any(), 'this shape must engage the rider launch'
    W, U = weights(R, K, 77), upper(K, 77, 1.0 / 8)
    scales = static_scales(W, fmt, 0)
    Ud = torch.from_numpy(U).cuda()
    with _ffi.helper_streams(False):            # riders belong to the one-stream schedule
        tmp, losses, s = run_loop(W, Ud, fmt, 0, False, None, scales)
        with _ffi.option(no_riders=1):
            tmp2, losses2, _ = run_loop(W, Ud, fmt, 0, False, None, scales)
    assert torch.equal(tmp.view(torch.int32), tmp2.view(torch.int32))
    assert torch.equal(losses.view(torch.int32), losses2.view(torch.int32))
    rows = np.sort(np.concatenate([np.arange(8), np.random.RandomState(5).choice(np.arange(8, R), 56, replace=False)]))
    ref = oracle_rows((R, K, fmt, 0, False), W, U, fmt, 0, False, None, scales, rows)
    check_rows('riders', tmp, losses, s, ref, rows, False)


# =========================================================================================================================
# 3. fast path == generic path
@pytest.mark.parametrize('gs', [0, 128], ids=['per_channel', 'g128_dynamic'])
def test_fast_and_generic_path_give_the_same_tensors(gs):
    R, K, fmt = 4096, 1024, 'e4m3'
    W = weights(R, K, 31 + gs)
    W[40, 300] = np.float32(2.0 ** 41)          # outside the range the hoisted division is proven for: the wave falls back
    W[41, 5] = np.float32(1e-40)                # a subnormal weight
    U = torch.from_numpy(upper(K, 31, 1.0 / 32)).cuda()
    scales = static_scales(W, fmt, 0) if not gs else None
    tmp, losses, s = run_loop(W, U, fmt, gs, False, None, scales)
    with generic_path(True):
        tmp2, losses2, s2 = run_loop(W, U, fmt, gs, False, None, scales)
    assert torch.equal(tmp.view(torch.int32), tmp2.view(torch.int32))
    assert torch.equal(losses.view(torch.int32), losses2.view(torch.int32))
    assert torch.equal(s.view(torch.int32), s2.view(torch.int32))
    assert torch.isfinite(tmp[:40]).all()


def test_unknown_format_is_refused_by_the_entry_point():
    L = _ffi.lib()
    W = torch.zeros(8, 256, device='cuda')
    U = torch.eye(256, device='cuda')
    s = torch.ones(8, 1, device='cuda')
    ws = _ffi.workspace(L.llmc_gptq_quantize_ws_bytes(8, 256), W.device)
    rc = L.llmc_gptq_quantize_fp8_cols(_ffi.ptr(W), _ffi.ptr(U), 8, 256, 256, 2, 0, 0, None, _ffi.ptr(s), _ffi.ptr(W.clone()), None,
                                       128, _ffi.ptr(ws), _ffi.stream())
    assert rc == -95 and 'fmt' in _ffi.last_error()
    rc = L.llmc_gptq_quantize_fp8_cols(_ffi.ptr(W), _ffi.ptr(U), 8, 256, 256, 0, 96, 0, None, _ffi.ptr(s), _ffi.ptr(W.clone()), None,
                                       128, _ffi.ptr(ws), _ffi.stream())
    assert rc == -95


# =========================================================================================================================
# 4. the class with the shipped configuration
class Cfg(dict):
    __getattr__ = dict.get


def _shipped_quant():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_quant_configs.json')
    with open(path) as f:
        return json.load(f)['backend/vllm/fp8/gptq_fp8.yml']['quant']


def _toy_gptq(record=None):
    import llmc_amd.compression.quantization as Qz
    from toy_model import ToyModel, calib_input
    model = ToyModel()
    q = _shipped_quant()
    assert q['weight']['quant_type'] == 'float-quant' and q['weight']['bit'] == 'e4m3' and q['method'] == 'GPTQ'
    config = Cfg(calib=Cfg(seq_len=64), model=Cfg(type='Toy'))

    class Recording(Qz.GPTQ):
        """before a subset goes through the stacked column loop, every layer of it goes through the reference's per-layer flow
        (the body of layer_transform_reference) on a twin, with the very Hessian the stacked loop is about to use"""
        def _transform_group(self, gid, layers, names):
            if record is not None:
                for l, n in zip(layers, names):
                    twin = torch.nn.Linear(l.weight.shape[1], l.weight.shape[0], bias=False)
                    twin.weight.data = l.weight.data.clone()
                    for b in ('buf_scales', 'buf_zeros', 'buf_qmax', 'buf_qmin'):
                        twin.register_buffer(b, getattr(l, b).clone())
                    self.initialize_qparams_and_prepare_weights(twin, n)
                    Wp, U = self.process_hessian_and_weights(twin, n)
                    kept = dict(layer=l, Wp=Wp.clone(), U=U.clone(), perm=self.perm.clone(), rtn=l.buf_scales.clone())
                    self.update_layer_with_transformed_weights(twin, Wp, U, n)
                    kept.update(w_ref=twin.weight.data.clone(), s_ref=twin.buf_scales.clone())
                    record.append(kept)
            return super()._transform_group(gid, layers, names)

    return model, Recording(model, q, calib_input(model), None, config)


def test_shipped_config_quantizes_to_the_e4m3_grid():
    """GPTQ on the toy model with the `quant` section of the shipped gptq_fp8.yml, run_block_loop -> deploy('fake_quant').
    What carries the weight (and fails where the loop rounds to an integer grid): the routing (algo.fp8), and every layer's
    compensated weights against the numpy oracle's e4m3 loop on the captured upper factor — the oracle is pinned to the
    reference by tests/test_gptq_fp8_oracle.py — together with their identity to the per-layer reference flow on the same Hessian.
    The grid property of the deployed weights comes after that and cannot fail because of the loop: w_qdq rounds the compensated
    weights afresh, so it checks deployment (the quantizer the layer is deployed with is the one the loop compensated for). It
    is stated on the fp32 product float_quantize(w / s) * s that w_qdq forms before its cast to the model dtype: (that) / s is a
    fixed point of the rounding and at most 240. The bf16 tensor w_qdq returns is the rounding of that product (an e4m3 value
    times a bf16 scale has 12 significant bits, bf16 keeps 8), so w_qdq / s itself lies within bf16's half ulp of a grid
    point, not on it."""
    record = []
    model, algo = _toy_gptq(record)
    assert algo.fp8 == 'e4m3' and algo.gcfg.fp8 == 'e4m3'
    algo.run_block_loop()
    assert len(record) == 6                                     # three Linears in each of the two blocks
    for r in record:
        layer = r['layer']
        R, K = layer.weight.shape
        # the stacked loop == the reference's per-layer flow on the same Hessian
        assert layer.weight.dtype == torch.float32
        assert torch.equal(layer.weight.data.view(torch.int32), r['w_ref'].view(torch.int32))
        assert torch.equal(layer.buf_scales, r['s_ref']) and layer.buf_scales.dtype == torch.bfloat16
        # ... == the oracle's loop on the captured factor, on 16 rows: the loop rounded to the e4m3 grid with qtorch's rule
        rows = np.sort(np.random.RandomState(K).choice(R, 16, replace=False))
        perm = r['perm'].cpu().numpy()
        ref = O.weight_transform(host(r['Wp'])[rows], host(r['U']), 'e4m3', 0, scales=host(r['rtn']).reshape(R, 1)[rows])
        np.testing.assert_array_equal(bits(host(layer.weight)[rows]), bits(ref['tmp'][:, np.argsort(perm)]))
        assert ref['t_absmax'] >= 248.0             # the scale maps the range to +-448, the grid ends at 240: it saturates
    kept = [(r['layer'], r['layer'].weight.data.clone(), r['layer'].buf_scales.clone()) for r in record]
    fqs = [algo.w_qdq(l, algo.wquantizer) for l, _, _ in kept]
    algo.deploy('fake_quant')
    linears = [getattr(b, n) for b in model.get_blocks() for n in ('gate_proj', 'up_proj', 'down_proj')]      # the record's order
    assert all(type(m).__name__ == 'EffcientFakeQuantLinear' for m in linears)
    for m, fq, (l, w, s) in zip(linears, fqs, kept):
        assert fq.dtype == torch.bfloat16
        s32 = s.float().reshape(-1, 1)
        prod = algo.wquantizer.fake_quant_weight_static(w, {'scales': s, 'zeros': l.buf_zeros, 'qmax': l.buf_qmax,
                                                            'qmin': l.buf_qmin})
        assert prod.dtype == torch.float32
        x = host(prod / s32)
        np.testing.assert_array_equal(bits(Q.qtorch_float_quantize(x, 4, 3)), bits(x))          # a fixed point of the rounding
        assert np.abs(x).max() <= 240.0
        assert torch.equal(fq, prod.to(torch.bfloat16))
        y = host(fq.float() / s32)
        assert (np.abs(y - x) <= np.abs(x) * 2.0 ** -8).all() and np.abs(y).max() <= 240.0 * (1 + 2.0 ** -8)
        inp = torch.randn(4, w.shape[1], device='cuda', dtype=torch.bfloat16)
        assert torch.isfinite(m.cuda()(inp)).all()


def test_shipped_config_deploys_the_float_quantized_export():
    model, algo = _toy_gptq()
    algo.run_block_loop()
    blk = model.get_blocks()[0]
    w, s = blk.down_proj.weight.data.clone(), blk.down_proj.buf_scales.clone()
    algo.deploy('vllm_quant')
    m = model.get_blocks()[0].down_proj
    # (GPTQ.deploy ends with model.convert_dtype(model_dtype), and the toy adapter's converts every floating-point weight: the
    # buffer holds the float8 values in bf16, exactly)
    assert type(m).__name__ == 'VllmRealQuantLinear' and m.weight_dtype == torch.float8_e4m3fn
    v = Q.qtorch_float_quantize((w / s.float().reshape(-1, 1)).cpu().numpy(), 4, 3)
    np.testing.assert_array_equal(bits(host(m.weight.float())), bits(v))
    assert torch.equal(m.weight_scale.reshape(-1).float().cpu(), s.reshape(-1).float().cpu())


def test_qparams_alone_keep_an_underflowed_scale_and_quantizing_replaces_it():
    """An all-zero fp16 row: get_tensor_qparams (get_qparams alone, quant.py:545-553) hands out the scale clamp(1e-5) / 448 as
    fp16 forms it, 0; the calls that go through quant() return it as 1 (quant.py:1062) and quantize the row to zeros."""
    from llmc_amd.compression.quantization import FloatQuantizer
    wq = FloatQuantizer('e4m3', True, 'per_channel', use_qtorch=True)
    w = (torch.randn(8, 256, generator=torch.Generator().manual_seed(3)) * 0.02).to(torch.float16).cuda()
    w[2] = 0.0
    _, s, z, _, _ = wq.get_tensor_qparams(w)
    assert s.dtype == torch.float16 and float(s[2]) == 0.0 and bool((s[[0, 1, 3]] != 0).all()) and z.dim() == 0
    cw, cs, _ = wq.real_quant_weight_dynamic(w)
    assert float(cs[2]) == 1.0 and torch.equal(cs[[0, 1, 3]].reshape(-1), s[[0, 1, 3]].reshape(-1))
    assert bool((cw[2].float() == 0).all())
    cw2, cs2, _ = wq.real_quant_weight_static(w, {'scales': s.clone(), 'zeros': z, 'qmax': wq.qmax, 'qmin': wq.qmin})
    assert torch.equal(cw2.view(torch.uint8), cw.view(torch.uint8)) and torch.equal(cs2.reshape(-1), cs.reshape(-1))
    assert torch.equal(wq.fake_quant_weight_dynamic(w)[2], w[2])
    wb = w.to(torch.bfloat16)                                  # bf16 has fp32's range: nothing underflows
    assert float(wq.get_tensor_qparams(wb)[1][2]) > 0
