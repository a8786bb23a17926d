"""The column-wise min/max quantizer (llmc_quant_dynamic_cols, csrc/quant_cols.hip) on the GPU: against the transposed
composition it replaces (bit for bit; zeros numerically, the sign of a zero minimum follows the reduction order), against the CPU
oracle on the transposed input, and the quantizer route that reaches it (fake_quant_weight_dynamic with dim 'ic')."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import quant_ref as Q  # noqa: E402

pytestmark = pytest.mark.gpu

TD = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}


def bits(t):
    t = t.detach().contiguous().cpu()
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.view(torch.int16).numpy()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy()
    return t.numpy()


def make_weight(R, K, dt, seed, layout='plain'):
    """A weight with planted columns (where it has at least four): all zeros, a constant, denormals only, and one holding the
    dtype's largest value. layout: 'plain' contiguous; 'offset' base moved by one element; 'slice' columns 8.. of a wider
    matrix (ld > K, vectors still fit); 'slice_odd' columns 3.. of a wider matrix."""
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(R, K, generator=gen) * 0.05
    w[:, ::7] *= 9
    w = w.to(dt)
    if K >= 4:
        fi = torch.finfo(dt)
        w[:, 0] = 0
        w[:, 1] = 0.37
        w[:, 2] = (torch.arange(R) % 3 + 1).to(dt) * torch.tensor(fi.smallest_normal / 4, dtype=dt)
        w[R // 2, 3] = fi.max
    w = w.cuda()
    if layout == 'offset':
        buf = torch.empty(R * K + 1, dtype=dt, device='cuda')
        buf[1:].copy_(w.reshape(-1))
        return buf[1:].view(R, K)
    if layout in ('slice', 'slice_odd'):
        off = 8 if layout == 'slice' else 3
        wide = torch.zeros(R, K + 16, dtype=dt, device='cuda')
        wide[:, off:off + K] = w
        return wide[:, off:off + K]
    return w


def shapes():
    """(R, K, g, layout) of the sweep"""
    from llmc_amd.compression.quantization import quant_cols_ops as qc
    ragged = qc.TILE_MAX_G + 2 * qc.SLAB_ROWS + 5          # long-column path, last slab of 5 rows
    out = [(R, K, R, 'plain') for R, K in ((1, 8), (7, 13), (64, 72), (257, 520), (1000, 24), (ragged, 40))]
    for K in (8, 72, 520):
        out += [(3 * g, K, g, 'plain') for g in (16, 32, 128)]
        out.append((72, K, 24, 'plain'))
    out.append((600, 72, 300, 'plain'))                    # groups longer than the tile path takes, two of them, ragged slabs
    out += [(96, 72, 32, 'offset'), (96, 72, 32, 'slice'), (96, 72, 32, 'slice_odd'), (96, 75, 32, 'plain'),
            (ragged, 72, ragged, 'offset'), (ragged, 72, ragged, 'slice')]
    return out


QUANTIZERS = [  # sym, round_zp, qmin, qmax, code kind that holds the range
    (True, True, -8.0, 7.0, 'I8'), (True, True, -128.0, 127.0, 'I8'), (True, False, -128.0, 127.0, 'I8'),
    (False, True, 0.0, 15.0, 'U8'), (False, True, 0.0, 255.0, 'U8'), (False, False, 0.0, 15.0, 'U8'),
    (False, False, 0.0, 255.0, 'U8'),
]


@pytest.mark.parametrize('dt', ['f16', 'bf16', 'f32'])
def test_kernel_equals_the_composition_on_every_path(dt):
    from llmc_amd import _ffi
    from llmc_amd.compression.quantization import quant_cols_ops as qc
    seen, bad, checked = set(), [], 0
    for si, (R, K, g, layout) in enumerate(shapes()):
        w = make_weight(R, K, TD[dt], 100 + si, layout)
        seen.add(qc.path(w, g))
        for sym, rz, qmin, qmax, code in QUANTIZERS:
            for kind in (_ffi.OUT_FAKE, _ffi.OUT_I32, getattr(_ffi, 'OUT_' + code)):
                out, s, z = qc.fake_quant_cols(w, g, sym, rz, qmin, qmax, kind, want_qparams=True)
                ref, rs, rzs = qc.fake_quant_cols_composed(w, g, sym, rz, qmin, qmax, kind, want_qparams=True)
                tag = (R, K, g, layout, sym, rz, qmax, kind)
                checked += 1
                if not (out.is_contiguous() and out.shape == (R, K) and out.dtype == ref.dtype):
                    bad.append(('layout', tag))
                elif not np.array_equal(bits(out), bits(ref)):
                    bad.append(('out', tag))
                elif not np.array_equal(bits(s), bits(rs.reshape(-1))):
                    bad.append(('scales', tag))
                elif (z is None) != (rzs is None) or (z is not None and not torch.equal(z, rzs.reshape(-1))):
                    bad.append(('zeros', tag))
    assert not bad, bad[:8]
    assert checked == len(shapes()) * len(QUANTIZERS) * 3
    # every launch path ran
    assert seen == set(range(_ffi.lib().llmc_quant_dynamic_cols_paths())), seen


@pytest.mark.parametrize('dt,R,K,g,sym,bit', [('bf16', 257, 520, 257, True, 8), ('f16', 96, 72, 32, False, 4)])
def test_kernel_equals_the_cpu_oracle_on_the_transposed_input(dt, R, K, g, sym, bit):
    from llmc_amd import _ffi
    from llmc_amd.compression.quantization import quant_cols_ops as qc
    gen = torch.Generator().manual_seed(7)
    w = torch.randn(R, K, generator=gen) * 0.05
    w[:, ::11] *= 12
    w = w.to(TD[dt])
    qmin, qmax = Q.int_range(bit, sym)
    rows = np.ascontiguousarray(w.float().numpy().T).reshape(-1, g)
    fq_ref, s_ref, _ = Q.fake_quant_dynamic(rows, dt, sym, qmin, qmax)
    codes_ref, _, _ = Q.real_quant_dynamic(rows, dt, sym, qmin, qmax)
    out, s, _ = qc.fake_quant_cols(w.cuda(), g, sym, True, qmin, qmax, want_qparams=True)
    want = torch.from_numpy(np.ascontiguousarray(fq_ref.reshape(K, R).T)).to(TD[dt])
    np.testing.assert_array_equal(bits(out), bits(want))
    np.testing.assert_array_equal(bits(s), bits(torch.from_numpy(s_ref.reshape(-1)).to(TD[dt])))
    codes = qc.fake_quant_cols(w.cuda(), g, sym, True, qmin, qmax, _ffi.OUT_I32)
    np.testing.assert_array_equal(codes.cpu().numpy(), codes_ref.reshape(K, R).T)


def _count_calls(monkeypatch):
    from llmc_amd.compression.quantization import quant_cols_ops as qc
    calls = []
    real = qc.fake_quant_cols

    def counted(*a, **k):
        calls.append(a[1])
        return real(*a, **k)
    monkeypatch.setattr(qc, 'fake_quant_cols', counted)
    return calls


@pytest.mark.parametrize('cfg', [dict(bit=8, symmetric=True, granularity='per_channel'),
                                 dict(bit=4, symmetric=False, granularity='per_group', group_size=32),
                                 dict(bit=4, symmetric=False, granularity='per_group', group_size=128)])
def test_quantizer_route_is_contiguous_and_bit_equal_on_and_off(cfg, monkeypatch):
    from llmc_amd import _ffi
    from llmc_amd.compression.quantization import IntegerQuantizer
    calls = _count_calls(monkeypatch)
    w = make_weight(96, 256, torch.bfloat16, 3)
    q = IntegerQuantizer(**cfg)
    on = q.fake_quant_weight_dynamic(w, {'dim': 'ic'})
    assert len(calls) == 1 and calls[0] == (32 if cfg.get('group_size') == 32 else 96)
    with _ffi.option(quant_cols=0):
        off = q.fake_quant_weight_dynamic(w, {'dim': 'ic'})
    assert len(calls) == 1
    assert on.is_contiguous() and on.shape == w.shape and on.dtype == w.dtype
    np.testing.assert_array_equal(bits(on), bits(off))
    # and the other axis is not touched by the switch
    oc = q.fake_quant_weight_dynamic(w, {'dim': 'oc'})
    np.testing.assert_array_equal(bits(oc), bits(q.fake_quant_weight_dynamic(w)))
    assert len(calls) == 1


@pytest.mark.parametrize('cfg', [dict(bit=8, symmetric=True, granularity='per_channel', calib_algo='mse'),
                                 dict(bit=8, symmetric=True, granularity='per_tensor'),
                                 dict(bit=8, symmetric=False, granularity='per_tensor')])
def test_mse_and_per_tensor_keep_the_old_route(cfg, monkeypatch):
    from llmc_amd.compression.quantization import IntegerQuantizer
    calls = _count_calls(monkeypatch)
    w = make_weight(96, 136, torch.bfloat16, 4)
    q = IntegerQuantizer(**cfg)
    ic = q.fake_quant_weight_dynamic(w, {'dim': 'ic'})
    assert calls == [] and ic.shape == w.shape
    # the old route: the transposed weight through the row kernels, returned as a transposed view
    np.testing.assert_array_equal(bits(ic), bits(q.fake_quant_weight_dynamic(w.T.contiguous()).T))
