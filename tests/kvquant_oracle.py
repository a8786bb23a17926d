"""The reference's two quantized KV caches (llmc/compression/quantization/kvquant.py:44-87, 136-186, 233-289) restated on the
CPU in numpy over oracle/quant_ref.py, and the reader of tests/golden/kvquant.npz (tools/make_golden_kvquant.py).

Values of a 16-bit dtype travel as float32 arrays that hold them exactly; `dt` is quant_ref's 'bf16' / 'f16' / 'f32'. A cache
holds, per tensor, the reference's dict: q_tensor [B, H, T, D] (integers), scales and zeros in the reference's shapes
([B, H, T, 1] per_token, [B * H * T * D / g, 1] per_group, 0-dim per_tensor; a symmetric zero is a 0-dim 0.0).
test_kvquant_oracle.py pins it to the goldens bit for bit; the GPU tests then use it at shapes the goldens do not have."""
import numpy as np

from oracle import quant_ref as Q

GRAN = {0: 'per_token', 1: 'per_group', 2: 'per_tensor'}


class OracleKVCache:
    """method 'Naive' or 'Kivi'; int-quant, calib_algo minmax, round_zp True."""

    def __init__(self, dt, bit, sym, granularity, group_size=None, method='Naive', residual_length=128):
        self.dt, self.sym, self.granularity, self.group_size = dt, sym, granularity, group_size
        self.qmin, self.qmax = Q.int_range(bit, sym)
        self.kivi = method == 'Kivi'
        self.residual_length = residual_length
        self.k = self.v = None              # the reference's _quantized_*_cache[layer] dicts
        self.resid_k = self.resid_v = None  # Kivi: None stands for the reference's 1-D empty tensor
        self.seen = 0

    # kvquant.py:136-176 with quant.py:132-143, 545-559, 699-707
    def quantize(self, x):
        x = np.asarray(x, np.float32)
        dt, sym, qmin, qmax = self.dt, self.sym, self.qmin, self.qmax
        if self.granularity == 'per_tensor':
            if sym:
                s, _ = Q.qparams_from_minmax(np.float32(x.min()), np.float32(x.max()), dt, True, qmin, qmax)
                codes, _ = Q.quant_codes(x, dt, s, dt, None, None, qmin, qmax)
                return {'q_tensor': codes, 'scales': np.float32(s), 'zeros': np.float32(0.0)}
            _, codes, s, z = Q.per_tensor_asym_fake_and_codes(x, dt, qmin, qmax)
            return {'q_tensor': codes.astype(np.float32), 'scales': s, 'zeros': z}
        grouped = self.granularity == 'per_group' and x.shape[-1] >= self.group_size
        rows = x.reshape(-1, self.group_size if grouped else x.shape[-1])
        s, z = Q.minmax_qparams(rows, dt, sym, qmin, qmax)
        codes, _ = Q.quant_codes(rows, dt, s, dt, None if sym else z, None if sym else dt, qmin, qmax)
        shp = (-1, 1) if grouped else (*x.shape[:-1], 1)
        return {'q_tensor': codes.reshape(x.shape), 'scales': s.reshape(shp),
                'zeros': np.float32(0.0) if sym else z.reshape(shp)}

    # kvquant.py:178-186 with quant.py:709-712
    def dequantize(self, d):
        q, s, z = d['q_tensor'], d['scales'], d['zeros']
        if np.ndim(s) == 2:
            return Q.dequant(q.reshape(-1, self.group_size), s, z, self.dt).reshape(q.shape)
        return Q.dequant(q, s, z, self.dt)

    def update(self, k, v):
        k, v = np.asarray(k, np.float32), np.asarray(v, np.float32)
        self.seen += k.shape[-2]
        if self.k is None:
            self.k, self.v = self.quantize(k), self.quantize(v)
            if self.kivi:
                return k, v
            return self.dequantize(self.k), self.dequantize(self.v)
        if not self.kivi:
            keys = np.concatenate([self.dequantize(self.k), k], axis=-2)
            values = np.concatenate([self.dequantize(self.v), v], axis=-2)
            self.k, self.v = self.quantize(keys), self.quantize(values)
            return keys, values
        flush = self.resid_k is not None and self.resid_k.shape[-2] + 1 >= self.residual_length
        k_new = k if self.resid_k is None else np.concatenate([self.resid_k, k], axis=-2)
        v_new = v if self.resid_v is None else np.concatenate([self.resid_v, v], axis=-2)
        keys = np.concatenate([self.dequantize(self.k), k_new], axis=-2)
        values = np.concatenate([self.dequantize(self.v), v_new], axis=-2)
        if flush:
            self.k, self.v = self.quantize(keys), self.quantize(values)
            self.resid_k = self.resid_v = None
        else:
            self.resid_k, self.resid_v = k_new, v_new
        return keys, values

    def quantized(self, is_key=True):
        return self.k if is_key else self.v


def from_meta(dt, meta):
    bit, sym, gran, group, B, H, T0, D, steps, kivi, resid = (int(x) for x in meta)
    return OracleKVCache(dt, bit, bool(sym), GRAN[gran], group or None, 'Kivi' if kivi else 'Naive', resid)


def case_dt(name):
    return 'bf16' if '_bf16_' in name else 'f16'


def as_f32(bits, dt):
    """the values behind recorded bits: uint16 of bf16 / f16, uint32 of fp32"""
    bits = np.asarray(bits)
    if bits.dtype == np.uint32:
        return bits.view(np.float32)
    if dt == 'bf16':
        return (bits.astype(np.uint32) << 16).view(np.float32)
    return bits.view(np.float16).astype(np.float32)


def to_bits(a, dt):
    """float32 values that are exact in dt -> the dtype's bit patterns"""
    shape = np.shape(a)
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    if dt == 'bf16':
        return (a.view(np.uint32) >> 16).astype(np.uint16).reshape(shape)
    if dt == 'f16':
        return a.astype(np.float16).view(np.uint16).reshape(shape)
    return a.view(np.uint32).reshape(shape)


def golden_steps(g, name):
    """Yield per step a dict of arrays in their recorded shapes: k_in, v_in, k_out, v_out (bit patterns), k_q, v_q (int16 values),
    k_scales, v_scales, k_zeros, v_zeros (bit patterns; uint32 where the reference holds fp32), and 'rows'."""
    bit, sym, gran, group, B, H, T0, D, steps, kivi, resid = (int(x) for x in g[name + '/meta'])
    rows = [int(r) for r in g[name + '/rows']]
    pos = {}

    def take(key, shape):
        n = int(np.prod(shape, dtype=np.int64))
        a = g[f'{name}/{key}']
        o = pos.get(key, 0)
        pos[key] = o + n
        return a[o:o + n].reshape(shape)

    for s in range(steps):
        n, T = (T0 if s == 0 else 1), rows[s]
        if gran == 2:
            qshape = ()
        elif gran == 1 and D >= group:
            qshape = (B * H * T * D // group, 1)
        else:
            qshape = (B, H, T, 1)
        step = {'rows': T}
        for t in 'kv':
            step[t + '_in'] = take(t + '_in', (B, H, n, D))
            step[t + '_out'] = take(t + '_out', (B, H, T0 + s, D))
            step[t + '_q'] = take(t + '_q', (B, H, T, D))
            step[t + '_scales'] = take(t + '_scales', qshape)
            step[t + '_zeros'] = take(t + '_zeros', () if sym else qshape)
        yield step
    for key, o in pos.items():
        assert o == g[f'{name}/{key}'].size, (name, key)
