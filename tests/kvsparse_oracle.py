"""The attention-sink KV cache restated in numpy, from its behaviour: a window of `sink` first rows plus the most recent rows,
`window` rows in all. Values are float32 arrays that are exact in the cache's dtype; every elementwise op rounds to that dtype
(oracle.quant_ref.rnd). tests/test_kvsparse_oracle.py pins it to tests/golden/kvsparse.npz; the GPU tests use it where the goldens
have no case.

An update of n rows onto a layer that holds T:
  nothing held     the rows are kept as they are, however many
  T + n < window   appended
  otherwise        the rows kept are the first `sink` and the last window - sink - n; the new rows follow. With cos / sin the kept
                   keys (not the sink, not the values) are rotated from window place sink + n + i to sink + i: by the angle
                   difference of the two places' table rows, cos_d = c_hi * c_lo + s_hi * s_lo, sin_d = -s_hi * c_lo + c_hi * s_lo
                   in fp32, rounded to the dtype; k' = rnd(rnd(k * cos_d) + rnd(half_swap(k) * sin_d)), half_swap = (-second half,
                   first half) of the first `partial` columns (all when partial is None); the columns behind them pass.
The table of places is the 2-dim cos / sin given last, or the rows of the 3-dim ones' batch 0 gathered until the window is
covered. The difference tables are made once per n."""
import numpy as np

from kvquant_oracle import as_f32, to_bits  # noqa: F401  (the bit-pattern helpers are the same)
from oracle import quant_ref as Q

DT_NAME = {0: 'bf16', 1: 'f16', 2: 'f32'}


class OracleSinkCache:
    def __init__(self, dt, window, sink):
        self.dt, self.window, self.sink = dt, window, sink
        self.k = self.v = None
        self.cos = self.sin = None
        self.tables = {}

    @property
    def rows(self):
        return 0 if self.k is None else self.k.shape[2]

    def _places(self, cos, sin):
        cos, sin = np.asarray(cos, np.float32), np.asarray(sin, np.float32)
        if cos.ndim == 2:
            self.cos, self.sin = cos, sin
        elif self.cos is None:
            self.cos, self.sin = cos[0], sin[0]
        elif self.cos.shape[0] < self.window:
            self.cos, self.sin = np.concatenate([self.cos, cos[0]]), np.concatenate([self.sin, sin[0]])

    def _difference(self, n):
        if n not in self.tables:
            c, s = self.cos[:self.window], self.sin[:self.window]
            hi, lo = slice(self.sink + n, None), slice(self.sink, c.shape[0] - n)
            cos_d = c[hi] * c[lo] + s[hi] * s[lo]
            sin_d = (-s[hi]) * c[lo] + c[hi] * s[lo]
            self.tables[n] = Q.rnd(cos_d, self.dt), Q.rnd(sin_d, self.dt)
        return self.tables[n]

    def update(self, k, v, cos=None, sin=None, partial=None):
        k, v = np.asarray(k, np.float32), np.asarray(v, np.float32)
        n = k.shape[2]
        rope = cos is not None and sin is not None
        if rope:
            self._places(cos, sin)
        if self.k is None:
            self.k, self.v = k, v
        elif self.rows + n < self.window:
            self.k, self.v = np.concatenate([self.k, k], 2), np.concatenate([self.v, v], 2)
        else:
            keep = self.window - self.sink - n
            assert keep > 0, (n, self.window, self.sink)
            kept = self.k[:, :, -keep:]
            if rope:
                cos_d, sin_d = self._difference(n)
                rot = kept.shape[-1] if partial is None else partial
                x = kept[..., :rot]
                swap = np.concatenate([-x[..., rot // 2:], x[..., :rot // 2]], -1)
                r = lambda a: Q.rnd(a, self.dt)      # noqa: E731
                kept = np.concatenate([r(r(x * cos_d[None, None]) + r(swap * sin_d[None, None])), kept[..., rot:]], -1)
            self.k = np.concatenate([self.k[:, :, :self.sink], kept, k], 2)
            self.v = np.concatenate([self.v[:, :, :self.sink], self.v[:, :, -keep:], v], 2)
        return self.k, self.v


def case_meta(g, name):
    dt, B, H, D, W, sink, width, prs, cos_dims, steps = (int(x) for x in g[name + '/meta'])
    return dict(dt=DT_NAME[dt], B=B, H=H, D=D, W=W, sink=sink, width=width, partial=prs or None, cos_dims=cos_dims, steps=steps)


def golden_steps(g, name):
    """Yield per step a dict: n, rows, k_in, v_in [B, H, n, D], k_out, v_out [B, H, rows, D] (bit patterns), and cos / sin as the
    reference was given them (bit patterns: [B, n, width], the whole [positions, width] table, or None)."""
    m = case_meta(g, name)
    B, H, D = m['B'], m['H'], m['D']
    pos = {}

    def take(key, shape):
        cnt = int(np.prod(shape, dtype=np.int64))
        o = pos.get(key, 0)
        pos[key] = o + cnt
        return g[f'{name}/{key}'][o:o + cnt].reshape(shape)

    cos = sin = None
    if m['cos_dims']:
        cos, sin = g[name + '/cos'].reshape(-1, m['width']), g[name + '/sin'].reshape(-1, m['width'])
    at = 0
    for n, rows in zip((int(x) for x in g[name + '/steps']), (int(x) for x in g[name + '/rows'])):
        step = {'n': n, 'rows': rows, 'cos': None, 'sin': None}
        for t in 'kv':
            step[t + '_in'] = take(t + '_in', (B, H, n, D))
            step[t + '_out'] = take(t + '_out', (B, H, rows, D))
        if m['cos_dims'] == 3:
            step['cos'] = np.broadcast_to(cos[at:at + n][None], (B, n, m['width']))
            step['sin'] = np.broadcast_to(sin[at:at + n][None], (B, n, m['width']))
        elif m['cos_dims'] == 2:
            step['cos'], step['sin'] = cos, sin
        at += n
        yield step


# ---- bit patterns <-> torch tensors, for the tests that drive the cache itself ---------------------------------------------------
def torch_tensor(bits, dt, device='cpu'):
    import torch
    tdt = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}[dt]
    raw = np.array(bits)          # a writable copy: the goldens are read-only
    t = torch.from_numpy(raw.view(np.int32)) if dt == 'f32' else torch.from_numpy(raw.view(np.int16))
    return t.view(tdt).to(device)


def torch_bits(t):
    import torch
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32)
    return t.view(torch.int16).numpy().view(np.uint16)


def run_golden_case(g, name, cache, device='cpu'):
    """Drive `cache` (a SinkKVCache) through every step of a golden case on `device` and compare what update() returns, bit for
    bit, before the next update (the fused path's views live until the second following update)."""
    m = case_meta(g, name)
    dt = m['dt']
    for s, st in enumerate(golden_steps(g, name)):
        kw = {}
        if st['cos'] is not None:
            kw = {'cos': torch_tensor(st['cos'], dt, device), 'sin': torch_tensor(st['sin'], dt, device)}
        if m['partial']:
            kw['partial_rotation_size'] = m['partial']
        k, v = cache.update(torch_tensor(st['k_in'], dt, device), torch_tensor(st['v_in'], dt, device), 0, kw)
        assert tuple(k.shape) == tuple(v.shape) == st['k_out'].shape, (name, s, k.shape)
        assert np.array_equal(torch_bits(k), st['k_out']), (name, s, 'keys')
        assert np.array_equal(torch_bits(v), st['v_out']), (name, s, 'values')
        assert cache.get_seq_length() == st['rows'] and cache.get_seq_length(1) == 0
