"""Write tests/golden/kvsparse.npz: the reference's SinkKVCache (llmc/compression/sparsification/kvsparse.py) on CPU, step by
step, on small seeded states and real RoPE tables.

Usage (where the reference tree exists; it needs no GPU):  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_kvsparse.py

The reference imports and CPU shims come from oracle/make_golden.py, read-only. The class runs unmodified. It leans on attributes of
transformers' DynamicCache that later releases dropped, so the tool sets them on the instance: _seen_tokens = 0 and two empty
lists key_cache / value_cache.

Keys: '<case>/meta' = [dtype (0 bf16, 1 f16, 2 f32), B, H, D, window_length, num_sink_tokens, table width (0: no cos / sin),
partial_rotation_size (0: not passed), cos dims (0, 2 or 3), steps]; '<case>/steps' = the new rows of every step; '<case>/rows' =
the rows update() returned after it; '<case>/<k|v>_<in|out>' = the concatenation over the steps of the flattened bit patterns
(16-bit tensors as uint16, fp32 as uint32) of the states given to update() [B, H, n, D] and of what it returned
[B, H, rows, D]; '<case>/cos', '<case>/sin' = the RoPE table [positions, width] in the case's dtype. A 3-dim case passes
table[pos:pos + n][None] (repeated over B) per step, the 2-dim case the whole table on every call. 'names'.
tests/kvsparse_oracle.py: golden_steps reads them back.

Cases at [B, H, D] = [1, 2, 32], window_length 8, 2 sink tokens: bf16, f16 and fp32 with new-row counts (5, 1, 1, 1, 1, 2, 1)
(growing, the n + len == W shift that drops nothing, steady shifts, a second table for n = 2); a prompt of 11 rows and two decode
steps; no cos / sin at all; partial_rotation_size 16 with 16-wide tables; the 2-dim cos branch; B = 2.
The tool asserts that in a bf16 case a key kept over several shifts differs in bits from one rotation of the original by the
total shift: without that the file could not tell step-wise rerotation from a single one."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.make_golden import DT, save  # noqa: E402

from llmc.compression.sparsification.kvsparse import SinkKVCache  # noqa: E402  (reference)

DT_CODE = {'bf16': 0, 'f16': 1, 'f32': 2}
W, SINK = 8, 2
MAIN = (5, 1, 1, 1, 1, 2, 1)


def bits(t):
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32).copy()
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def rope_table(positions, width, dt, base=10000.0):
    """cos / sin [positions, width] as a rotary embedding hands them over: fp32 angles, cat(freqs, freqs), cast to dt."""
    inv_freq = 1.0 / (base ** (torch.arange(0, width, 2, dtype=torch.float32) / width))
    freqs = torch.outer(torch.arange(positions, dtype=torch.float32), inv_freq)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().to(dt), emb.sin().to(dt)


def run_case(gen, name, dname, steps, B=1, H=2, D=32, width=32, prs=0, cos_dims=3):
    dt = DT[dname]
    cache = SinkKVCache(1, W, SINK)
    cache._seen_tokens = 0
    cache.key_cache, cache.value_cache = [], []
    total = sum(steps)
    out = {f'{name}/meta': np.array([DT_CODE[dname], B, H, D, W, SINK, width if cos_dims else 0, prs, cos_dims, len(steps)], np.int64),
           f'{name}/steps': np.array(steps, np.int64)}
    if cos_dims:
        cos, sin = rope_table(max(total, W), width, dt)
        out[f'{name}/cos'], out[f'{name}/sin'] = bits(cos).reshape(-1), bits(sin).reshape(-1)
    parts, rows, pos, keys_out = {}, [], 0, []
    for n in steps:
        k, v = torch.randn(B, H, n, D, generator=gen).to(dt), torch.randn(B, H, n, D, generator=gen).to(dt)
        kw = {}
        if cos_dims == 3:
            kw = {'cos': cos[pos:pos + n][None].expand(B, -1, -1), 'sin': sin[pos:pos + n][None].expand(B, -1, -1)}
        elif cos_dims == 2:
            kw = {'cos': cos, 'sin': sin}
        if prs:
            kw['partial_rotation_size'] = prs
        ko, vo = cache.update(k, v, 0, kw)
        assert ko.shape == vo.shape and ko.dtype == vo.dtype == dt and cache.get_seq_length() == ko.shape[-2]
        for key, t in (('k_in', k), ('v_in', v), ('k_out', ko), ('v_out', vo)):
            parts.setdefault(key, []).append(bits(t).reshape(-1))
        rows.append(ko.shape[-2])
        keys_out.append(ko.clone())
        pos += n
    out.update({f'{name}/{key}': np.concatenate(v) for key, v in parts.items()})
    out[f'{name}/rows'] = np.array(rows, np.int64)
    return out, rows, keys_out


def single_rotation_differs(keys_out, cos, sin):
    """The main bf16 case: the row appended at step 3 (window place 7) sits at place 3 after the shifts of steps 4-6 (1 + 2 + 1
    rows). Rotate the original once from place 7 to place 3, tables made as the cache makes them, and count the differing bits."""
    c, s = cos.float(), sin.float()
    rc = (c[7] * c[3] + s[7] * s[3]).to(torch.bfloat16)
    rs = (-s[7] * c[3] + c[7] * s[3]).to(torch.bfloat16)
    k0 = keys_out[3][:, :, 7]
    once = (k0 * rc) + (torch.cat((-k0[..., 16:], k0[..., :16]), dim=-1) * rs)
    stepwise = keys_out[6][:, :, 3]
    return int((bits(once) != bits(stepwise)).sum())


def main():
    gen = torch.Generator().manual_seed(20261020)
    out, names = {}, []

    def add(name, *a, **k):
        o, rows, keys_out = run_case(gen, name, *a, **k)
        out.update(o)
        names.append(name)
        print(f'{name}: rows {rows}')
        return rows, keys_out

    for dname in ('bf16', 'f16', 'f32'):
        rows, keys_out = add(f'main_{dname}', dname, MAIN)
        assert rows == [5, 6, 7, 8, 8, 8, 8], rows
        if dname == 'bf16':
            differs = single_rotation_differs(keys_out, *rope_table(sum(MAIN), 32, torch.bfloat16))
            print(f'main_bf16: {differs} elements of the key kept over three shifts differ from one rotation by the total shift')
            assert differs > 0, 'step-wise rerotation and a single rotation give the same bits'
    rows, _ = add('prompt11_bf16', 'bf16', (11, 1, 1))
    assert rows == [11, 8, 8], rows
    add('norope_bf16', 'bf16', MAIN, cos_dims=0)
    add('partial16_bf16', 'bf16', MAIN, width=16, prs=16)
    add('cos2d_bf16', 'bf16', MAIN, cos_dims=2)
    add('b2_bf16', 'bf16', MAIN, B=2)
    out['names'] = np.array(names)
    save('kvsparse', **out)


if __name__ == '__main__':
    main()
