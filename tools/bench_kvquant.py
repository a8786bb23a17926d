"""Time one decode update() of NaiveQuantKVCache (kvquant.py: llmc_kv_cache_update, csrc/kv_cache.hip) against the reference's
op sequence for the same step, transcribed to torch ops on the same GPU (`RefCache` below: kvquant.py:44-87, 136-186 with
quant.py:132-143, 545-559, 699-712 of the reference; it lives here, not in the product, and reads nothing of the reference).

    python tools/bench_kvquant.py --txt profiles/kvquant.txt

The driver opens no GPU itself. It runs one child process per step (a T and a quantizer), each under `timeout -k 10`, one after
the other, and stops at the first that fails. A step: bf16, B = 1, H = 8, D = 128; both caches are filled with T rows of seeded
states, then one-token updates are timed: device events around one update() of keys and values ending in a synchronise, --warmup
calls per side first, the two sides alternating inside every repetition, median with min..max of --reps. Every update appends a
row, so T grows by warmup + reps during a step: 0.1 % at the smallest T of the default 3 + 20.
GB/s = the bytes the fused update must move, 4 per stored element (1 code read, 2 + 1 written) for keys and values, over the
median time of the whole call (allocation of the returned tensors and launch included; not a kernel time).
equal = the share of the last returned keys' elements with the same bits on both sides."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, D = 1, 8, 128
CONFIGS = {'w8sym_token': dict(bit=8, symmetric=True, granularity='per_token'),
           'w4asym_g32': dict(bit=4, symmetric=False, granularity='per_group', group_size=32)}
TS = (512, 4096, 32768)


class RefCache:
    """The reference's Naive cache for one layer from torch ops: float codes in the tensor dtype, the whole cache dequantized,
    concatenated and quantized again on every update."""

    def __init__(self, bit, symmetric, granularity, group_size=None):
        import torch
        self.sym, self.granularity, self.group_size = symmetric, granularity, group_size
        if symmetric:
            self.qmin, self.qmax = torch.tensor(-(2 ** (bit - 1))), torch.tensor(2 ** (bit - 1) - 1)
        else:
            self.qmin, self.qmax = torch.tensor(0.0), torch.tensor(2 ** bit - 1)
        self.k = self.v = None

    def reshape(self, t):
        return t.reshape(-1, self.group_size) if self.granularity == 'per_group' else t

    def quantize(self, tensor):
        import torch
        shape = tensor.shape
        tensor = self.reshape(tensor)
        max_val, min_val = tensor.amax(dim=-1, keepdim=True), tensor.amin(dim=-1, keepdim=True)
        qmin, qmax = self.qmin.to(tensor.device), self.qmax.to(tensor.device)
        if self.sym:
            scales = torch.max(max_val.abs(), min_val.abs()).clamp(min=1e-5) / qmax
            zeros = torch.tensor(0.0)
            q = torch.clamp(torch.round(tensor / scales) + zeros.to(tensor.device), qmin, qmax)
        else:
            scales = (max_val - min_val).clamp(min=1e-5) / (qmax - qmin)
            zeros = (qmin - torch.round(min_val / scales)).clamp(qmin, qmax)
            q = torch.clamp(torch.round(tensor / scales) + zeros, qmin, qmax)
        return {'q_tensor': q.reshape(shape), 'scales': scales, 'zeros': zeros}

    def dequantize(self, d):
        q = d['q_tensor']
        return ((self.reshape(q) - d['zeros'].to(q.device)) * d['scales']).reshape(q.shape)

    def update(self, key_states, value_states):
        import torch
        if self.k is None:
            self.k, self.v = self.quantize(key_states.contiguous()), self.quantize(value_states.contiguous())
            return self.dequantize(self.k), self.dequantize(self.v)
        keys = torch.cat([self.dequantize(self.k), key_states], dim=-2)
        values = torch.cat([self.dequantize(self.v), value_states], dim=-2)
        self.k, self.v = self.quantize(keys.contiguous()), self.quantize(values.contiguous())
        return keys, values


def step(T, cfg_name, reps, warmup):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_kvquant: needs the GPU (no CPU fallback)')
    torch.set_grad_enabled(False)
    from llmc_amd.compression.quantization.kvquant import NaiveQuantKVCache
    cfg = CONFIGS[cfg_name]
    gen = torch.Generator(device='cuda').manual_seed(T)

    def states(n):
        x = torch.randn(B, H, n, D, generator=gen, device='cuda') * torch.exp(0.7 * torch.randn(1, H, 1, D, generator=gen, device='cuda'))
        return x.to(torch.bfloat16)

    ours = NaiveQuantKVCache('int-quant', dict(cfg, method='Naive'), 1, initial_capacity=T + warmup + reps + 8)
    theirs = RefCache(**cfg)
    k0, v0 = states(T), states(T)
    ours.update(k0, v0, 0, {})
    theirs.update(k0, v0)
    assert ours._layers[0].fused
    del k0, v0
    sides = (lambda k, v: ours.update(k, v, 0, {}), theirs.update)
    acc, last = ([], []), [None, None]
    for r in range(warmup + reps):
        k, v = states(1), states(1)
        for i, fn in enumerate(sides):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn(k, v)
            b.record()
            torch.cuda.synchronize()
            if r >= warmup:
                acc[i].append(a.elapsed_time(b))
            last[i] = out[0]
            del out
    equal = float((last[0].view(torch.int16) == last[1].view(torch.int16)).float().mean())
    res = [(statistics.median(t), min(t), max(t)) for t in acc]
    moved = 2 * B * H * T * D * 4

    def f(t):
        return f'{t[0]:9.4f} ({t[1]:.4f}..{t[2]:.4f})'
    k, c = res
    overlap = bool(k[2] >= c[1] and c[2] >= k[1])
    print(f'{f"T={T} {cfg_name}":24s} {f(k):>30s} {f(c):>32s} {k[0] / c[0]:12.4f} {str(overlap):>7s} '
          f'{moved / (k[0] * 1e-3) / 1e9:9.1f} {equal:9.6f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--txt', default=None)
    ap.add_argument('--step', default=None, help='internal: T,config of one child process')
    ap.add_argument('--limit', type=int, default=180, help='time limit of one step in seconds')
    args = ap.parse_args()
    if args.reps < 3 or args.warmup < 1:
        raise SystemExit('bench_kvquant: at least 3 repetitions and 1 warm-up')
    if args.step:
        T, name = args.step.split(',')
        step(int(T), name, args.reps, args.warmup)
        return
    lines = [f'KV-cache decode update, bf16, B = {B}, H = {H}, D = {D}: one update() of keys and values with one new token on T stored '
             f'rows; device events, {args.warmup} warm-up, median (min..max) of {args.reps} alternating repetitions, ms; fused = '
             'NaiveQuantKVCache.update (llmc_kv_cache_update); transcription = the reference\'s dequant / cat / contiguous / amax / '
             'amin / quant from torch ops on the same GPU; GB/s = 4 bytes per stored element of keys and values over the fused '
             'median; equal = share of the returned keys with the same bits on both sides',
             f'{"case":24s} {"fused ms":>30s} {"transcription ms":>32s} {"fused/transcr":>12s} {"overlap":>7s} {"GB/s":>9s} {"equal":>9s}']
    print('\n'.join(lines), flush=True)
    for T in TS:
        for name in CONFIGS:
            cmd = ['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--step', f'{T},{name}',
                   '--reps', str(args.reps), '--warmup', str(args.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f'bench_kvquant: step T={T} {name} ended with status {r.returncode}; nothing after it is run')
            row = r.stdout.strip().splitlines()[-1]
            print(row, flush=True)
            lines.append(row)
    if args.txt:
        os.makedirs(os.path.dirname(os.path.abspath(args.txt)), exist_ok=True)
        with open(args.txt, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
