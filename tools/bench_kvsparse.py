"""Time one steady-state decode update() of SinkKVCache (kvsparse.py) on its fused path (llmc_kv_sink_update, csrc/kv_sink.hip)
against its composed path (the reference's slice / mul / cat sequence from torch ops) on the same GPU.

    python tools/bench_kvsparse.py --txt profiles/kvsparse.txt

The driver opens no GPU itself. It runs one child process per window length, each under `timeout -k 10`, one after the other, and
stops at the first that fails. A step: bf16, B = 1, H = 8, D = 128, 4 sink tokens; both caches are filled with W - 1 rows of
seeded states and RoPE tables, then one-token updates are timed (every one shifts the whole window and rotates the kept keys):
device events around one update() of keys and values ending in a synchronise, --warmup calls per side first, the two sides
alternating inside every repetition, median with min..max of --reps.
GB/s = the bytes the update must move, one read and one write of every cached element of keys and values (2 tensors x B * H * W * D
x 2 bytes x 2), over the median time of the whole call (host argument handling and launch included; not a kernel time).
equal = the share of the last returned keys' elements with the same bits on both sides."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, D, SINK = 1, 8, 128, 4
WS = (256, 4096, 32768)


def step(W, reps, warmup):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_kvsparse: needs the GPU (no CPU fallback)')
    torch.set_grad_enabled(False)
    from llmc_amd.compression.sparsification.kvsparse import SinkKVCache
    gen = torch.Generator(device='cuda').manual_seed(W)

    def states(n):
        return torch.randn(B, H, n, D, generator=gen, device='cuda').to(torch.bfloat16)

    ang = torch.outer(torch.arange(W + warmup + reps + 1, dtype=torch.float32), 1.0 / 10000.0 ** (torch.arange(0, D, 2) / float(D)))
    cos, sin = (torch.cat((f(ang), f(ang)), -1).to(torch.bfloat16).cuda() for f in (torch.cos, torch.sin))
    fused, composed = SinkKVCache(1, W, SINK), SinkKVCache(1, W, SINK)
    composed._fusable = False
    k0, v0 = states(W - 1), states(W - 1)
    kw = {'cos': cos[None, :W - 1], 'sin': sin[None, :W - 1]}
    fused.update(k0, v0, 0, kw)
    composed.update(k0, v0, 0, kw)
    assert fused._layers[0].fused and not composed._layers[0].fused
    del k0, v0
    sides = (fused, composed)
    acc, last = ([], []), [None, None]
    for r in range(warmup + reps):
        k, v = states(1), states(1)
        p = W - 1 + r
        kw = {'cos': cos[None, p:p + 1], 'sin': sin[None, p:p + 1]}
        for i, cache in enumerate(sides):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = cache.update(k, v, 0, kw)
            b.record()
            torch.cuda.synchronize()
            if r >= warmup:
                acc[i].append(a.elapsed_time(b))
            last[i] = out[0]
            del out
    assert fused._layers[0].fused and fused.get_seq_length() == composed.get_seq_length() == W
    equal = float((last[0].view(torch.int16) == last[1].view(torch.int16)).float().mean())
    res = [(statistics.median(t), min(t), max(t)) for t in acc]
    moved = 2 * B * H * W * D * 2 * 2

    def f(t):
        return f'{t[0]:9.4f} ({t[1]:.4f}..{t[2]:.4f})'
    k, c = res
    overlap = bool(k[2] >= c[1] and c[2] >= k[1])
    print(f'{f"W={W}":12s} {f(k):>30s} {f(c):>32s} {k[0] / c[0]:14.4f} {str(overlap):>7s} {moved / 1e6:9.2f} '
          f'{moved / (k[0] * 1e-3) / 1e9:9.1f} {equal:9.6f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--txt', default=None)
    ap.add_argument('--step', default=None, help='internal: W of one child process')
    ap.add_argument('--limit', type=int, default=180, help='time limit of one step in seconds')
    args = ap.parse_args()
    if args.reps < 3 or args.warmup < 1:
        raise SystemExit('bench_kvsparse: at least 3 repetitions and 1 warm-up')
    if args.step:
        step(int(args.step), args.reps, args.warmup)
        return
    lines = [f'SinkKV steady-state decode update, bf16, B = {B}, H = {H}, D = {D}, {SINK} sink tokens: one update() of keys and values '
             f'with one new token on a full window of W rows; device events, {args.warmup} warm-up, median (min..max) of {args.reps} '
             'alternating repetitions, ms; fused = llmc_kv_sink_update; composed = the reference\'s slice / mul / rotate_half / add / '
             'cat from torch ops on the same GPU; MB = one read and one write of every cached element of keys and values; GB/s = MB '
             'over the fused median; equal = share of the returned keys with the same bits on both sides',
             f'{"case":12s} {"fused ms":>30s} {"composed ms":>32s} {"fused/composed":>14s} {"overlap":>7s} {"MB":>9s} {"GB/s":>9s} {"equal":>9s}']
    print('\n'.join(lines), flush=True)
    for W in WS:
        cmd = ['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--step', str(W),
               '--reps', str(args.reps), '--warmup', str(args.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f'bench_kvsparse: step W={W} ended with status {r.returncode}; nothing after it is run')
        row = r.stdout.strip().splitlines()[-1]
        print(row, flush=True)
        lines.append(row)
    if args.txt:
        os.makedirs(os.path.dirname(os.path.abspath(args.txt)), exist_ok=True)
        with open(args.txt, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
