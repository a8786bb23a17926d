"""Time ShortGPT's block score (sparse_ops.block_influence: llmc_block_influence, csrc/block_influence.hip) against the same
quantity composed row-wise from torch ops (block_influence_composed and an fp64 sum) on the same GPU, and, at N = 4096 only,
against the reference's formulation (shortgpt.py:49-55: two norms, input @ output.T, its diagonal, nan_to_num, 1 - sim, a sum in
the model dtype).

    python tools/bench_shortgpt.py --txt profiles/shortgpt.txt

The driver opens no GPU itself. It runs one child process per (N, d, dtype), each under `timeout -k 10`, one after the other, and
stops at the first that fails. A step: seeded features, output = input + noise; device events around one whole call (per-token
values and the fp64 total; host argument handling, the workspace and every launch included) ending in a synchronise, --warmup
calls per side first, the sides alternating inside every repetition, median with min..max of --reps.
MB = what the score must move, 2 * N * d * sizeof(dtype) + 4 * N; GB/s = MB over the kernel side's median call time (a call
time, not a kernel time: the profile file quotes the kernel time from a profiler run of its own).
err = the largest |kernel - composed| over the tokens. At N = 65536 the reference's formulation is not run: its N x N product
is 2 * N * N * d flop (35 TFLOP at d = 4096) and an N * N intermediate (8.6 GB in bf16); those figures are computed."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((4096, 4096), (65536, 4096), (65536, 8192))
DTYPES = ('bf16', 'f32')
REF_MAX_N = 4096


def reference_form(x, y):
    """shortgpt.py:49-55 and the .sum() of :64-66, from torch ops in the tensors' dtype"""
    sim = (x @ y.T) / (x.norm(dim=-1, keepdim=True) * y.norm(dim=-1, keepdim=True))
    return (1 - sim.diagonal().nan_to_num(nan=0.5)).sum()


def step(N, d, dname, reps, warmup):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_shortgpt: needs the GPU (no CPU fallback)')
    torch.set_grad_enabled(False)
    from llmc_amd.compression.sparsification import sparse_ops
    dt = {'bf16': torch.bfloat16, 'f32': torch.float32}[dname]
    gen = torch.Generator(device='cuda').manual_seed(N + d)
    x = torch.randn(N, d, generator=gen, device='cuda')
    y = (x + 0.3 * torch.randn(N, d, generator=gen, device='cuda')).to(dt)
    x = x.to(dt)
    total = torch.zeros((), dtype=torch.float64, device='cuda')

    def kernel():
        return sparse_ops.block_influence(x, y, total)[0]

    def composed():
        bi = sparse_ops.block_influence_composed(x, y)
        return bi, bi.double().sum()

    sides = [kernel, composed]
    if N <= REF_MAX_N:
        sides.append(lambda: reference_form(x, y))
    acc = [[] for _ in sides]
    for r in range(warmup + reps):
        for i, fn in enumerate(sides):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            torch.cuda.synchronize()
            if r >= warmup:
                acc[i].append(a.elapsed_time(b))
            del out
    err = float((kernel().double() - composed()[0].double()).abs().max())
    res = [(statistics.median(t), min(t), max(t)) for t in acc]
    moved = 2 * N * d * x.element_size() + 4 * N

    def f(t):
        return f'{t[0]:9.4f} ({t[1]:.4f}..{t[2]:.4f})'
    k, c = res[0], res[1]
    overlap = bool(k[2] >= c[1] and c[2] >= k[1])
    ref = f(res[2]) if len(res) > 2 else 'not run'
    print(f'{f"{N}x{d} {dname}":18s} {f(k):>30s} {f(c):>32s} {k[0] / c[0]:15.4f} {str(overlap):>7s} {ref:>32s} {moved / 1e6:9.2f} '
          f'{moved / (k[0] * 1e-3) / 1e9:9.1f} {err:9.2e}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--txt', default=None)
    ap.add_argument('--step', default=None, help='internal: N,d,dtype of one child process')
    ap.add_argument('--limit', type=int, default=180, help='time limit of one step in seconds')
    args = ap.parse_args()
    if args.reps < 3 or args.warmup < 1:
        raise SystemExit('bench_shortgpt: at least 3 repetitions and 1 warm-up')
    if args.step:
        N, d, dname = args.step.split(',')
        step(int(N), int(d), dname, args.reps, args.warmup)
        return
    lines = [f'ShortGPT block score of [N, d] input and output features: per-token 1 - cos and its fp64 sum; device events around a '
             f'whole call, {args.warmup} warm-up, median (min..max) of {args.reps} alternating repetitions, ms; kernel = '
             'llmc_block_influence (three launches); composed = the row-wise torch ops of block_influence_composed and an fp64 sum; '
             'reference form = norms, input @ output.T, diagonal, nan_to_num, 1 - sim, sum in the model dtype, run at N = 4096 only; '
             'MB = 2 N d sizeof(dtype) + 4 N; GB/s = MB over the kernel median; err = max |kernel - composed| per token',
             f'{"case":18s} {"kernel ms":>30s} {"composed ms":>32s} {"kernel/composed":>15s} {"overlap":>7s} {"reference form ms":>32s} '
             f'{"MB":>9s} {"GB/s":>9s} {"err":>9s}']
    print('\n'.join(lines), flush=True)
    for N, d in SHAPES:
        for dname in DTYPES:
            cmd = ['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--step', f'{N},{d},{dname}',
                   '--reps', str(args.reps), '--warmup', str(args.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f'bench_shortgpt: step {N}x{d} {dname} ended with status {r.returncode}; nothing after it is run')
            row = r.stdout.strip().splitlines()[-1]
            print(row, flush=True)
            lines.append(row)
    if args.txt:
        os.makedirs(os.path.dirname(os.path.abspath(args.txt)), exist_ok=True)
        with open(args.txt, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
