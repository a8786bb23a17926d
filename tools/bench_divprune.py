"""Time DivPrune's selection (divprune(): llmc_cosine_dist + llmc_maxmin_select, csrc/token_select.hip) against the reference's op
sequence on the same GPU (cosine_distance_composed chained with maxmin_select_composed: norm, division, mm, 1 -, then per step
index_select, min, argmax and a scalar write), and the two kernels alone against their compositions.

    python tools/bench_divprune.py --txt profiles/divprune.txt

The driver opens no GPU itself. It runs one child process per (N, d, ratio, dtype), each under `timeout -k 10`, one after the other,
and stops at the first that fails. A step: seeded random features; device events around one whole call (host argument handling,
the workspace and every launch included) ending in a synchronise, --warmup calls per side first, the sides alternating inside every
repetition, median with min..max of --reps. k = int(round(ratio * N)). `same` = the kernel route and the composition chose the same
indices on the kernel's own matrix (on random features the two matrices differ by roundings and need not choose alike)."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((576, 4096, 0.1), (576, 4096, 0.5), (2880, 4096, 0.25))
DTYPES = ('bf16', 'f16')


def step(N, d, ratio, dname, reps, warmup):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_divprune: needs the GPU')
    torch.set_grad_enabled(False)
    from llmc_amd.compression.token_reduction import token_ops
    from llmc_amd.compression.token_reduction.divprune import divprune
    dt = {'bf16': torch.bfloat16, 'f16': torch.float16}[dname]
    gen = torch.Generator(device='cuda').manual_seed(N + d)
    x = torch.randn(N, d, generator=gen, device='cuda').to(dt)
    k = int(round(ratio * N))
    D = token_ops.cosine_distance(x)

    sides = [lambda: divprune(x, N, None, ratio)[0],
             lambda: token_ops.maxmin_select_composed(token_ops.cosine_distance_composed(x), k),
             lambda: token_ops.cosine_distance(x), lambda: token_ops.cosine_distance_composed(x),
             lambda: token_ops.maxmin_select(D, k), lambda: token_ops.maxmin_select_composed(D, k)]
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
    same = bool(torch.equal(token_ops.maxmin_select(D, k), token_ops.maxmin_select_composed(D, k)))
    res = [(statistics.median(t), min(t), max(t)) for t in acc]

    def f(t):
        return f'{t[0]:.3f} ({t[1]:.3f}..{t[2]:.3f})'

    def pair(a, b):
        overlap = bool(a[2] >= b[1] and b[2] >= a[1])
        return f'{f(a):>26s} {f(b):>30s} {a[0] / b[0]:7.3f} {str(overlap):>7s}'
    print(f'{f"{N}x{d} r{ratio} {dname}":24s} {pair(res[0], res[1])} | {pair(res[2], res[3])} | {pair(res[4], res[5])} {str(same):>5s}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--txt', default=None)
    ap.add_argument('--step', default=None, help='internal: N,d,ratio,dtype of one child process')
    ap.add_argument('--limit', type=int, default=240, help='time limit of one step in seconds')
    args = ap.parse_args()
    if args.reps < 3 or args.warmup < 1:
        raise SystemExit('bench_divprune: at least 3 repetitions and 1 warm-up')
    if args.step:
        N, d, ratio, dname = args.step.split(',')
        step(int(N), int(d), float(ratio), dname, args.reps, args.warmup)
        return
    head = f'{"kernel ms":>26s} {"composed ms":>30s} {"k/c":>7s} {"overlap":>7s}'
    lines = [f'DivPrune on [N, d] random features, k = round(ratio N): device events around a whole call, {args.warmup} warm-up, median '
             f'(min..max) of {args.reps} alternating repetitions, ms. Three pairs per row: divprune() against the reference\'s op sequence '
             '(cosine_distance_composed + maxmin_select_composed); llmc_cosine_dist against cosine_distance_composed; '
             'llmc_maxmin_select against maxmin_select_composed on the kernel\'s matrix. same = the last pair chose the same indices',
             f'{"case":24s} {head} | {head} | {head} {"same":>5s}']
    print('\n'.join(lines), flush=True)
    for N, d, ratio in CASES:
        for dname in DTYPES:
            cmd = ['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--step', f'{N},{d},{ratio},{dname}',
                   '--reps', str(args.reps), '--warmup', str(args.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f'bench_divprune: step {N}x{d} r{ratio} {dname} ended with status {r.returncode}; nothing after it is run')
            row = r.stdout.strip().splitlines()[-1]
            print(row, flush=True)
            lines.append(row)
    if args.txt:
        os.makedirs(os.path.dirname(os.path.abspath(args.txt)), exist_ok=True)
        with open(args.txt, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
