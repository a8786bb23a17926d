"""Time the pruning kernels (csrc/prune.hip through sparse_ops) against the torch-op compositions they replace, on the same GPU.

    python tools/bench_prune.py [--reps 9] [--txt profiles/prune.txt] [--json out.json]

  * prune_rows against prune_rows_composed (the reference's metric + stable sort + scatter + masked assignment), bf16 weights
    4096 x 4096, 1024 x 4096, 14336 x 4096, 4096 x 14336 (R x K), per row at sparsity 0.5 and n:m 2:4, with a scaler_row;
  * magnitude_prune against torch.sort(|W|.flatten())[0][kth] + masked assignment, and col_sqsum against
    x.float().pow(2).sum(0), at 262144 x 4096 bf16.
Pruning works in place, so every timed call starts from a fresh copy of the weight made outside the timed window. Times are
device events around one call, 2 warm-up calls per side, the sides alternating inside every repetition, median of --reps (>= 5)
with min..max. GB/s is on the algorithmic bytes: 2 * R * K * sizeof(dt) for the pruning calls (read once, write once), N * K *
sizeof(dt) for the column sums. The outputs are compared bit for bit at every timed shape (the column sums within the fp32
summation bound)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

WARMUP = 2
SHAPES = ((4096, 4096), (1024, 4096), (14336, 4096), (4096, 14336))
BIG = (262144, 4096)


def timed(sides, reps):
    """sides: (prep, fn) pairs; prep() runs outside the timed window and returns fn's argument"""
    for _ in range(WARMUP):
        for prep, fn in sides:
            fn(prep())
    torch.cuda.synchronize()
    acc = [[] for _ in sides]
    for _ in range(reps):
        for (prep, fn), t in zip(sides, acc):
            arg = prep()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(arg)
            b.record()
            torch.cuda.synchronize()
            t.append(a.elapsed_time(b))
            del arg
    return [(statistics.median(t), min(t), max(t)) for t in acc]


def row(case, path, nbytes, k, c, same):
    return dict(case=case, path=path, bytes=nbytes, kernel_ms=k, composed_ms=c, kernel_over_composed=k[0] / c[0],
                ranges_overlap=bool(k[2] >= c[1] and c[2] >= k[1]), same_bits=bool(same))


def bench_rows(reps):
    from llmc_amd.compression.sparsification import sparse_ops as S
    gen = torch.Generator(device='cuda').manual_seed(0)
    rows = []
    for R, K in SHAPES:
        w = (torch.randn(R, K, generator=gen, device='cuda') * 0.02).to(torch.bfloat16)
        scaler = torch.exp(torch.randn(K, generator=gen, device='cuda')) ** 2
        for tag, n, m in (('per_row_0.5', int(K * 0.5), None), ('2:4', 2, 4)):
            a, b = w.clone(), w.clone()
            S.prune_rows(a, scaler, n, m)
            S.prune_rows_composed(b, scaler, n, m)
            same = torch.equal(a.view(torch.int16), b.view(torch.int16))
            del a, b
            k, c = timed([(w.clone, lambda t: S.prune_rows(t, scaler, n, m)),
                          (w.clone, lambda t: S.prune_rows_composed(t, scaler, n, m))], reps)
            rows.append(row(f'prune_rows {R}x{K} {tag}', S.path(w, m), 2 * w.numel() * w.element_size(), k, c, same))
    return rows


def bench_big(reps):
    from llmc_amd.compression.sparsification import sparse_ops as S
    gen = torch.Generator(device='cuda').manual_seed(1)
    N, K = BIG
    x = torch.empty(N, K, dtype=torch.bfloat16, device='cuda')
    for i in range(0, N, 16384):          # filled in slabs: no fp32 image of the whole tensor
        x[i:i + 16384] = (torch.randn(16384, K, generator=gen, device='cuda') * 0.02).to(torch.bfloat16)
    rows = []
    # column sums
    ours, theirs = S.col_sqsum(x), x.float().pow(2).sum(0)
    same = bool(((ours - theirs).abs() <= 2 * (N + 1) * 2.0 ** -24 * theirs).all())
    k, c = timed([(lambda: x, lambda t: S.col_sqsum(t)), (lambda: x, lambda t: t.float().pow(2).sum(0))], reps)
    rows.append(row(f'col_sqsum {N}x{K}', '-', x.numel() * x.element_size(), k, c, same))
    del ours, theirs
    # global magnitude
    kth = int(x.numel() * 0.5)

    def composed(t):
        a = torch.abs(t)
        thresh = torch.sort(a.flatten())[0][kth]
        t[a <= thresh] = 0
    a, b = x.clone(), x.clone()
    S.magnitude_prune(a, kth)
    composed(b)
    same = torch.equal(a.view(torch.int16), b.view(torch.int16))
    del a, b
    torch.cuda.empty_cache()
    k, c = timed([(x.clone, lambda t: S.magnitude_prune(t, kth)), (x.clone, composed)], max(5, reps // 2))
    rows.append(row(f'magnitude_prune {N}x{K} kth = numel / 2', '-', 2 * x.numel() * x.element_size(), k, c, same))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--txt', default=None)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit('bench_prune: at least 5 repetitions')
    if not torch.cuda.is_available():
        raise SystemExit('bench_prune: needs the GPU (no CPU fallback)')
    torch.set_grad_enabled(False)
    rows = bench_rows(args.reps) + bench_big(args.reps)

    def f(t):
        return f'{t[0]:9.4f} ({t[1]:.4f}..{t[2]:.4f})'
    lines = [f'pruning kernels, bf16; device events, {WARMUP} warm-ups, median (min..max) of {args.reps} alternating repetitions '
             '(magnitude: at least 5); every call starts from a fresh copy made outside the timed window; GB/s on 2 * R * K * 2 bytes '
             '(col_sqsum: N * K * 2); composed = the reference\'s sequence from torch ops on the same GPU',
             f'{"case":44s} {"path":>9s} {"kernel ms":>30s} {"GB/s":>6s} {"composed ms":>32s} {"GB/s":>6s} {"k/composed":>10s} '
             f'{"overlap":>7s} {"same":>5s}']
    for r in rows:
        lines.append(f"{r['case']:44s} {r['path']:>9s} {f(r['kernel_ms']):>30s} {r['bytes'] / r['kernel_ms'][0] / 1e6:6.0f} "
                     f"{f(r['composed_ms']):>32s} {r['bytes'] / r['composed_ms'][0] / 1e6:6.0f} {r['kernel_over_composed']:10.4f} "
                     f"{str(r['ranges_overlap']):>7s} {str(r['same_bits']):>5s}")
    text = '\n'.join(lines)
    print(text)
    if args.txt:
        os.makedirs(os.path.dirname(os.path.abspath(args.txt)), exist_ok=True)
        with open(args.txt, 'w') as fh:
            fh.write(text + '\n')
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(rows, fh, indent=1)
    if not all(r['same_bits'] for r in rows):
        raise SystemExit('bench_prune: the kernel and the composition disagree')


if __name__ == '__main__':
    main()
