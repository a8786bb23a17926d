"""Time sparse_ops.sparsegpt_prune (csrc/sparsegpt_loop.hip) against the published SparseGPT loop transcribed to torch ops on the
same GPU. The transcription (`fasterprune` below: Frantar & Alistarh 2023, sparsegpt.py of the paper's code, at blocksize 128 on
a given upper factor) lives here, not in the product.

One shape per process, each under its own time limit, chained so that a failure stops the rest:

    timeout -k 10 420 python tools/bench_sparsegpt.py --shape 4096x4096 --txt profiles/sparsegpt.txt && \
    timeout -k 10 600 python tools/bench_sparsegpt.py --shape 14336x4096 --txt profiles/sparsegpt.txt --append && \
    timeout -k 10 900 python tools/bench_sparsegpt.py --shape 4096x14336 --txt profiles/sparsegpt.txt --append

Shapes are R x K of a bf16 weight (taken to fp32, as the method does); modes sparsity 0.5 and 2:4. The factor U is a real one:
H = 2/T X^T X of seeded Gaussian X with per-column scales in [1, 4], damped by 0.01 mean(diag), through hessian_prep and
chol_inv_upper. Both sides overwrite their weight, so every timed call starts from a fresh fp32 copy made outside the timed
window. Times are device events around one call ending in a synchronise, --warmup calls per side first, the sides alternating
inside every repetition, median with min..max of --reps. The two sides are not bit-identical (the transcription's products go
through the BLAS, whose order of summation differs, and its n:m ties through topk), so the tool reports how far apart they are:
the share of equal mask entries and max |dWout| / max |Wout|."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

BLOCKSIZE = 128


def fasterprune(W, Hinv, sparsity, prunen=0, prunem=0, blocksize=BLOCKSIZE):
    """The published loop, op for op, in place on W (fp32 [rows, columns]); Hinv the upper factor. -> (W, mask)"""
    rows, columns = W.shape
    Losses = torch.zeros(rows, device=W.device)
    mask = torch.zeros_like(W, dtype=torch.bool)
    for i1 in range(0, columns, blocksize):
        i2 = min(i1 + blocksize, columns)
        count = i2 - i1
        W1 = W[:, i1:i2].clone()
        Q1 = torch.zeros_like(W1)
        Err1 = torch.zeros_like(W1)
        Losses1 = torch.zeros_like(W1)
        Hinv1 = Hinv[i1:i2, i1:i2]
        if prunen == 0:
            tmp = W1 ** 2 / (torch.diag(Hinv1).reshape((1, -1))) ** 2
            thresh = torch.sort(tmp.flatten())[0][int(tmp.numel() * sparsity)]
            mask1 = tmp <= thresh
        else:
            mask1 = torch.zeros_like(W1) == 1
        for i in range(count):
            w = W1[:, i]
            d = Hinv1[i, i]
            if prunen != 0 and i % prunem == 0:
                tmp = W1[:, i:(i + prunem)] ** 2 / (torch.diag(Hinv1)[i:(i + prunem)].reshape((1, -1))) ** 2
                mask1.scatter_(1, i + torch.topk(tmp, prunen, dim=1, largest=False)[1], True)
            q = w.clone()
            q[mask1[:, i]] = 0
            Q1[:, i] = q
            Losses1[:, i] = (w - q) ** 2 / d ** 2
            err1 = (w - q) / d
            W1[:, i:] -= err1.unsqueeze(1).matmul(Hinv1[i, i:].unsqueeze(0))
            Err1[:, i] = err1
        W[:, i1:i2] = Q1
        mask[:, i1:i2] = mask1
        Losses += torch.sum(Losses1, 1) / 2
        W[:, i2:] -= Err1.matmul(Hinv[i1:i2, i2:])
    return W, mask


def timed(sides, reps, warmup):
    """sides: (prep, fn) pairs; prep() runs outside the timed window and returns fn's argument"""
    for _ in range(warmup):
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


def make_inputs(R, K):
    from llmc_amd.compression.quantization import gptq_ops
    gen = torch.Generator(device='cuda').manual_seed(R + K)
    w = (torch.randn(R, K, generator=gen, device='cuda') * 0.02).to(torch.bfloat16)
    T = 2 * K
    scale = 1 + 3 * torch.rand(K, generator=gen, device='cuda')
    H = torch.zeros(K, K, device='cuda')
    for t0 in range(0, T, 4096):          # in slabs: no [T, K] fp32 image
        x = torch.randn(min(4096, T - t0), K, generator=gen, device='cuda') * scale
        H.addmm_(x.T, x, alpha=2.0 / T)
    Hp, _ = gptq_ops.hessian_prep(H, None, None, 0.01, want_h=True)
    del H
    U = gptq_ops.chol_inv_upper(Hp, check=True)          # Hp, overwritten by the factor
    gptq_ops.release_workspaces()
    return w, U


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', required=True, help='RxK, e.g. 4096x4096')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--txt', default=None)
    ap.add_argument('--append', action='store_true')
    args = ap.parse_args()
    if args.reps < 3 or args.warmup < 1:
        raise SystemExit('bench_sparsegpt: at least 3 repetitions and 1 warm-up')
    if not torch.cuda.is_available():
        raise SystemExit('bench_sparsegpt: needs the GPU (no CPU fallback)')
    torch.set_grad_enabled(False)
    from llmc_amd.compression.sparsification import sparse_ops as S
    R, K = (int(v) for v in args.shape.lower().split('x'))
    w, U = make_inputs(R, K)

    def fresh():
        return w.float()

    def f(t):
        return f'{t[0]:10.3f} ({t[1]:.3f}..{t[2]:.3f})'
    lines = []
    if not args.append:
        lines += [f'SparseGPT column loop, fp32 image of a bf16 weight R x K, real upper factor; device events, {args.warmup} warm-up, '
                  f'median (min..max) of {args.reps} alternating repetitions; every call starts from a fresh copy made outside the '
                  'timed window; transcription = the published fasterprune from torch ops on the same GPU; mask = / dWout: how far '
                  'apart the two results are (not bit-identical: BLAS summation order, topk ties)',
                  f'{"case":30s} {"kernel ms":>34s} {"transcription ms":>38s} {"kernel/transcr":>14s} {"overlap":>7s} {"mask =":>9s} '
                  f'{"dWout":>9s}']
    for tag, kw, tr in (('sparsity 0.5', dict(sparsity=0.5), (0.5, 0, 0)), ('2:4', dict(nm=(2, 4)), (0.0, 2, 4))):
        ours, _, mk = S.sparsegpt_prune(fresh(), U, want_mask=True, **kw)
        theirs, tmask = fasterprune(fresh(), U, *tr)
        agree = float((mk.bool() == tmask).float().mean())
        dw = float((ours - theirs).abs().max() / theirs.abs().max())
        del ours, theirs, mk, tmask
        k, c = timed([(fresh, lambda t: S.sparsegpt_prune(t, U, **kw)), (fresh, lambda t: fasterprune(t, U, *tr))], args.reps, args.warmup)
        overlap = bool(k[2] >= c[1] and c[2] >= k[1])
        lines.append(f'{f"{R}x{K} {tag}":30s} {f(k):>34s} {f(c):>38s} {k[0] / c[0]:14.5f} {str(overlap):>7s} {agree:9.6f} {dw:9.2e}')
    text = '\n'.join(lines)
    print(text)
    if args.txt:
        os.makedirs(os.path.dirname(os.path.abspath(args.txt)), exist_ok=True)
        with open(args.txt, 'a' if args.append else 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
