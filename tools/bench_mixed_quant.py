"""Time the mixed int / fp column kernel (llmc_quant_dynamic_mixed, csrc/mixed_quant.hip) against the composition of existing
kernels it replaces (mixed_ops.fake_quant_mixed_composed: index_select -> llmc_quant_dynamic -> two index_copy_ into zeros),
on the same GPU, at the shapes QUIK and LLM.int8() run on every forward.

    python tools/bench_mixed_quant.py [--reps 9] [--txt profiles/mixed_quant.txt] [--json out.json]

  * activations [2048, K], K = 4096 / 14336 / 28672, bf16, int8 symmetric per_token, 256 outlier columns, the integer columns
    in QUIK's order (ascending activation scale: scattered over the row);
  * weights 4096 x 4096 bf16: int8 symmetric per_channel, and int4 asymmetric per_group g = 128 (3840 integer columns in
    scale order, 256 fp).
Both sides include what a caller pays per call: the kernel side builds the role mask and the int32 index copy with torch ops,
the composition gathers and scatters. Times are device events around one call, 2 warm-up calls per side, the two sides
alternating inside every repetition, median of --reps (>= 5). GB/s is on the algorithmic bytes 2 * N * K * sizeof(dt) (one
read, one write of the tensor) for both sides. The outputs of the two sides are compared bit for bit at every timed shape."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

WARMUP = 2


def timed_pair(fa, fb, reps):
    for _ in range(WARMUP):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, acc in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            acc.append(a.elapsed_time(b))
    return statistics.median(ta), statistics.median(tb), (min(ta), max(ta)), (min(tb), max(tb))


def case(tag, N, K, g, sym, qmin, qmax, gen):
    c = torch.exp(0.5 * torch.randn(K, generator=gen, device='cuda'))
    c[torch.randperm(K, generator=gen, device='cuda')[:256]] *= 30
    x = (torch.randn(N, K, generator=gen, device='cuda') * c).to(torch.bfloat16)
    order = torch.sort(x.abs().amax(0).float(), stable=True)[1]       # QUIK's order: ascending activation scale
    return dict(tag=tag, x=x, ints=order[:K - 256].contiguous(), fp=order[K - 256:].contiguous(), g=g or K - 256, sym=sym,
                qmin=qmin, qmax=qmax)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--txt', default=None)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit('bench_mixed_quant: at least 5 repetitions')
    if not torch.cuda.is_available():
        raise SystemExit('bench_mixed_quant: needs the GPU (no CPU fallback)')
    from llmc_amd.compression.quantization import mixed_ops
    torch.set_grad_enabled(False)
    gen = torch.Generator(device='cuda').manual_seed(0)
    cases = [case(f'act_2048x{K}_int8_per_token', 2048, K, None, True, -128.0, 127.0, gen) for K in (4096, 14336, 28672)]
    cases.append(case('w_4096x4096_int8_per_channel', 4096, 4096, None, True, -128.0, 127.0, gen))
    cases.append(case('w_4096x4096_int4_asym_g128', 4096, 4096, 128, False, 0.0, 15.0, gen))
    rows = []
    for c in cases:
        x = c['x']
        a = (x, c['ints'], c['fp'], c['g'], c['sym'], True, c['qmin'], c['qmax'])
        if not mixed_ops.kernel_takes(x):
            raise SystemExit(f"{c['tag']}: the resident kernel does not take this width")
        same = torch.equal(mixed_ops.fake_quant_mixed(*a).view(torch.int16), mixed_ops.fake_quant_mixed_composed(*a).view(torch.int16))
        k_ms, c_ms, k_rng, c_rng = timed_pair(lambda: mixed_ops.fake_quant_mixed(*a), lambda: mixed_ops.fake_quant_mixed_composed(*a),
                                              args.reps)
        nbytes = 2 * x.numel() * x.element_size()
        rows.append(dict(case=c['tag'], bytes=nbytes, kernel_ms=k_ms, composed_ms=c_ms, kernel_GBps=nbytes / k_ms / 1e6,
                         composed_GBps=nbytes / c_ms / 1e6, kernel_over_composed=k_ms / c_ms, kernel_min_max_ms=k_rng,
                         composed_min_max_ms=c_rng, same_bits=bool(same)))
    lines = [f'mixed int / fp column pass, bf16, 256 fp columns in scale order; device events, {WARMUP} warm-ups, median of '
             f'{args.reps} alternating repetitions; GB/s on 2 * N * K * 2 bytes',
             f'{"case":34s} {"kernel ms":>10s} {"GB/s":>8s} {"composed ms":>12s} {"GB/s":>8s} {"kernel/composed":>16s} {"same bits":>10s}']
    for r in rows:
        lines.append(f"{r['case']:34s} {r['kernel_ms']:10.4f} {r['kernel_GBps']:8.0f} {r['composed_ms']:12.4f} "
                     f"{r['composed_GBps']:8.0f} {r['kernel_over_composed']:16.3f} {str(r['same_bits']):>10s}")
        lines.append(f"{'':34s} min..max {r['kernel_min_max_ms'][0]:.4f}..{r['kernel_min_max_ms'][1]:.4f}"
                     f"{'':14s}{r['composed_min_max_ms'][0]:.4f}..{r['composed_min_max_ms'][1]:.4f}")
    text = '\n'.join(lines)
    print(text)
    print(json.dumps(rows))
    if args.txt:
        os.makedirs(os.path.dirname(os.path.abspath(args.txt)), exist_ok=True)
        with open(args.txt, 'w') as fh:
            fh.write(text + '\n')
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(rows, fh, indent=1)
    if not all(r['same_bits'] for r in rows):
        raise SystemExit('bench_mixed_quant: the kernel and the composition disagree')


if __name__ == '__main__':
    main()
