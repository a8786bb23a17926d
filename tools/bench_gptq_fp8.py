"""Time GPTQ's column loop alone (gptq_ops.gptq_quantize: the in-block kernels and the trailing updates, no Hessian, no
factorisation) per_channel at 4096x4096, 14336x4096 and 4096x14336, on the integer grid and on the FP8 grids.

    python tools/bench_gptq_fp8.py [--reps 5] [--arms int8,e4m3,e4m3_generic,e5m2,e5m2_generic] [--json out.json]
    python tools/bench_gptq_fp8.py --package-root OTHER_CHECKOUT --arms int8      # the same loop of another checkout

Arms: int8 = W8 symmetric per_channel (llmc_gptq_quantize_cols); e4m3 / e5m2 = the FloatQuantizer grids on the default
in-block path (the fast path); *_generic = the same with the generic in-block path forced (option gptq_generic). Every arm
runs the same seeded weights and the same upper factor (of a damped random Hessian's inverse); the loop overwrites its weight
operand, so each repetition starts from a fresh copy made outside the timed window. Times are device events around one call
after a warm-up call per arm and shape; the arms of a shape are timed interleaved (rep 0 of every arm, then rep 1, ...), so
drift of the machine hits all of them alike. Reported: median, min and max of --reps repetitions, in ms."""
import argparse
import contextlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(4096, 4096), (14336, 4096), (4096, 14336)]
ARMS = ('int8', 'e4m3', 'e4m3_generic', 'e5m2', 'e5m2_generic')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--arms', default=','.join(ARMS))
    ap.add_argument('--package-root', default=ROOT, help='directory holding the llmc_amd package to time')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_gptq_fp8: needs the GPU (no CPU fallback)')
    from llmc_amd import _ffi
    from llmc_amd.compression.quantization import gptq_ops
    arms = [a for a in args.arms.split(',') if a]
    assert all(a in ARMS for a in arms), arms

    def call(arm, W, U, scales):
        if arm == 'int8':
            return gptq_ops.gptq_quantize(W, U, True, -128.0, 127.0, 0, scales=scales['int8'], want_losses=True)
        fmt = arm.split('_')[0]
        ctx = _ffi.option(gptq_generic=1) if arm.endswith('_generic') else contextlib.nullcontext()
        with ctx:
            return gptq_ops.gptq_quantize(W, U, True, 0.0, 0.0, 0, scales=scales[fmt], want_losses=True, fp8=fmt)

    res = {'what': 'GPTQ column loop alone, per_channel, ms per call', 'reps': args.reps,
           'package_root': os.path.abspath(args.package_root), 'shapes': {}}
    for R, K in SHAPES:
        gen = torch.Generator(device='cuda').manual_seed(R + K)
        n = max(K // 4, 512)
        X = torch.randn(n, K, generator=gen, device='cuda')
        X[:, ::5] *= 4
        H = (X.T @ X) / n
        del X
        H.diagonal().add_(0.05 * float(H.diagonal().mean()))
        U = gptq_ops.chol_inv_upper(H).clone()
        W0 = (torch.randn(R, K, generator=gen, device='cuda') * 0.02).to(torch.bfloat16).float()
        amax = W0.abs().amax(dim=1, keepdim=True).clamp(min=1e-5)
        scales = {'int8': (amax / 127.0).to(torch.bfloat16).float(), 'e4m3': (amax / 448.0).to(torch.bfloat16).float(),
                  'e5m2': (amax / 57344.0).to(torch.bfloat16).float()}
        times = {a: [] for a in arms}
        for a in arms:                                   # warm-up: code objects, workspaces
            call(a, W0.clone(), U, scales)
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for a in arms:
                W = W0.clone()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(a, W, U, scales)
                e1.record()
                torch.cuda.synchronize()
                times[a].append(e0.elapsed_time(e1))
        res['shapes'][f'{R}x{K}'] = {a: {'median': statistics.median(t), 'min': min(t), 'max': max(t), 'all': t}
                                     for a, t in times.items()}
        del U, H, W0
        gptq_ops.release_workspaces()
        for a in arms:
            t = times[a]
            print(f'{R}x{K} {a:13s} median {statistics.median(t):8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}', flush=True)
    print(json.dumps(res))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
