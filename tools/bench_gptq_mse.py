"""GPTQ column loop with min/max vs calib_algo 'mse' dynamic groups on the Llama-3-8B subsets (w4 asym g128, actorder).

    python tools/bench_gptq_mse.py [--reps 3]

Prints one JSON line per subset: quantize_stacked ms (Hessian prep, factorisation, column loop, unpermute) for min/max
and for mse, from the same H and W, and the difference, which is the per-block panel search on the chain.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from llmc_amd.compression.quantization.gptq_pipeline import GptqConfig, quantize_stacked  # noqa: E402

SUBSETS = [('qkv', [4096, 1024, 1024], 4096), ('o', [4096], 4096), ('gate_up', [14336, 14336], 4096),
           ('down', [4096], 14336)]


def time_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    for name, rows, K in SUBSETS:
        gen = torch.Generator(device='cuda').manual_seed(K + sum(rows))
        Ws = [(torch.randn(r, K, generator=gen, device='cuda') * 0.02).to(torch.bfloat16) for r in rows]
        X = torch.randn(K + 512, K, generator=gen, device='cuda')
        H = X.T @ X / X.shape[0]
        del X
        work = torch.empty_like(H)
        res = {'subset': name, 'R': sum(rows), 'K': K, 'group_size': 128}
        for algo, mse in (('minmax', None), ('mse', (True, 80, 100, 2.4))):
            cfg = GptqConfig(bit=4, symmetric=False, group_size=128, actorder=True, mse=mse)

            def run():
                work.copy_(H)
                quantize_stacked(Ws, work, cfg, want_losses=False)
            res[f'{algo}_ms'] = round(time_ms(run, args.reps), 3)
        res['mse_extra_ms'] = round(res['mse_ms'] - res['minmax_ms'], 3)
        res['blocks'] = K // 128
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
