"""OCP MX kernels (csrc/mx_gemm.hip) on the Llama-3-8B Linear shapes at 4096 tokens: sustained rates of mx_act_quant, mx_gemm
and the whole MxFp4 forward (act quant + GEMM), beside the route the same stored weight had before the GEMM existed:
dequant_fpx + hip_linear on the bf16 activation. Device events around batches of calls; the arms are timed in interleaved
rounds inside one process, median and min-max spread over the rounds are reported. Random operands (a quantized Gaussian
weight, Gaussian activations with per-channel spread), never zeros.

Peaks (MI355X, dense): ~10 PF FP4, ~5 PF block-scaled FP8 (the 8-bit operand sets the instruction's rate), 8 TB/s HBM.

    python tools/bench_mx_gemm.py [--rounds 7] [--out profiles/mx_gemm_rates.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from llmc_amd.compression.quantization import FloatQuantizer
from llmc_amd.compression.quantization.module_utils import hip_linear
from llmc_amd.compression.quantization.mx_ops import mx_act_quant, mx_gemm, mx_linear_forward
from llmc_amd.compression.quantization.quant import dequant_fpx

TOKENS = 4096
SHAPES = ((4096, 4096), (14336, 4096), (4096, 14336))        # N x K
PEAK = {'e2m1': 10e15, 'e4m3': 5e15}


def batch_time(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls


def interleaved(arms, rounds, calls):
    """arms: name -> fn. Every round times every arm once (a batch of `calls`), in turn. name -> sorted per-call times."""
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ts[k].append(batch_time(fn, calls))
    return {k: sorted(v) for k, v in ts.items()}


def fmt(ts):
    med = ts[len(ts) // 2]
    return med, f'{med * 1e6:8.1f} us (min {ts[0] * 1e6:.1f}, max {ts[-1] * 1e6:.1f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the rates are measured on an MI355X only'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device='cuda').manual_seed(0)
    wq = FloatQuantizer('e2m1', True, 'per_group', group_size=32, use_qtorch=True, float_semantics='ocp', scale_format='e8m0')
    M = TOKENS
    for N, K in SHAPES:
        x = (torch.randn(M, K, generator=g, device='cuda') * torch.exp(0.5 * torch.randn(K, generator=g, device='cuda'))).to(torch.bfloat16)
        w = (torch.randn(N, K, generator=g, device='cuda') * 0.02).to(torch.bfloat16)
        wp, ws, _ = wq.real_quant_weight_dynamic(w)
        ws = ws.reshape(N, K // 32).contiguous()
        fl = 2.0 * M * N * K
        q = {bit: mx_act_quant(x, bit) for bit in PEAK}
        arms = {'parent route: dequant_fpx + hip_linear (bf16 activation)': lambda: hip_linear(x, dequant_fpx(wp, ws, 'e2m1', 32, torch.bfloat16), None)}
        for bit in PEAK:
            arms[f'mx_act_quant {bit}'] = lambda bit=bit: mx_act_quant(x, bit)
            arms[f'mx_gemm {bit} x e2m1'] = lambda bit=bit: mx_gemm(q[bit][0], q[bit][1], bit, wp, ws)
            arms[f'forward {bit} (act quant + GEMM)'] = lambda bit=bit: mx_linear_forward(x, wp, ws, bit, None)
        ts = interleaved(arms, args.rounds, args.calls)
        say(f'tokens={M} N={N} K={K}  ({args.rounds} interleaved rounds of {args.calls} calls; median, min, max per call)')
        base, text = fmt(ts['parent route: dequant_fpx + hip_linear (bf16 activation)'])
        say(f'  parent route: dequant_fpx + hip_linear  {text} = {fl / base / 1e15:.3f} PFLOP/s')
        for bit in PEAK:
            t, text = fmt(ts[f'mx_act_quant {bit}'])
            nbytes = M * K * (2 + (0.5 if bit == 'e2m1' else 1.0) + 1.0 / 32)
            say(f'  mx_act_quant {bit}                      {text} = {nbytes / t / 1e12:.2f} TB/s of {nbytes / 1e6:.1f} MB (X read once + codes + scales)')
            t, text = fmt(ts[f'mx_gemm {bit} x e2m1'])
            say(f'  mx_gemm {bit} x e2m1                    {text} = {fl / t / 1e15:.3f} PFLOP/s = {fl / t / PEAK[bit]:.3f} of the {PEAK[bit] / 1e15:.0f} PF '
                f'{"FP4" if bit == "e2m1" else "block-scaled FP8"} peak')
            t, text = fmt(ts[f'forward {bit} (act quant + GEMM)'])
            say(f'  forward {bit} (act quant + GEMM)        {text} = {fl / t / 1e15:.3f} PFLOP/s, {base / t:.2f} x the parent route')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
