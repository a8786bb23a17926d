"""MXFP6 kernels (csrc/mx6_gemm.hip) on the Llama-3-8B Linear shapes at 1, 16 and 4096 tokens: llmc_mx6_gemm on each rung that
takes the shape, beside llmc_mx_gemm (MXFP4 x MXFP4) on the same layer in the same run, and the whole MxFp6 forward (act quant +
GEMM) beside the route the stored weight has without the GEMM: unpack + dequant_fpx + hip_linear on the bf16 activation. Device
events around batches of calls; the arms are timed in interleaved rounds inside one process, median and min-max spread over the
rounds are reported. Random operands (quantized Gaussian weights, Gaussian activations with per-channel spread), never zeros.
Decode rows also give the weight bytes per second (codes + scales of the weight over the call time; HBM peak 8 TB/s).

    python tools/bench_mx6.py [--rounds 7] [--out profiles/mx6_gemm.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_mx_gemm import fmt, interleaved
from llmc_amd.compression.quantization import FloatQuantizer
from llmc_amd.compression.quantization.module_utils import hip_linear
from llmc_amd.compression.quantization.mx_ops import (mx6_act_quant, mx6_gemm, mx6_linear_forward, mx6_pack, mx6_unpack, mx_act_quant,
                                                      mx_gemm)
from llmc_amd.compression.quantization.quant import dequant_fpx

TOKENS = (1, 16, 4096)
SHAPES = ((4096, 4096), (14336, 4096), (4096, 14336))        # N x K
RUNGS = ('decode', 'tile128')


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
    mk = lambda bit: FloatQuantizer(bit, True, 'per_group', group_size=32, use_qtorch=True, float_semantics='ocp', scale_format='e8m0')
    for N, K in SHAPES:
        w = (torch.randn(N, K, generator=g, device='cuda') * 0.02).to(torch.bfloat16)
        c6, s6, _ = mk('e3m2').real_quant_weight_dynamic(w)
        w6, s6 = mx6_pack(c6.reshape(N, K)), s6.reshape(N, K // 32).contiguous()
        w4, s4, _ = mk('e2m1').real_quant_weight_dynamic(w)
        s4 = s4.reshape(N, K // 32).contiguous()
        for M in TOKENS:
            x = (torch.randn(M, K, generator=g, device='cuda') * torch.exp(0.5 * torch.randn(K, generator=g, device='cuda'))).to(torch.bfloat16)
            a6, a4 = mx6_act_quant(x), mx_act_quant(x, 'e2m1')
            rungs = [r for r in range(2) if r == 1 or M <= 16]
            arms = {'route without the GEMM: unpack + dequant_fpx + hip_linear': lambda: hip_linear(x, dequant_fpx(mx6_unpack(w6), s6, 'e3m2', 32, torch.bfloat16), None),
                    'mx_gemm e2m1 x e2m1 (MXFP4)': lambda: mx_gemm(a4[0], a4[1], 'e2m1', w4, s4),
                    'mx6_act_quant': lambda: mx6_act_quant(x),
                    'mx6 forward (act quant + GEMM)': lambda: mx6_linear_forward(x, w6, s6, None)}
            for r in rungs:
                arms[f'mx6_gemm rung {RUNGS[r]}'] = lambda r=r: mx6_gemm(a6[0], a6[1], w6, s6, rung=r)
            ts = interleaved(arms, args.rounds, args.calls)
            fl = 2.0 * M * N * K
            say(f'tokens={M} N={N} K={K}  ({args.rounds} interleaved rounds of {args.calls} calls; median, min, max per call)')
            t4, text = fmt(ts['mx_gemm e2m1 x e2m1 (MXFP4)'])
            say(f'  mx_gemm e2m1 x e2m1 (MXFP4)           {text} = {fl / t4 / 1e15:.3f} PFLOP/s')
            for r in rungs:
                t, text = fmt(ts[f'mx6_gemm rung {RUNGS[r]}'])
                wb = N * K * (0.75 + 1.0 / 32)
                say(f'  mx6_gemm rung {RUNGS[r]:<8}               {text} = {fl / t / 1e15:.3f} PFLOP/s, {t4 / t:.2f} x the MXFP4 GEMM'
                    + (f', {wb / t / 1e12:.2f} TB/s of weight ({wb / 1e6:.1f} MB)' if M <= 16 else ''))
            t, text = fmt(ts['mx6_act_quant'])
            say(f'  mx6_act_quant                         {text}')
            base, text = fmt(ts['route without the GEMM: unpack + dequant_fpx + hip_linear'])
            say(f'  unpack + dequant_fpx + hip_linear     {text}')
            t, text = fmt(ts['mx6 forward (act quant + GEMM)'])
            say(f'  mx6 forward (act quant + GEMM)        {text} = {base / t:.2f} x that route')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
