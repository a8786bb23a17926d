"""The W4A16 Linear on AutoAWQ's GEMM layout (csrc/awq_gemm.hip) on Llama-3-8B Linear shapes (K, R) at 1 .. 4096 tokens, g = 128, f16 and
bf16. Arms, timed in interleaved rounds inside one process with device events around batches of calls (median, min..max):

  (a) the module's forward        AutoawqRealQuantLinear.forward: awq_gemm_ops.LADDER's way, allocation included, one copy of the weight
  (b) llmc_awq_gemm               each rung by name, on preallocated buffers
  (c) awq_dequant + hip_linear    the 16-bit GEMM on the unpacked weight: the route a rung has to beat to get a row of the LADDER
  (d) hip_linear                  on a 16-bit weight

The parent commit cannot run this forward at all, so there is no parent time: the yardsticks are (c) and (d).
Below 1024 tokens (b), (c) and (d) walk round copies of their weight that together exceed the 256 MiB Infinity Cache, so every
call reads its weight from HBM as a decode step does. Every batch is sized to about 20 ms from a first timing of its arm; a row
of a few microseconds is still bounded below by the launch rate of one stream. Random operands, never zeros.
Rates: TB/s of the bytes a W4A16 product moves (packed weight, zeros, scales, x, y) below 1024 tokens, PFLOP/s from there on.
Peaks (MI355X, dense): ~2.5 PF for the 16-bit matrix instructions, 8 TB/s HBM.
Every (b) row carries its verdict against (c): a rung whose min..max range lies above (c)'s loses that shape.

    python tools/bench_awq_gemm.py [--rounds 5] [--out profiles/awq_gemm.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_fp8_linear import fmt, interleaved
from llmc_amd import _ffi
from llmc_amd.compression.quantization import IntegerQuantizer
from llmc_amd.compression.quantization.awq_gemm_ops import LADDER, RUNGS, awq_dequant, route
from llmc_amd.compression.quantization.module_utils import AutoawqRealQuantLinear, hip_linear

TOKENS = (1, 16, 64, 256, 1024, 4096)
SHAPES = ((4096, 4096), (4096, 6144), (4096, 28672), (14336, 4096))        # K x R: o, qkv, gate + up, down
ROTATE_BYTES = 320 << 20          # more than the Infinity Cache
G = 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--dtypes', default='f16,bf16')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the rates are measured on an MI355X only'
    L = _ffi.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'LADDER when measured: {LADDER}')
    gen = torch.Generator(device='cuda').manual_seed(0)
    q = IntegerQuantizer(4, False, 'per_group', group_size=G)
    cfg = {'weight': {'bit': 4, 'group_size': G, 'pack_version': 'gemm_pack'}}
    for dname in args.dtypes.split(','):
        dtype = {'f16': torch.float16, 'bf16': torch.bfloat16}[dname]
        for K, R in SHAPES:
            lin = torch.nn.Linear(K, R, bias=False, device='cuda', dtype=torch.float16)
            lin.weight.data.copy_(torch.randn(R, K, generator=gen, device='cuda') * 0.02)
            mod = AutoawqRealQuantLinear.new(lin, lambda m: q.real_quant_weight_dynamic(m.weight.data), cfg)
            qw, qz, sc = mod.qweight, mod.qzeros, mod.scales
            w16 = lin.weight.data.to(dtype)
            qw_rot = [qw] + [qw.clone() for _ in range(-(-ROTATE_BYTES // (qw.numel() * 4)) - 1)]
            w16_rot = [w16] + [w16.clone() for _ in range(-(-ROTATE_BYTES // (w16.numel() * 2)) - 1)]
            for M in TOKENS:
                x = torch.randn(M, K, generator=gen, device='cuda').to(dtype)
                y = torch.empty(M, R, dtype=dtype, device='cuda')
                ws = _ffi.workspace(L.llmc_awq_gemm_ws_bytes(M, K, R), 'cuda')
                st, turn = _ffi.stream(), [0]

                def pick(copies):
                    if M >= 1024:
                        return copies[0]
                    turn[0] += 1
                    return copies[turn[0] % len(copies)]

                def gemm(rung):
                    _ffi.check(L.llmc_awq_gemm(_ffi.ptr(x), _ffi.dt(dtype), M, K, R, _ffi.ptr(pick(qw_rot)), _ffi.ptr(qz), _ffi.ptr(sc), G,
                                               None, _ffi.ptr(y), _ffi.ptr(ws), st, rung), 'llmc_awq_gemm')

                way = route(M, K, R)
                arms = {f'(a) module forward [{way}: the LADDER]': lambda: mod(x)}
                for name, r in RUNGS.items():
                    arms[f'(b) llmc_awq_gemm [{name}]'] = lambda r=r: gemm(r)
                arms['(c) awq_dequant + hip_linear'] = lambda: hip_linear(x, awq_dequant(pick(qw_rot), qz, sc, G, dtype), None)
                arms[f'(d) hip_linear, {dname} weight'] = lambda: hip_linear(x, pick(w16_rot), None)
                ts = interleaved(arms, args.rounds)
                fl = 2.0 * M * K * R
                nbytes = float(K * R // 2 + (K // G) * R * 2 + (K // G) * R // 2 + 2 * M * K + 2 * M * R)
                say(f'{dname} tokens={M} K={K} R={R}  ({args.rounds} interleaved rounds of about 20 ms per arm; median, min, max per call)')
                tc = ts['(c) awq_dequant + hip_linear']
                for k in arms:
                    t, text = fmt(ts[k])
                    tail = f'{fl / t / 1e15:.3f} PFLOP/s' if M >= 1024 else f'{nbytes / t / 1e12:.2f} TB/s of {nbytes / 1e6:.1f} MB'
                    if k.startswith('(b)'):
                        tail += ('  — beats (c), ranges apart' if ts[k][-1] < tc[0] else '  — loses to (c), ranges apart' if ts[k][0] > tc[-1]
                                 else '  — ranges overlap with (c)')
                    say(f'  {k:44s}{text} = {tail}')
            del qw_rot, w16_rot, mod, lin
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
