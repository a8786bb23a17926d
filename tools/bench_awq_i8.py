"""The W4A8 Linear on AutoAWQ's GEMM layout (csrc/awq_i8_gemm.hip) on Llama-3-8B Linear shapes (K, R) at 1 .. 4096 tokens, g = 128, bf16
activations and outputs, int8 per-token activation codes. Arms, timed in interleaved rounds inside one process with device events
around batches of calls (median, min..max: the run-to-run spread a difference has to exceed):

  (a) awq_i8_linear_forward       the deployed W4A8 module's whole forward: activation quantization + awq_gemm_ops.I8_LADDER's way
  (p) awq_linear_forward          the parent commit's forward of the same module: W4A16 on the unquantized activation
  (b) llmc_awq_i8_gemm            alone, each rung by name, on preallocated buffers (the stream rung up to 256 tokens)
  (c) i8_dequant + W4A16          the fallback: the activation codes back to bf16, then awq_linear_forward — the route a rung has to
                                  beat to get a row of the I8_LADDER
  (d) llmc_i8_scaled_gemm         on an int8 weight of the same shape: the ceiling (the same MFMA work without the nibble opening and
                                  the group folds, twice the weight bytes)

Below 1024 tokens (b) and (d) walk round copies of their weight that together exceed the 256 MiB Infinity Cache, so every call
reads its weight from HBM as a decode step does. Every batch is sized to about 20 ms from a first timing of its arm. Random
operands, never zeros. Rates: TB/s of the bytes a W4A8 product moves below 1024 tokens, POP/s from there on.
Every (b) row carries its verdict against (c): a rung whose min..max range lies above (c)'s loses that shape.

    python tools/bench_awq_i8.py [--rounds 5] [--out profiles/awq_i8_gemm.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bench_fp8_linear import fmt, interleaved

from llmc_amd import _ffi
from llmc_amd.compression.quantization import IntegerQuantizer
from llmc_amd.compression.quantization.awq_gemm_ops import I8_LADDER, I8_RUNGS, awq_i8_linear_forward, awq_linear_forward, i8_route
from llmc_amd.compression.quantization.i8_linear_ops import i8_act_quant, i8_dequant
from llmc_amd.compression.quantization.module_utils import AutoawqRealQuantLinear

TOKENS = (1, 16, 64, 256, 1024, 4096)
SHAPES = ((4096, 4096), (4096, 6144), (4096, 28672), (14336, 4096))        # K x R: o, qkv, gate + up, down
ROTATE_BYTES = 320 << 20          # more than the Infinity Cache
STREAM_MAX_M = 256                # the stream rung re-reads the weight for every 32 rows: not timed beyond
G = 128
ACT = dict(bit=8, symmetric=True, granularity='per_token')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the rates are measured on an MI355X only'
    L = _ffi.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'I8_LADDER when measured: {I8_LADDER}')
    gen = torch.Generator(device='cuda').manual_seed(0)
    q, aq = IntegerQuantizer(4, False, 'per_group', group_size=G), IntegerQuantizer(**ACT)
    cfg = {'weight': {'bit': 4, 'group_size': G, 'pack_version': 'gemm_pack'}}
    bf16, st = _ffi.dt(torch.bfloat16), _ffi.stream()
    for K, R in SHAPES:
        lin = torch.nn.Linear(K, R, bias=False, device='cuda', dtype=torch.float16)
        lin.weight.data.copy_(torch.randn(R, K, generator=gen, device='cuda') * 0.02)
        mod = AutoawqRealQuantLinear.new(lin, lambda m: q.real_quant_weight_dynamic(m.weight.data), cfg)
        qw, qz, sc = mod.qweight, mod.qzeros, mod.scales
        w8 = torch.randint(-127, 128, (R, K), generator=gen, device='cuda', dtype=torch.int8)         # (d) is a timing arm
        w_s = torch.full((R,), 0.01, device='cuda')
        qw_rot = [qw] + [qw.clone() for _ in range(-(-ROTATE_BYTES // (qw.numel() * 4)) - 1)]
        w8_rot = [w8] + [w8.clone() for _ in range(-(-ROTATE_BYTES // w8.numel()) - 1)]
        del lin
        for M in TOKENS:
            x = torch.randn(M, K, generator=gen, device='cuda').to(torch.bfloat16)
            a8, a_s = i8_act_quant(x, aq)
            a_s32 = a_s.reshape(-1).contiguous()
            y = torch.empty(M, R, dtype=torch.bfloat16, device='cuda')
            nws = max(L.llmc_awq_i8_gemm_ws_bytes(M, K, R, G), L.llmc_i8_scaled_gemm_ws_bytes(M, R, K), 16)
            ws, turn = _ffi.workspace(nws, 'cuda'), [0]

            def pick(copies):
                if M >= 1024:
                    return copies[0]
                turn[0] += 1
                return copies[turn[0] % len(copies)]

            def w4a8(rung):
                _ffi.check(L.llmc_awq_i8_gemm_on_rung(_ffi.ptr(a8), _ffi.ptr(a_s32), M, M, K, R, _ffi.ptr(pick(qw_rot)), _ffi.ptr(qz), _ffi.ptr(sc), G,
                                                      bf16, None, _ffi.ptr(y), _ffi.ptr(ws), nws, rung, st), 'llmc_awq_i8_gemm_on_rung')

            def w8a8():
                _ffi.check(L.llmc_i8_scaled_gemm(_ffi.ptr(a8), _ffi.ptr(a_s32), M, _ffi.ptr(pick(w8_rot)), _ffi.ptr(w_s), R, M, R, K, bf16, None,
                                                 _ffi.ptr(y), _ffi.ptr(ws), nws, st), 'llmc_i8_scaled_gemm')

            arms = {f'(a) awq_i8_linear_forward [{i8_route(M, K, R)}: the I8_LADDER]': lambda: awq_i8_linear_forward(x, qw, qz, sc, G, aq, None, None),
                    '(p) awq_linear_forward (W4A16, the parent)': lambda: awq_linear_forward(x, qw, qz, sc, G, None)}
            for name, r in I8_RUNGS.items():
                if name != 'stream' or M <= STREAM_MAX_M:
                    arms[f'(b) llmc_awq_i8_gemm [{name}]'] = lambda r=r: w4a8(r)
            arms['(c) i8_dequant + awq_linear_forward'] = lambda: awq_linear_forward(i8_dequant(a8, a_s, torch.bfloat16), qw, qz, sc, G, None)
            arms['(d) llmc_i8_scaled_gemm, int8 weight'] = w8a8
            ts = interleaved(arms, args.rounds)
            ops = 2.0 * M * K * R
            nbytes = float(K * R // 2 + (K // G) * R * 2 + (K // G) * R // 2 + M * K + 2 * M * R)
            say(f'tokens={M} K={K} R={R}  ({args.rounds} interleaved rounds of about 20 ms per arm; median, min, max per call)')
            tc = ts['(c) i8_dequant + awq_linear_forward']
            for k in arms:
                t, text = fmt(ts[k])
                tail = f'{ops / t / 1e15:.3f} POP/s' if M >= 1024 else f'{nbytes / t / 1e12:.2f} TB/s of {nbytes / 1e6:.1f} MB'
                if k.startswith('(b)'):
                    tail += ('  — beats (c), ranges apart' if ts[k][-1] < tc[0] else '  — loses to (c), ranges apart' if ts[k][0] > tc[-1]
                             else '  — ranges overlap with (c)')
                say(f'  {k:56s}{text} = {tail}')
        del qw_rot, w8_rot, mod
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
