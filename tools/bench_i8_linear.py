"""The W8A8 integer Linear (csrc/i8_linear.hip) on the Llama-3-8B Linear shapes at 1, 4, 16, 32, 64, 512 and 4096 tokens, bf16 activations
and outputs. Arms, timed in interleaved rounds inside one process with device events around batches of calls (median, min..max:
the run-to-run spread a difference has to exceed):

  (a) i8_linear_forward           activation quantization + llmc_i8_scaled_gemm, the whole forward of the deployed module
  (b) llmc_i8_scaled_gemm         alone, each rung that takes the shape by name (the ladder's pick is marked); decode_split also
                                  with S = 2, 4, 8, 16 K slices (option i8_split_slices) beside the library's own S: the ladder
                                  (csrc/i8_linear.hip, I8_LADDER) and the slice rule are set from these rows
  (c) llmc_fp8_scaled_gemm        the FP8 GEMM of the same build at the same shape: the same bytes and the same instruction rate
  (d) de-quantize + hip_linear    what a user had to do before: both operands back to bf16, then the 16-bit GEMM

(b) and (c) call the library's entry points on preallocated buffers. Below 1024 tokens they walk round copies of the weight that
together exceed the 256 MiB Infinity Cache, so every call reads its weight from HBM as a decode step does. Every batch is sized
to about 20 ms from a first timing of its arm. Random codes over the full range, never zeros.

    python tools/bench_i8_linear.py [--rounds 7] [--out profiles/i8_linear.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bench_fp8_linear import fmt, interleaved

from llmc_amd import _ffi
from llmc_amd.compression.quantization import IntegerQuantizer
from llmc_amd.compression.quantization.i8_linear_ops import DECODE_MAX_M, RUNGS, i8_act_quant, i8_dequant, i8_linear_forward
from llmc_amd.compression.quantization.module_utils import hip_linear

TOKENS = (4096, 512, 64, 32, 16, 4, 1)
ROTATE_BYTES = 320 << 20          # more than the Infinity Cache
SHAPES = ((4096, 4096), (1024, 4096), (14336, 4096), (4096, 14336))        # N x K: o / q, k / v, gate / up, down
SLICES = (2, 4, 8, 16)
ACT = dict(bit=8, symmetric=True, granularity='per_token')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the rates are measured on an MI355X only'
    L = _ffi.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device='cuda').manual_seed(0)
    wq, aq = IntegerQuantizer(8, True, 'per_channel'), IntegerQuantizer(**ACT)
    bf16 = _ffi.dt(torch.bfloat16)
    names = {v: k for k, v in RUNGS.items()}
    st = _ffi.stream()
    for N, K in SHAPES:
        w = (torch.randn(N, K, generator=g, device='cuda') * 0.02).to(torch.bfloat16)
        w8, w_s, _ = wq.real_quant_weight_dynamic(w)
        w_s32 = w_s.reshape(-1).float().contiguous()
        nrot = -(-ROTATE_BYTES // (N * K))
        w8_rot = [w8] + [w8.clone() for _ in range(nrot - 1)]
        f8_rot = [t.view(torch.uint8) for t in w8_rot]            # any bytes are e4m3 codes: (c) is a timing arm
        for M in TOKENS:
            x = (torch.randn(M, K, generator=g, device='cuda') * torch.exp(0.5 * torch.randn(K, generator=g, device='cuda'))).to(torch.bfloat16)
            a8, a_s = i8_act_quant(x, aq)
            a_s32 = a_s.reshape(-1).contiguous()
            c = torch.empty(M, N, dtype=torch.bfloat16, device='cuda')
            with _ffi.option(i8_split_slices=max(SLICES)):
                ws = _ffi.workspace(max(L.llmc_i8_scaled_gemm_ws_bytes(M, N, K), 4), 'cuda')
            turn = [0]

            def pick(rot):
                if M >= 1024:
                    return rot[0]
                turn[0] = (turn[0] + 1) % nrot
                return rot[turn[0]]

            def i8(rung, slices=0):        # every i8 arm sets the option (one host call), so the arms stay comparable
                L.llmc_hip_set_option(b'i8_split_slices', slices)
                _ffi.check(L.llmc_i8_scaled_gemm_on_rung(_ffi.ptr(a8), _ffi.ptr(a_s32), M, _ffi.ptr(pick(w8_rot)), _ffi.ptr(w_s32), N, M, N, K,
                                                         bf16, None, _ffi.ptr(c), _ffi.ptr(ws), ws.numel(), rung, st), 'llmc_i8_scaled_gemm_on_rung')

            def f8():
                _ffi.check(L.llmc_fp8_scaled_gemm(_ffi.ptr(a8), _ffi.ptr(a_s32), M, _ffi.ptr(pick(f8_rot)), _ffi.ptr(w_s32), N, M, N, K, bf16, None,
                                                  _ffi.ptr(c), st), 'llmc_fp8_scaled_gemm')

            picked = L.llmc_i8_scaled_gemm_rung(M, N, K)
            arms = {'(a) i8_linear_forward': lambda: i8_linear_forward(x, w8, w_s, aq, None, None)}
            for r, name in sorted(names.items()):
                if name == 'tile128' or M <= DECODE_MAX_M:
                    arms[f'(b) llmc_i8_scaled_gemm [{name}]' + (' <- the ladder' if r == picked else '')] = lambda r=r: i8(r)
            if M <= DECODE_MAX_M:
                for s in SLICES:
                    arms[f'    decode_split, S = {s}'] = lambda s=s: i8(RUNGS['decode_split'], s)
            arms['(c) llmc_fp8_scaled_gemm (the ladder)'] = f8
            arms['(d) de-quantize both + hip_linear'] = lambda: hip_linear(i8_dequant(a8, a_s, torch.bfloat16), i8_dequant(w8, w_s, torch.bfloat16), None)
            ts = interleaved(arms, args.rounds)
            fl, wbytes = 2.0 * M * N * K, float(N * K + M * K + 2 * M * N)
            say(f'tokens={M} N={N} K={K}  ({args.rounds} interleaved rounds of about 20 ms per arm; median, min, max per call)')
            for k in arms:
                t, text = fmt(ts[k])
                tail = f'{fl / t / 1e15:.3f} POP/s' if M >= 512 else f'{wbytes / t / 1e12:.2f} TB/s of the {wbytes / 1e6:.1f} MB an 8-bit GEMM moves'
                say(f'  {k:58s}{text} = {tail}')
            _ffi.reset_options()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
