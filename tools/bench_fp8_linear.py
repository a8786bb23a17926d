"""The plain FP8 Linear (csrc/fp8_linear.hip) on the Llama-3-8B Linear shapes at 4096, 1024, 256, 64, 16 and 1 tokens, bf16 activations and
outputs. Arms, timed in interleaved rounds inside one process with device events around batches of calls (median, min..max):

  (a) fp8_linear_forward          activation quantization + llmc_fp8_scaled_gemm, the whole forward of the deployed module
  (b) llmc_fp8_scaled_gemm        alone, on the rung the library's ladder picks — and on the other rung where it takes the shape,
                                  by name: the ladder's threshold (csrc/fp8_linear.hip, FL_LADDER) is set from these rows
  (c) llmc_fp8_block_gemm         the parent's FP8 GEMM on the same codes with 128-block scales (a timing arm: other numbers)
  (d) de-quantize + hip_linear    the only route from the stored weight to an output before this kernel existed
  (e) hip_linear                  on the bf16 weight

(b) and (c) call the library's entry points on preallocated buffers, so that at 64, 16 and 1 tokens the rows show the kernels and
not tensor allocation; a row whose time is a few microseconds is still bounded below by the launch rate of one stream.
Below 1024 tokens (b) and (c) walk round copies of the weight that together exceed the 256 MiB Infinity Cache, so every call
reads its weight from HBM as a decode step does; "(b) cache-warm" re-reads one copy, the figure a loop over one layer would show.
Every batch is sized to about 20 ms from a first timing of its arm.
Random operands (Gaussian weight, Gaussian activations with per-channel spread), never zeros.

Peaks (MI355X, dense): ~2.5 PF for the non-scaled fp8 matrix instructions (b) issues (the bf16 rate), ~5 PF for the block-scaled
form (c) issues, 8 TB/s HBM.

    python tools/bench_fp8_linear.py [--rounds 7] [--out profiles/fp8_linear.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from llmc_amd import _ffi
from llmc_amd.compression.quantization import FloatQuantizer
from llmc_amd.compression.quantization.fp8_linear_ops import RUNGS, fp8_act_quant, fp8_dequant, fp8_linear_forward
from llmc_amd.compression.quantization.module_utils import hip_linear

TOKENS = (4096, 1024, 256, 64, 16, 1)
ROTATE_BYTES = 320 << 20          # more than the Infinity Cache
SHAPES = ((4096, 4096), (1024, 4096), (14336, 4096), (4096, 14336))        # N x K: o / q, k / v, gate / up, down
ACT = dict(bit='e4m3', symmetric=True, granularity='per_token', use_qtorch=True, quant_type='float-quant')


def batch_time(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls


def interleaved(arms, rounds):
    """arms: name -> fn. Every round times every arm once (a batch of about 20 ms), in turn. name -> sorted per-call times."""
    calls = {}
    for k, fn in arms.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[k] = max(10, min(4000, int(0.02 / batch_time(fn, 10))))
    ts = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ts[k].append(batch_time(fn, calls[k]))
    return {k: sorted(v) for k, v in ts.items()}


def fmt(ts):
    med = ts[len(ts) // 2]
    return med, f'{med * 1e6:9.1f} us (min {ts[0] * 1e6:.1f}, max {ts[-1] * 1e6:.1f})'


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
    wq = FloatQuantizer('e4m3', True, 'per_channel', use_qtorch=True)
    aq = FloatQuantizer(**{k: v for k, v in ACT.items() if k != 'quant_type'})
    bf16 = _ffi.dt(torch.bfloat16)
    names = {v: k for k, v in RUNGS.items()}
    for N, K in SHAPES:
        w = (torch.randn(N, K, generator=g, device='cuda') * 0.02).to(torch.bfloat16)
        w8, w_s, _ = wq.real_quant_weight_dynamic(w)
        w_s32 = w_s.reshape(-1).float().contiguous()
        b_s128 = torch.full((N // 128, K // 128), float(w_s32.mean()), device='cuda')
        nrot = -(-ROTATE_BYTES // (N * K))
        w8_rot = [w8] + [w8.clone() for _ in range(nrot - 1)]
        for M in TOKENS:
            x = (torch.randn(M, K, generator=g, device='cuda') * torch.exp(0.5 * torch.randn(K, generator=g, device='cuda'))).to(torch.bfloat16)
            a8, a_s = fp8_act_quant(x, aq)
            a_s32 = a_s.reshape(-1).contiguous()
            a_s128 = a_s32.reshape(M, 1).expand(M, K // 128).contiguous()
            c = torch.empty(M, N, dtype=torch.bfloat16, device='cuda')
            st = _ffi.stream()

            turn = [0]

            def weight(rotate):
                if not rotate or M >= 1024:
                    return w8
                turn[0] = (turn[0] + 1) % nrot
                return w8_rot[turn[0]]

            def scaled(rung=-1, rotate=True):
                _ffi.check(L.llmc_fp8_scaled_gemm_on_rung(_ffi.ptr(a8), _ffi.ptr(a_s32), M, _ffi.ptr(weight(rotate)), _ffi.ptr(w_s32), N, M, N, K,
                                                          bf16, None, _ffi.ptr(c), rung, st), 'llmc_fp8_scaled_gemm_on_rung')

            def block():
                _ffi.check(L.llmc_fp8_block_gemm(_ffi.ptr(a8), _ffi.ptr(a_s128), _ffi.ptr(weight(True)), _ffi.ptr(b_s128), M, N, K, bf16, None,
                                                 _ffi.ptr(c), st), 'llmc_fp8_block_gemm')

            picked = L.llmc_fp8_scaled_gemm_rung(M, N)
            arms = {'(a) fp8_linear_forward': lambda: fp8_linear_forward(x, w8, w_s, aq, None, None),
                    f'(b) llmc_fp8_scaled_gemm [{names[picked]}: the ladder]': scaled}
            for r, name in sorted(names.items()):
                if r != picked and (name != 'decode' or M <= 64):
                    arms[f'    llmc_fp8_scaled_gemm [{name}, by name]'] = lambda r=r: scaled(r)
            if M < 1024:
                arms['    (b) cache-warm: one copy of the weight re-read'] = lambda: scaled(-1, False)
            arms['(c) llmc_fp8_block_gemm (parent)'] = block
            arms['(d) de-quantize + hip_linear'] = lambda: hip_linear(x, fp8_dequant(w8, w_s, torch.bfloat16), None)
            arms['(e) hip_linear, bf16 weight'] = lambda: hip_linear(x, w, None)
            ts = interleaved(arms, args.rounds)
            fl, wbytes = 2.0 * M * N * K, float(N * K + M * K + 2 * M * N)
            say(f'tokens={M} N={N} K={K}  ({args.rounds} interleaved rounds of about 20 ms per arm; median, min, max per call)')
            tb = None
            for k in arms:
                t, text = fmt(ts[k])
                if k.startswith('(b)'):
                    tb = ts[k]
                tail = f'{fl / t / 1e15:.3f} PFLOP/s' if M >= 1024 else f'{wbytes / t / 1e12:.2f} TB/s of the {wbytes / 1e6:.1f} MB an FP8 GEMM moves'
                say(f'  {k:58s}{text} = {tail}')
            tc = ts['(c) llmc_fp8_block_gemm (parent)']
            verdict = ('(b) faster, ranges apart' if tb[-1] < tc[0] else '(b) slower, ranges apart' if tb[0] > tc[-1] else 'ranges overlap')
            say(f'  (b) / (c) medians: {tb[len(tb) // 2] / tc[len(tc) // 2]:.2f} — {verdict}')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
