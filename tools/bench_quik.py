"""The QUIK real-quant Linear (csrc/quik_gemm.hip) on the Llama-3-8B Linear shapes at 1, 16, 64, 512 and 4096 tokens, bf16, F = 256
outlier channels. Arms, timed in interleaved rounds inside one process with device events around batches of calls (median,
min..max: the run-to-run spread a difference has to exceed):

  (a) quik_act_split             alone, against the bytes it moves (2 K read, Ki + 2 Fp + 4 written per row)
  (b) llmc_quik_gemm             alone, each rung that takes the shape by name (the ladder's pick is marked)
  (c) llmc_i8_scaled_gemm        the parent's int8 GEMM at the same M, N and K = Ki on its own ladder: (b) - (c) is what the outlier
                                 phase costs
  (d) quik_linear_forward        split + GEMM, the whole forward of the deployed module
  (e) quik_linear_composed       the same product from the existing operators (gather, quantize, int8 GEMM, 16-bit linear, add)

(b) and (c) call the library's entry points on preallocated buffers. Below 1024 tokens they walk round copies of the weight that
together exceed the 256 MiB Infinity Cache, so every call reads its weight from HBM as a decode step does.

    python tools/bench_quik.py [--rounds 7] [--out profiles/quik_gemm.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bench_fp8_linear import fmt, interleaved

from llmc_amd import _ffi
from llmc_amd.compression.quantization import IntegerQuantizer
from llmc_amd.compression.quantization import quik_ops as QK
from llmc_amd.compression.quantization.module_utils import QuikRealQuantLinear
from llmc_amd.compression.quantization.quik import choose_indices

TOKENS = (4096, 512, 64, 16, 1)
ROTATE_BYTES = 320 << 20          # more than the Infinity Cache
SHAPES = ((4096, 4096), (1024, 4096), (14336, 4096), (4096, 14336))        # N x K: o / q, k / v, gate / up, down
F = 256
CFG = {'weight': dict(bit=8, symmetric=True, granularity='per_channel'), 'act': dict(bit=8, symmetric=True, granularity='per_token')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--shapes', type=int, default=len(SHAPES), help='only the first n shapes')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the rates are measured on an MI355X only'
    L = _ffi.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device='cuda').manual_seed(0)
    wq = IntegerQuantizer(8, True, 'per_channel')
    bf16 = _ffi.dt(torch.bfloat16)
    names = {v: k for k, v in QK.RUNGS.items()}
    st = _ffi.stream()
    for N, K in SHAPES[:args.shapes]:
        col_scale = torch.exp(0.5 * torch.randn(K, generator=g, device='cuda'))
        lin = torch.nn.Linear(K, N, bias=False, dtype=torch.bfloat16, device='cuda')
        lin.weight.data = (torch.randn(N, K, generator=g, device='cuda') * 0.02).to(torch.bfloat16)
        int_ids, fp_ids = choose_indices(col_scale, F)
        lin.register_buffer('buf_int_ids', int_ids)
        lin.register_buffer('buf_fp_ids', fp_ids)
        m = QuikRealQuantLinear.new(lin, lambda mod: wq.real_quant_weight_dynamic(mod.weight.data.index_select(1, mod.buf_int_ids)), CFG)
        Ki, Fp = m.weight.shape[1], m.weight_fp.shape[1]
        w_s32 = m.weight_scale.reshape(-1).contiguous()
        nrot = -(-ROTATE_BYTES // (N * (Ki + 2 * Fp)))
        w8_rot = [m.weight] + [m.weight.clone() for _ in range(nrot - 1)]
        wfp_rot = [m.weight_fp] + [m.weight_fp.clone() for _ in range(nrot - 1)]
        for M in TOKENS:
            x = (torch.randn(M, K, generator=g, device='cuda') * col_scale).to(torch.bfloat16)
            a8, a_s, a_fp = QK.quik_act_split(x, m.col_map, Ki, Fp)
            a_s32 = a_s.reshape(-1).contiguous()
            c = torch.empty(M, N, dtype=torch.bfloat16, device='cuda')
            ws = _ffi.workspace(max(L.llmc_i8_scaled_gemm_ws_bytes(M, N, Ki), 4), 'cuda')
            turn = [0]

            def pick():
                if M < 1024:
                    turn[0] = (turn[0] + 1) % nrot
                return turn[0]

            def quik(rung):
                i = pick()
                _ffi.check(L.llmc_quik_gemm_on_rung(_ffi.ptr(a8), _ffi.ptr(a_s32), _ffi.ptr(a_fp), _ffi.ptr(w8_rot[i]), _ffi.ptr(w_s32),
                                                    _ffi.ptr(wfp_rot[i]), M, N, Ki, Fp, bf16, bf16, None, _ffi.ptr(c), rung, st),
                           'llmc_quik_gemm_on_rung')

            def i8():
                _ffi.check(L.llmc_i8_scaled_gemm(_ffi.ptr(a8), _ffi.ptr(a_s32), M, _ffi.ptr(w8_rot[pick()]), _ffi.ptr(w_s32), N, M, N, Ki, bf16,
                                                 None, _ffi.ptr(c), _ffi.ptr(ws), ws.numel(), st), 'llmc_i8_scaled_gemm')

            picked = L.llmc_quik_gemm_rung(M, N)
            arms = {'(a) quik_act_split': lambda: QK.quik_act_split(x, m.col_map, Ki, Fp)}
            for r, name in sorted(names.items()):
                if name == 'tile128' or M <= QK.DECODE_MAX_M:
                    arms[f'(b) llmc_quik_gemm [{name}]' + (' <- the ladder' if r == picked else '')] = lambda r=r: quik(r)
            arms['(c) llmc_i8_scaled_gemm, K = Ki (its ladder)'] = i8
            arms['(d) quik_linear_forward'] = lambda: QK.quik_linear_forward(x, m)
            arms['(e) quik_linear_composed'] = lambda: QK.quik_linear_composed(x, m)
            ts = interleaved(arms, args.rounds)
            split_bytes = float(M * (2 * K + Ki + 2 * Fp + 4))
            say(f'tokens={M} N={N} K={K} (Ki={Ki}, Fp={Fp})  ({args.rounds} interleaved rounds of about 20 ms per arm; median, min, max per call)')
            for k in arms:
                t, text = fmt(ts[k])
                tail = f' = {split_bytes / t / 1e12:.2f} TB/s of the {split_bytes / 1e6:.2f} MB it moves' if k.startswith('(a)') else ''
                say(f'  {k:58s}{text}{tail}')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
