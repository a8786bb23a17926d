"""What gfx950's non-scaled fp8 matrix instructions keep of a small product beside a large one: through
llmc_fp8_scaled_gemm on each rung, A and B hold one product of 256 at k = 0 and one of 2^-j at k = pos; the line of a (rung, pos)
lists, per j, (result - 256) / 2^-j: 1.00 = the small product survived, 0.00 = it was cut off. pos 1 shares a lane's 8 operand
bytes with k = 0; pos 9 is the same lane's next instruction, pos 17 another lane of the same instruction, pos 40 / 100 further
instructions. Then the largest error over sum |a b| on random data, per rung, beside torch's fp32 product of the same codes.

    python tools/probes/fp8_window_probe.py > profiles/fp8_linear_window_probe.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np, torch
import fp8_linear_oracle as O
from llmc_amd.compression.quantization.fp8_linear_ops import fp8_scaled_gemm

def gpu(a): return torch.from_numpy(np.ascontiguousarray(a)).cuda()
one = gpu(np.ones(1, np.float32))
# window probe: big product 256 = 16 * 16 at k = 0, small product 2^-j at k = pos
for rung, M in (('decode', 16), ('tile128', 32)):
    for pos in (1, 9, 17, 40, 100):
        res = []
        for j in range(2, 19):
            # 2^-j = 2^-ja * 2^-jb with both factors e4m3 numbers (>= 2^-9)
            ja = j // 2; jb = j - ja
            a = np.zeros((M, 128)); b = np.zeros((16, 128))
            a[:, 0] = 16.0; b[:, 0] = 16.0
            a[:, pos] = 2.0 ** -ja; b[:, pos] = 2.0 ** -jb
            got = fp8_scaled_gemm(gpu(O.encode_exact(a)), one, gpu(O.encode_exact(b)), one, dtype=torch.float32, rung=rung).double().cpu().numpy()
            exact = 256.0 + 2.0 ** -j
            res.append((j, float(got[0, 0] - 256.0) / 2.0 ** -j))
        print(rung, 'pos', pos, ' '.join(f'{j}:{v:.2f}' for j, v in res), flush=True)
# error ratios on random data, every rung
for (M, N, K) in ((1, 16, 128), (17, 130, 384), (64, 130, 1152), (257, 256, 1152), (257, 256, 4096)):
    a, a_s, b, b_s = O.random_case(M, N, K, 3)
    E, P = O.gemm(a, a_s, b, b_s)
    for rung in ((None, 'decode', 'tile128') if M <= 64 else ('tile128',)):
        got = fp8_scaled_gemm(gpu(a), gpu(a_s), gpu(b), gpu(b_s), dtype=torch.float32, rung=rung).double().cpu().numpy()
        err = np.abs(got - E)
        T = ((gpu(a).view(torch.float8_e4m3fn).float() @ gpu(b).view(torch.float8_e4m3fn).float().T) * gpu(a_s)[:, None] * gpu(b_s)[None, :]).double().cpu().numpy()
        print((M, N, K), rung, 'max err/P = 2^%.2f' % np.log2((err / P).max()), 'max err/bound = %.3f' % (err / O.bound(E, P, K, 'f32')).max(),
              'torch fp32 err/P = 2^%.2f' % np.log2((np.abs(T - E) / P).max() + 1e-300), flush=True)
