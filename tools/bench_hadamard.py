"""Time the Walsh-Hadamard kernel (llmc_hadamard) on the online-rotation shapes: down_proj's input of Llama-3-8B ([262144, 14336]
bf16, 28 * 512) and a 4096-wide power-of-two row ([262144, 4096] bf16), in the 16-bit mode (bf16 in, fp32 accumulation, bf16 out)
and the fp32_had mode of Rotater.rotate (cast to fp32, fp32 kernel, cast back), and the fp64 offline rotation at [14336, 4096].
Beside each, in the same process: a device copy of the same bytes (torch.Tensor.copy_) and the dense formulation of the
reference's CPU path (x @ M_n^T through torch.matmul). GB/s is algorithmic traffic: one read plus one write of the tensor in its
own dtype. Device events around ITER back-to-back calls, ROUNDS alternating rounds (profiles/hadamard_bench.txt is this output)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llmc_amd.compression.quantization.hadamard_utils import get_hadK, hadamard_transform, matmul_hadU_cuda  # noqa: E402
from llmc_amd.compression.quantization.module_utils import Rotater  # noqa: E402

ROUNDS = 3


def dense_M(n, dtype):
    hadK, K = get_hadK(n)
    m = n // K
    S = torch.ones(1, 1, dtype=torch.float64)
    while S.shape[0] < m:
        S = torch.cat([torch.cat([S, S], 1), torch.cat([S, -S], 1)], 0)
    M = S if K == 1 else torch.kron(hadK.double(), S)
    return M.to(dtype).cuda()


def time_arms(arms, iters):
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for name, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) * 1e-3 / iters)
    return times


def case(rows, n, dtype, iters):
    gen = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randn(rows, n, generator=gen, device='cuda', dtype=torch.float32).to(dtype)
    y = torch.empty_like(x)
    hadK, K = get_hadK(n)
    hk = None if hadK is None else hadK.cuda()
    M = dense_M(n, dtype)
    scale = 1.0 / float(torch.tensor(n).sqrt())
    nbytes = 2 * x.numel() * x.element_size()
    arms = {'llmc_hadamard': lambda: hadamard_transform(x, n, 1, hk, K, scale, out=y)}
    if dtype != torch.float64:
        rot = Rotater(True, False, True, K, hk, None)
        arms['Rotater.rotate fp32_had (cast + fp32 kernel + cast)'] = lambda: rot.rotate(x)
    arms['copy_ of the same bytes'] = lambda: y.copy_(x)
    arms['dense x @ M_n^T (torch.matmul)'] = lambda: torch.matmul(x, M.T, out=y)
    times = time_arms(arms, iters)
    ref = matmul_hadU_cuda(x[:64].double() if dtype == torch.float64 else x[:64].float(), hk, K)
    assert torch.isfinite(ref).all()
    print(f'# [{rows}, {n}] {str(dtype).replace("torch.", "")} (factor {K} x {n // K}), {nbytes / 1e9:.2f} GB read + written, '
          f'{iters} calls per measurement')
    copy_best = min(times['copy_ of the same bytes'])
    for name, ts in times.items():
        best = min(ts)
        print(f'{name:54s} {" ".join(f"{t * 1e3:9.3f}" for t in ts)} ms   {nbytes / best / 1e9:8.0f} GB/s   '
              f'{copy_best / best:5.2f} x copy rate')
    del x, y, M
    torch.cuda.empty_cache()


def main():
    print(f'# {torch.cuda.get_device_name(0)}; time per call in ms ({ROUNDS} alternating rounds), GB/s of one read + one write, '
          'rate relative to copy_')
    case(262144, 14336, torch.bfloat16, 5)
    case(262144, 4096, torch.bfloat16, 10)
    case(14336, 4096, torch.float64, 20)


if __name__ == '__main__':
    main()
