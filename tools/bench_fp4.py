"""Time the single-pass narrow-format fake-quant (llmc_fpx_quant: e2m1, qtorch and ocp rounding, plus the MX form) against the
two-pass FP8 analogue (FloatQuantizer e4m3 per_group: llmc_minmax_qparams + k_fp8_cast) on one 14336 x 4096 bf16 weight,
per_group 128. Three alternating rounds of each arm in one process; device events around ITER back-to-back calls.
Prints us per call and the HBM bytes each arm has to move over 8 TB/s (profiles/fp4_quant.txt is this output)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llmc_amd.compression.quantization import FloatQuantizer  # noqa: E402

R, K, G, ITER, ROUNDS = 14336, 4096, 128, 200, 3
PEAK = 8e12


def main():
    gen = torch.Generator(device='cuda').manual_seed(0)
    w = (torch.randn(R, K, generator=gen, device='cuda') * 0.02).to(torch.bfloat16)
    cols = (0.5 + 1.5 * torch.rand(K, generator=gen, device='cuda')).to(torch.bfloat16)
    n = R * K
    arms = {}

    def arm(name, fn, bytes_moved):
        arms[name] = (fn, bytes_moved, [])

    f8 = FloatQuantizer('e4m3', True, 'per_group', group_size=G, use_qtorch=True)
    q4 = FloatQuantizer('e2m1', True, 'per_group', group_size=G, use_qtorch=True)
    o4 = FloatQuantizer('e2m1', True, 'per_group', group_size=G, use_qtorch=True, float_semantics='ocp')
    mx = FloatQuantizer('e2m1', True, 'per_group', group_size=32, use_qtorch=True, float_semantics='ocp', scale_format='e8m0')
    sc = n // G * 2
    arm('e4m3 qtorch fake (parent: minmax pass + cast pass)', lambda: f8.fake_quant_weight_dynamic(w), 3 * n * 2 + 2 * sc)
    arm('e2m1 qtorch fake (one pass)', lambda: q4.fake_quant_weight_dynamic(w), 2 * n * 2 + sc)
    arm('e2m1 ocp fake (one pass)', lambda: o4.fake_quant_weight_dynamic(w), 2 * n * 2 + sc)
    arm('e2m1 ocp e8m0 g32 fake (one pass)', lambda: mx.fake_quant_weight_dynamic(w), 2 * n * 2 + n // 32)
    arm('e2m1 qtorch codes (one pass)', lambda: q4._run(q4.reshape_tensor(w), False), n * 2 + n + sc)
    arm('e2m1 qtorch fake with cols (one pass)', lambda: q4._run(q4.reshape_tensor(w), True, cols=cols), 2 * n * 2 + sc)
    for fn, _, _ in arms.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, (fn, _, times) in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(ITER):
                fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / ITER)
    print(f'# {R} x {K} bf16, per_group {G}; us per call (device events around {ITER} calls), {ROUNDS} alternating rounds')
    print(f'# {"arm":58s} {"rounds (us)":28s} {"bytes":>10s} {"bytes / 8 TB/s (us)":>20s} {"best / bound":>13s}')
    for name, (_, nbytes, times) in arms.items():
        bound = nbytes / PEAK * 1e6
        print(f'{name:60s} {" ".join(f"{t:8.1f}" for t in times):28s} {nbytes:10d} {bound:20.1f} {min(times) / bound:13.2f}')


if __name__ == '__main__':
    main()
