"""Time HQQ (the shipped hqq_w_only config: 4-bit asym, per_group 128, axis 0, lp_norm 0.7, beta 10, iters 20) over the
seven Linears of one synthetic Llama-3-8B block, against a torch restatement of the reference loop on the same GPU.

    python tools/bench_hqq.py [--reps 10] [--json out.json]

Per layer: one llmc_hqq_optimize chain (HQQ.solve_layer). Times are device events around the whole block, after a
warm-up, median of --reps. The torch restatement is the reference's optimize_weights_proximal (hqq.py:36-60) with its
per-iteration host sync, on W.float().T reshaped like get_tensor_qparams does."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

LAYERS = [('q_proj', 4096, 4096), ('k_proj', 1024, 4096), ('v_proj', 1024, 4096), ('o_proj', 4096, 4096),
          ('gate_proj', 14336, 4096), ('up_proj', 14336, 4096), ('down_proj', 4096, 14336)]
FP32_PEAK = 157.3e12          # MI355X dense FP32 vector rate (an FMA counts 2)

# VALU instructions per element and iteration on the path the benchmark takes (k_hqq_chunk, fast division, shrink guard
# below tau, llmc_amd/csrc/hqq.hip hqq_term SH_GUARD + the ATen-order sum), as issued: v_add_f64 counted as 2 slots
# (fp64 runs at half the fp32 rate). Kept here so the count travels with the number it divides.
OPS = {'copy into the ordering barrier': 1, 'x * inv': 1, '+ z': 1, 'rint': 1, 'clamp (max, min)': 2, 'q - z': 1,
       'div tail (mul, 4 fma)': 5, 'x - r': 1, 'cvt |d| to f64': 1, 'f64 add (2 slots)': 2, '|d| < tau': 1,
       'q - x * inv': 1, 'group sum': 1}
OPS_PER_ELEM_ITER = sum(OPS.values())


def torch_reference(W, qmin, qmax, iters=20, beta=10, p=0.7, g=128):
    t = W.float().T.reshape(-1, g)
    mn, mx = t.amin(dim=-1, keepdim=True), t.amax(dim=-1, keepdim=True)
    scales = (mx - mn).clamp(min=1e-5) / (qmax - qmin)
    zeros = qmin - (mn / scales)
    best = 1e4
    scales = 1 / scales
    for _ in range(iters):
        W_q = torch.round(t * scales + zeros).clamp(qmin, qmax)
        W_r = (W_q - zeros) / scales
        x = t - W_r
        W_e = torch.sign(x) * torch.nn.functional.relu(torch.abs(x) - (1.0 / beta) * torch.pow(torch.abs(x), p - 1))
        zeros = torch.mean(W_q - (t - W_e) * scales, axis=-1, keepdim=True)
        err = float(torch.abs(t - W_r).mean())
        if err < best:
            best = err
        else:
            break
    return 1 / scales, zeros


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--ref-reps', type=int, default=3)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_hqq: needs the GPU (no CPU fallback)')
    from llmc_amd.compression.quantization import IntegerQuantizer
    wq = IntegerQuantizer(4, False, 'per_group', group_size=128, round_zp=False)
    gen = torch.Generator(device='cuda').manual_seed(0)
    Ws = {}
    for n, R, K in LAYERS:
        w = torch.randn(R, K, generator=gen, device='cuda') * 0.02
        m = torch.rand(R, K, generator=gen, device='cuda') < 1e-3
        Ws[n] = torch.where(m, w * 20, w).to(torch.bfloat16)

    Ts = {}

    def block():
        for n, _, _ in LAYERS:
            Ts[n] = wq.hqq_solve(Ws[n], axis=0, lp_norm=0.7, beta=10, iters=20)[2]

    per_layer = {}
    for n, _, _ in LAYERS:
        per_layer[n] = timed(lambda n=n: wq.hqq_solve(Ws[n], axis=0, lp_norm=0.7, beta=10, iters=20), args.reps)[0]
    med, all_ms = timed(block, args.reps)
    Ts = {n: int(t.item()) for n, t in Ts.items()}
    elems_iters = sum(R * K * (Ts[n] + 1) for n, R, K in LAYERS)
    share = OPS_PER_ELEM_ITER * elems_iters / (med * 1e-3) / (FP32_PEAK / 2)
    qmin, qmax = torch.tensor(0.0, device='cuda'), torch.tensor(15.0, device='cuda')
    ref_ms, _ = timed(lambda: [torch_reference(Ws[n], qmin, qmax) for n, _, _ in LAYERS], args.ref_reps)
    res = {'what': 'HQQ shipped config over one Llama-3-8B block (7 Linears, bf16)', 'ms_per_block': med,
           'ms_all': all_ms, 'ms_per_layer': per_layer, 'T': Ts, 'valu_ops_per_element_iteration': OPS_PER_ELEM_ITER,
           'share_of_fp32_vector_peak': share, 'torch_restatement_ms_per_block': ref_ms,
           'speedup_vs_torch': ref_ms / med}
    print(json.dumps(res))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
