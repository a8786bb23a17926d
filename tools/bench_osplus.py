"""Time the OS+ threshold search and its kernels on Llama-3-8B block shapes (N = 512 tokens: the shipped osplus_w_a.yml
calibrates 1 x 512; bf16, W8A8 per_channel / per_token), against a torch restatement of the reference loop on the same GPU.

    python tools/bench_osplus.py [--reps 20] [--ref-points 12] [--json out.json]

  * kernels: llmc_col_stats on the activations and on a weight, and the fused activation step (llmc_osplus_act_step) against
    the parent's two-kernel path (llmc_div_cols + the quantizer's dynamic fake-quant) at K = 4096 / 8192 / 14336 / 28672, with
    the GB/s each achieves against its byte count (col stats: one read of the tensor; activation step: one read of x, one
    write of q_x — the two-kernel path moves twice that and is held against the same count);
  * subset searches {q, k, v} (inspected module: the three projections side by side) and {gate, up} (inspected module: the
    gated MLP): ms per search and per grid point;
  * the torch restatement is osplus.py:104-171 as written: per grid point it re-quantizes every weight in place, divides and
    fake-quantizes the input with torch ops, runs the module and reloads the module's state dict from host copies
    (`load_state_dict(org_sd)`); it is timed over the first --ref-points thresholds only, per point.
Times are device events after a warm-up, median of --reps (kernels) or of 3 (searches)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402

N_TOK = 512


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
    return statistics.median(out)


def make_x(K, gen):
    c = torch.exp(0.5 * torch.randn(K, generator=gen, device='cuda'))
    c[torch.randperm(K, generator=gen, device='cuda')[:4]] *= 30
    return (torch.randn(1, N_TOK, K, generator=gen, device='cuda') * c).to(torch.bfloat16)


class Side(torch.nn.Module):
    """q / k / v side by side: the projections' outputs concatenated (no attention arithmetic in the timing)"""

    def __init__(self, K, outs):
        super().__init__()
        self.layers = torch.nn.ModuleList([torch.nn.Linear(K, r, bias=False) for r in outs])

    def forward(self, x):
        return torch.cat([l(x) for l in self.layers], dim=-1)

    def searched(self):
        return list(self.layers)


def torch_reference_points(layers, x, mod, wq_bits, n_points):
    """osplus.py:104-171 in torch ops (W8A8 sym per_channel / per_token), the first n_points thresholds"""
    qmax = 2 ** (wq_bits - 1) - 1
    org_sd = {k: v.cpu() for k, v in mod.state_dict().items()}
    org_out = mod(x)
    cmx, cmn = torch.amax(x, dim=(0, 1)), torch.amin(x, dim=(0, 1))
    amx, amn = max(x.max(), torch.tensor(0.0, dtype=x.dtype, device=x.device)), min(x.min(), torch.tensor(0.0, dtype=x.dtype, device=x.device))
    num = max(100, int(amx / 0.5))
    b1 = max(-amn.item(), amx.item())
    step = (b1 - 1.0) / num
    st, best = b1, None
    one = torch.tensor(1.0, dtype=x.dtype, device=x.device)

    def fq(t):
        s = t.abs().amax(dim=-1, keepdim=True).clamp(min=1e-5) / qmax
        return torch.clamp(torch.round(t / s), -qmax - 1, qmax) * s

    for _ in range(n_points):
        mxr, mnr = torch.tensor(st, dtype=x.dtype, device=x.device), torch.tensor(-st, dtype=x.dtype, device=x.device)
        cur = torch.max(torch.where(cmx > mxr, cmx / mxr, one), torch.where(cmn < mnr, cmn / mnr, one))
        for fc in layers:
            fc.weight.data.mul_(cur.view(1, -1))
            fc.weight.data = fq(fc.weight.data)
        out = mod(fq(x / cur.view(1, -1)))
        loss = (org_out - out).pow(2).sum(-1).mean()
        if best is None or best > loss:            # the reference's per-point host sync
            best = loss
        st -= step
        mod.load_state_dict(org_sd)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--ref-points', type=int, default=12)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_osplus: needs the GPU (no CPU fallback)')
    import llmc_amd.compression.quantization as Q
    from llmc_amd.compression.quantization import awq_ops, smooth_ops
    from smooth_osplus_cases import GatedMLP, OneBlockModel
    torch.set_grad_enabled(False)
    gen = torch.Generator(device='cuda').manual_seed(0)
    res = {'what': f'OS+ on Llama-3-8B block shapes, {N_TOK} tokens, bf16, W8A8 per_channel / per_token', 'kernels': {}, 'search': {}}

    # ---- kernels ---------------------------------------------------------------------------------------------------------
    for tag, shape in (('x_512x4096', (N_TOK, 4096)), ('x_512x14336', (N_TOK, 14336)), ('w_14336x4096', (14336, 4096))):
        t = torch.randn(*shape, generator=gen, device='cuda').to(torch.bfloat16)
        st = smooth_ops.ColStats(shape[1], t.device)
        ms = timed(lambda: st.update(t), args.reps)
        res['kernels']['col_stats_' + tag] = {'ms': ms, 'bytes': t.numel() * 2, 'GBps': t.numel() * 2 / ms / 1e6}
    aqs = {'int8_sym': Q.IntegerQuantizer(8, True, 'per_token'),
           'e4m3': Q.FloatQuantizer('e4m3', True, 'per_token', use_qtorch=True)}
    for K in (4096, 8192, 14336, 28672):
        x = make_x(K, gen)
        s = (1 + torch.rand(K, generator=gen, device='cuda')).to(torch.bfloat16)
        nbytes = 2 * x.numel() * 2 + K * 2
        for an, aq in aqs.items():
            fused = timed(lambda: smooth_ops.act_step(x, s, aq), args.reps)
            two = timed(lambda: aq.fake_quant_act_dynamic(awq_ops.div_cols(x, s)), args.reps)
            res['kernels'][f'act_step_{an}_K{K}'] = {'fused_ms': fused, 'two_kernel_ms': two, 'bytes': nbytes,
                                                     'fused_GBps': nbytes / fused / 1e6, 'two_kernel_GBps': nbytes / two / 1e6,
                                                     'fused_over_two': fused / two}

    # ---- subset searches ---------------------------------------------------------------------------------------------------
    qc = {'method': 'OsPlus', 'weight': dict(bit=8, symmetric=True, granularity='per_channel'),
          'act': dict(bit=8, symmetric=True, granularity='per_token')}
    subsets = {'qkv': Side(4096, (4096, 1024, 1024)), 'gate_up': GatedMLP(4096, 14336, False)}
    for tag, mod in subsets.items():
        for p in mod.parameters():
            p.data = torch.randn(p.shape, generator=torch.Generator().manual_seed(1)) * 0.02
        mod = mod.to(torch.bfloat16).cuda()
        x = make_x(4096, gen)
        algo = Q.OsPlus(OneBlockModel(mod, False), qc, None, None, {})
        ms = timed(lambda: algo.search_scale_shift_subset(mod.searched(), [x], mod, {}), 3)
        pts = len(algo.last_search['thresholds'])
        ref_ms = timed(lambda: torch_reference_points(mod.searched(), x, mod, 8, args.ref_points), 3)
        res['search'][tag] = {'grid_points': pts, 'ms_per_search': ms, 'ms_per_point': ms / pts,
                              'torch_restatement_ms_per_point': ref_ms / args.ref_points,
                              'torch_restatement_points_timed': args.ref_points,
                              'speedup_per_point': (ref_ms / args.ref_points) / (ms / pts),
                              'winner': int(algo.last_search['index'])}
        del mod, algo
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
