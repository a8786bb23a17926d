"""Time the column-wise min/max quantizer (llmc_quant_dynamic_cols, csrc/quant_cols.hip) against the composition it replaces
(quant_cols_ops.fake_quant_cols_composed: contiguous transposed copy -> llmc_quant_dynamic -> transposed back and made
contiguous, which is what the parent's fake_quant_weight_dynamic(w, {'dim': 'ic'}) plus the GEMM's .contiguous() cost per forward
of an 'ic' layer), on the same GPU, and AdaDim.search_dim_subset against a plain-torch restatement of the reference's loop.

    python tools/bench_quant_cols.py [--reps 9] [--txt profiles/quant_cols.txt] [--json out.json]

  * weights, all bf16: 4096 x 4096, 1024 x 4096, 14336 x 4096, 4096 x 14336 (R x K; groups run down the R rows of a column);
  * quantizers: int8 symmetric per_channel (g = R, the slab path) and int4 asymmetric per_group g = 128 (the tile path);
  * a third column times the parent's quantizer route alone (HOST_OPTIONS quant_cols = 0: it returns a transposed view and
    leaves the last copy to the GEMM), so the table also shows the kernel against the composition without that copy.
Times are device events around one call, 2 warm-up calls per side, the sides alternating inside every repetition, median of
--reps (>= 5) with min..max. GB/s is on the algorithmic bytes 2 * R * K * sizeof(dt) for every side. The outputs are compared
bit for bit at every timed shape.
  * search_dim_subset on a q / k / v-shaped subset (three 4096 x 4096 layers, 8 samples of 2048 tokens) against the reference's
    loop in torch ops (F.linear twice per sample and axis, .item() per sample) on the same quantized weights.
  * the losses of the planted golden layers (tests/golden/adadim.npz: the reference's CPU fp16 GEMM) against ours."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

WARMUP = 2
SHAPES = ((4096, 4096), (1024, 4096), (14336, 4096), (4096, 14336))
QUANTIZERS = (('int8_sym_per_channel', dict(bit=8, symmetric=True, granularity='per_channel')),
              ('int4_asym_g128', dict(bit=4, symmetric=False, granularity='per_group', group_size=128)))


def timed(fns, reps):
    for _ in range(WARMUP):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    acc = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, acc):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            t.append(a.elapsed_time(b))
    return [(statistics.median(t), min(t), max(t)) for t in acc]


def bench_kernel(reps):
    from llmc_amd import _ffi
    from llmc_amd.compression.quantization import IntegerQuantizer, quant_cols_ops
    gen = torch.Generator(device='cuda').manual_seed(0)
    rows = []
    for R, K in SHAPES:
        w = (torch.randn(R, K, generator=gen, device='cuda') * 0.02)
        w[:, ::97] *= 20
        w = w.to(torch.bfloat16)
        for tag, cfg in QUANTIZERS:
            q = IntegerQuantizer(**cfg)
            g = q._cols_group(w)
            a = (w, g, q.sym, q.round_zp, float(q.qmin), float(q.qmax))

            def old_route():
                with _ffi.option(quant_cols=0):
                    return q.fake_quant_weight_dynamic(w, {'dim': 'ic'})
            kern = quant_cols_ops.fake_quant_cols(*a)
            same = torch.equal(kern.view(torch.int16), quant_cols_ops.fake_quant_cols_composed(*a).view(torch.int16)) and \
                torch.equal(kern.view(torch.int16), old_route().contiguous().view(torch.int16))
            (k, c, o) = timed([lambda: quant_cols_ops.fake_quant_cols(*a), lambda: quant_cols_ops.fake_quant_cols_composed(*a),
                               old_route], reps)
            nbytes = 2 * w.numel() * w.element_size()
            rows.append(dict(case=f'{R}x{K}_{tag}', path=quant_cols_ops.path(w, g), bytes=nbytes, kernel_ms=k, composed_ms=c,
                             old_route_view_ms=o, kernel_over_composed=k[0] / c[0], kernel_over_old_route=k[0] / o[0],
                             ranges_overlap=bool(k[2] >= c[1] and c[2] >= k[1]), same_bits=bool(same)))
            del kern
    return rows


def bench_search(reps):
    import torch.nn.functional as F
    import llmc_amd.compression.quantization as Q
    gen = torch.Generator(device='cuda').manual_seed(1)
    n, T, H = 8, 2048, 4096
    a = object.__new__(Q.AdaDim)
    a.n_samples, a.dim_losses = n, {}
    a.wquantizer = Q.IntegerQuantizer(8, True, 'per_channel')
    layers = {}
    for name in ('q_proj', 'k_proj', 'v_proj'):
        m = torch.nn.Linear(H, H, bias=False)
        m.weight.data = (torch.randn(H, H, generator=gen, device='cuda') * 0.02).to(torch.bfloat16)
        layers[name] = m
    c = torch.exp(0.5 * torch.randn(H, generator=gen, device='cuda'))
    xs = [(torch.randn(1, T, H, generator=gen, device='cuda') * c).to(torch.bfloat16) for _ in range(n)]

    def ours():
        a.search_dim_subset(layers, list(xs))
        return {k: int(m.buf_qdim) for k, m in layers.items()}

    def restated():
        out = {}
        for name, m in layers.items():
            loss = {}
            for dim in ('oc', 'ic'):
                wq = a.wquantizer.fake_quant_weight_dynamic(m.weight.data.clone(), {'dim': dim})
                lm = 0
                for x in xs:
                    lm += x.shape[0] * 1.0 / n * (F.linear(x, m.weight.data) - F.linear(x, wq)).float().pow(2).mean().item()
                loss[dim] = lm
            out[name] = 0 if loss['ic'] < loss['oc'] else 1
        return out
    same = ours() == restated()
    (o, r) = timed([ours, restated], reps)
    return dict(case=f'search_dim_subset qkv {H}x{H} bf16, {n} samples x {T} tokens', ours_ms=o, restated_ms=r,
                ours_over_restated=o[0] / r[0], same_decisions=bool(same))


def golden_losses():
    import llmc_amd.compression.quantization as Q
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'adadim.npz'), allow_pickle=False)
    R, K, T, n = (int(v) for v in g['shape'])
    rows = []
    for case in (str(c) for c in g['names']):
        cfg = json.loads(str(g[f'{case}/cfg']))
        a = object.__new__(Q.AdaDim)
        a.n_samples, a.dim_losses = n, {}
        a.wquantizer = Q.IntegerQuantizer(cfg['bit'], cfg['symmetric'], cfg['granularity'],
                                          **({'group_size': cfg['group_size']} if 'group_size' in cfg else {}))
        layers = {}
        for kind in (str(k) for k in g['layers']):
            w = torch.from_numpy(g[f'{case}/{kind}/w_bits'].view(np.int16).copy()).view(torch.float16).cuda()
            m = torch.nn.Linear(K, R, bias=False)
            m.weight.data = w
            layers[kind] = m
        xs = [torch.from_numpy(g[f'{case}/x{i}_bits'].view(np.int16).copy()).view(torch.float16).reshape(1, T, K) for i in range(n)]
        a.search_dim_subset(layers, xs)
        for kind, m in layers.items():
            ref = [float(v) for v in g[f'{case}/{kind}/losses']]
            ours = a.dim_losses[kind]
            rows.append(dict(case=f'{case}/{kind}', ours=ours, reference=ref, rel=[abs(o - r) / r for o, r in zip(ours, ref)],
                             qdim=int(m.buf_qdim), ref_qdim=int(g[f'{case}/{kind}/qdim'])))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--txt', default=None)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit('bench_quant_cols: at least 5 repetitions')
    if not torch.cuda.is_available():
        raise SystemExit('bench_quant_cols: needs the GPU (no CPU fallback)')
    torch.set_grad_enabled(False)
    rows = bench_kernel(args.reps)
    search = bench_search(max(5, args.reps // 2))
    gold = golden_losses()

    def f(t):
        return f'{t[0]:8.4f} ({t[1]:.4f}..{t[2]:.4f})'
    lines = [f'column-wise quantizer (dim = ic), bf16; device events, {WARMUP} warm-ups, median (min..max) of {args.reps} alternating '
             'repetitions; GB/s on 2 * R * K * 2 bytes; composed = transposed copy + row kernel + copy back; old route = the '
             'parent\'s quantizer call alone (returns a view)',
             f'{"case R x K":40s} {"path":>4s} {"kernel ms":>27s} {"GB/s":>6s} {"composed ms":>27s} {"GB/s":>6s} '
             f'{"old route (view) ms":>27s} {"k/composed":>10s} {"k/old":>6s} {"overlap":>7s} {"same bits":>9s}']
    for r in rows:
        lines.append(f"{r['case']:40s} {r['path']:4d} {f(r['kernel_ms']):>27s} {r['bytes'] / r['kernel_ms'][0] / 1e6:6.0f} "
                     f"{f(r['composed_ms']):>27s} {r['bytes'] / r['composed_ms'][0] / 1e6:6.0f} {f(r['old_route_view_ms']):>27s} "
                     f"{r['kernel_over_composed']:10.3f} {r['kernel_over_old_route']:6.3f} {str(r['ranges_overlap']):>7s} "
                     f"{str(r['same_bits']):>9s}")
    lines += ['', f"{search['case']}: ours {f(search['ours_ms'])} ms, torch restatement {f(search['restated_ms'])} ms, "
              f"ours / restated {search['ours_over_restated']:.3f}, same decisions {search['same_decisions']}", '',
              'losses on the planted golden layers: ours (HIP GEMM, fp32 accumulation) against the reference\'s (CPU fp16 GEMM); '
              'not asserted anywhere, the decisions are',
              f'{"case":34s} {"ours oc":>13s} {"ours ic":>13s} {"ref oc":>13s} {"ref ic":>13s} {"rel oc":>9s} {"rel ic":>9s} {"qdim":>5s} {"ref":>4s}']
    for r in gold:
        lines.append(f"{r['case']:34s} {r['ours'][0]:13.6g} {r['ours'][1]:13.6g} {r['reference'][0]:13.6g} {r['reference'][1]:13.6g} "
                     f"{r['rel'][0]:9.2e} {r['rel'][1]:9.2e} {r['qdim']:5d} {r['ref_qdim']:4d}")
    text = '\n'.join(lines)
    print(text)
    if args.txt:
        os.makedirs(os.path.dirname(os.path.abspath(args.txt)), exist_ok=True)
        with open(args.txt, 'w') as fh:
            fh.write(text + '\n')
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(dict(kernel=rows, search=search, golden=gold), fh, indent=1)
    if not all(r['same_bits'] for r in rows):
        raise SystemExit('bench_quant_cols: the kernel and the composition disagree')


if __name__ == '__main__':
    main()
