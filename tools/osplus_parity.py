"""How far apart two correct evaluations of the OS+ loss curve lie: the reference itself on this GPU against its own CPU
golden (tests/golden/smooth_osplus.npz), and llmc_amd against the same golden, on the same inputs.

    python tools/osplus_parity.py [--out profiles/osplus_parity.txt]

Arm `ref_gpu` imports the plain copy of the reference (oracle/_ref/plain, made by __graft_entry__.build(); with the import
shims of oracle/_shims) and runs OsPlus.search_scale_shift_subset unmodified on cuda, bound onto a SimpleNamespace as
tools/make_golden_smooth_osplus.py does on the CPU; the curve is read with forward hooks on the inspected module. FloatQuantizer
cases are left out of that arm (qtorch is not installed; the restated float_quantize is a CPU routine). Arm `ours` is
llmc_amd's OsPlus. Per case and arm: the largest relative deviation of a grid point's loss from the golden's, and the winner.
tests/test_smooth_osplus_gpu.py allows our curve twice the reference's own spread (a single sample). Test infrastructure."""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import smooth_osplus_cases as C  # noqa: E402

PLAIN = os.path.join(ROOT, 'oracle', '_ref', 'plain')


def curve_dev(loss, gold):
    loss, gold = np.asarray(loss, np.float64), np.asarray(gold, np.float64)
    return float(np.max(np.abs(loss - gold) / gold))


def ref_arm(z, names):
    sys.path.insert(0, os.path.join(ROOT, 'oracle', '_shims'))
    sys.path.insert(0, PLAIN)
    from llmc.compression.quantization.osplus import OsPlus
    from llmc.compression.quantization.quant import IntegerQuantizer
    res = {}
    for name in names:
        cfg, dt, mod, x = C.os_case(z, name)
        if cfg['weight'][0] != 'int' or cfg['act'][0] != 'int':
            continue
        mod, x = mod.cuda(), x.cuda()
        ns = types.SimpleNamespace(wquantizer=IntegerQuantizer(*cfg['weight'][1:]), aquantizer=IntegerQuantizer(*cfg['act'][1:]),
                                   fp8_block_size=128, model=types.SimpleNamespace(has_bias=lambda b=cfg['has_bias']: b))
        for n in ('get_original_out', 'search_scale_shift_subset'):
            setattr(ns, n, types.MethodType(getattr(OsPlus, n), ns))
        calls = []
        h = mod.register_forward_hook(lambda m, a, o: calls.append((o[0] if isinstance(o, tuple) else o).detach().clone()))
        with torch.no_grad():
            ns.search_scale_shift_subset(mod.searched(), [x.clone()], mod, {})
        h.remove()
        loss = torch.stack([(calls[0] - o).pow(2).sum(-1).mean() for o in calls[1:]]).float().cpu().numpy()
        res[name] = loss
    return res


def ours_arm(z, names):
    import llmc_amd.compression.quantization as Q
    res = {}
    for name in names:
        cfg, dt, mod, x = C.os_case(z, name)
        mod, x = mod.cuda(), x.cuda()
        algo = Q.OsPlus(C.OneBlockModel(mod, cfg['has_bias']), C.quant_section(cfg), None, None, {})
        algo.search_scale_shift_subset(mod.searched(), [x.clone()], mod, {})
        res[name] = algo.last_search['losses'].float().cpu().numpy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    z = C.gold()
    names = [str(n) for n in z['os_names']]
    ours = ours_arm(z, names)
    ref = ref_arm(z, names) if os.path.isdir(os.path.join(PLAIN, 'llmc')) else {}
    lines = ['# OS+ loss curves against the reference\'s CPU golden (tools/osplus_parity.py): max over the grid of |loss - golden| / golden',
             '# case dtype points golden_winner | ref_gpu: max_rel_dev winner | ours: max_rel_dev winner']
    worst = {}
    for name in names:
        gold, dt = z[name + '/loss'], str(z[name + '/dt'])
        row = f'{name:28s} {dt:5s} {len(gold):4d} {int(z[name + "/win"]):4d} |'
        if name in ref and len(ref[name]) == len(gold):
            d = curve_dev(ref[name], gold)
            worst.setdefault(dt, {}).setdefault('ref_gpu', []).append(d)
            row += f' {d:.4e} {int(np.argmax(ref[name] == ref[name].min())):4d} |'
        else:
            row += '        n/a  n/a |'
        if len(ours[name]) == len(gold):
            d = curve_dev(ours[name], gold)
            worst.setdefault(dt, {}).setdefault('ours', []).append(d)
            row += f' {d:.4e} {int(np.argmax(ours[name] == ours[name].min())):4d}'
        else:
            row += f' {len(ours[name])} points'
        lines.append(row)
    lines.append('# per dtype: ' + json.dumps({dt: {k: max(v) for k, v in arms.items()} for dt, arms in sorted(worst.items())}))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
