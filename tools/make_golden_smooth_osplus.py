"""Write tests/golden/smooth_osplus.npz and tests/golden/ref_smooth_osplus_configs.json: the reference's SmoothQuant
(smoothquant.py) and OsPlus (osplus.py) on CPU.

Usage (where the reference tree exists; it needs no GPU):  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_smooth_osplus.py

The reference imports and CPU shims come from oracle/make_golden.py, read-only. SmoothQuant.search_scale_subset and
OsPlus.search_scale_shift_subset / subset_transform run unmodified, bound onto a SimpleNamespace that carries what they read
(model.has_bias, wquantizer, aquantizer, get_original_out, the scale / shift folds of the base class).

Two things about the reference on a CPU:
  * host aliasing — OsPlus copies the inspected module's state dict with `v.cpu()` (osplus.py:54), which on a CPU run ALIASES
    the live parameters, so the in-place `fc.bias.data += shift @ W.T` (osplus.py:135) accumulates over the grid; on a GPU
    the copy is real. `Tensor.cpu` returns a clone for the duration of every call here (the patch oracle/make_golden.py
    applies for Awq); the npz says so in `note`.
  * ties — a 16-bit loss has few significant bits, several thresholds can share the minimum. A case is flagged `clear` when
    its minimum is unique in the model dtype and the fp32-recomputed runner-up is at least 1e-3 (relative) away.

Per OS+ case: inputs as bit patterns of the model dtype, cmx / cmn / shift / amx / amn, the fp64 threshold list, cur_scale at
three grid points, the fake-quantized weight of the first layer and q_x at one grid point (taken from the inspected module
with forward hooks), the loss curve in the model dtype and in fp32, the winning index, the returned scale / shift.
FloatQuantizer cases bind float_quantize to the restated qtorch of oracle/quant_ref.py, like the other FP8 goldens."""
import glob
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.make_golden import DT, GOLD, IntegerQuantizer, _qtorch_stub, f32, save  # noqa: E402
from oracle.build_ref import REF  # noqa: E402
from smooth_osplus_cases import GatedMLP, OptShaped, Stack  # noqa: E402  (tests/: the modules the cases are built from)

import llmc.compression.quantization.quant as qmod  # noqa: E402  (reference)
from llmc.compression.quantization.base_blockwise_quantization import BaseBlockwiseQuantization as RefBase  # noqa: E402
from llmc.compression.quantization.osplus import OsPlus  # noqa: E402
from llmc.compression.quantization.smoothquant import SmoothQuant  # noqa: E402

qmod.float_quantize = _qtorch_stub
REF_CONFIGS = os.path.join(REF, 'configs', 'quantization')
NOTE = ('Tensor.cpu returned a clone during every OsPlus call: on a CPU the reference\'s `org_sd = {k: v.cpu()}` aliases the '
        'live parameters and the in-place bias shift accumulates over the grid; on a GPU the copy is real.')


def bits(t):
    """a tensor's own bit pattern (uint16 for 16-bit dtypes, uint32 for fp32)"""
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32).copy()
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def make_q(kind, bit, sym, gran):
    if kind == 'int':
        return IntegerQuantizer(bit, sym, gran)
    return qmod.FloatQuantizer(bit, sym, gran, use_qtorch=True)


def init_module(m, gen, dt):
    for p in m.parameters():
        p.data = (torch.randn(p.shape, generator=gen) * (0.05 if p.dim() == 2 else 0.1))
    return m.to(DT[dt])


def make_x(gen, shape, dt, offset):
    """log-normal channel magnitudes, 4 outlier channels x30; with `offset` the outliers sit off-centre (a shift to find);
    a planted all-zero token and a constant token"""
    K = shape[-1]
    c = torch.exp(0.5 * torch.randn(K, generator=gen))
    idx = torch.randperm(K, generator=gen)[:4]
    c[idx] *= 30
    x = torch.randn(*shape, generator=gen) * c
    if offset:
        x[..., idx] += 2.0 * c[idx]
    x.reshape(-1, K)[0] = 0.0
    x.reshape(-1, K)[1] = 0.25
    return x.to(DT[dt])


def osplus_ns(wq, aq, has_bias):
    ns = types.SimpleNamespace(wquantizer=wq, aquantizer=aq, act_static=False, fp8_block_size=128,
                               model=types.SimpleNamespace(has_bias=lambda: has_bias))
    for name in ('get_original_out', 'search_scale_shift_subset', 'filter_subset', 'subset_transform'):
        setattr(ns, name, types.MethodType(getattr(OsPlus, name), ns))
    for name in ('apply_shift', 'apply_scale', 'shift_ln_fcs', 'scale_ln_fcs', 'shift_fc_fc', 'scale_fc_fc'):
        setattr(ns, name, types.MethodType(getattr(RefBase, name), ns))
    return ns


def thresholds(amx, amn):
    """the loop of osplus.py:104-117, 170 restated to record the list the reference walks"""
    num = 100 if amx != amx else max(100, int(amx / 0.5))
    b1 = max(-amn, amx)
    step = (b1 - 1.0) / num
    st, out = b1, []
    while st >= 1.0:
        out.append(st)
        st -= step
    return out


# name, dtype, weight quantizer, act quantizer, has_bias, module, K, R, x shape
W8 = ('int', 8, True, 'per_channel')
OS_CASES = [
    ('w8a8_bf16_mlp', 'bf16', W8, ('int', 8, True, 'per_token'), False, 'mlp', 128, 48, (1, 48, 128)),
    ('w8a8_f16_mlp', 'f16', W8, ('int', 8, True, 'per_token'), False, 'mlp', 128, 48, (1, 48, 128)),
    ('w8a8_f32_stack', 'f32', W8, ('int', 8, True, 'per_token'), False, 'stack', 128, 48, (48, 128)),
    ('w8a8_f16_mlp_bias', 'f16', W8, ('int', 8, True, 'per_token'), True, 'mlp', 128, 48, (1, 48, 128)),
    ('w8a8_bf16_stack_bias', 'bf16', W8, ('int', 8, True, 'per_token'), True, 'stack', 128, 48, (1, 48, 128)),
    ('w8a8_asym_f16_stack_bias', 'f16', W8, ('int', 8, False, 'per_token'), True, 'stack', 128, 48, (48, 128)),
    ('fp8_e4m3_bf16_mlp', 'bf16', ('float', 'e4m3', True, 'per_channel'), ('float', 'e4m3', True, 'per_token'), False, 'mlp',
     128, 48, (1, 48, 128)),
    ('w8a8_f16_mlp_k120', 'f16', W8, ('int', 8, True, 'per_token'), False, 'mlp', 120, 48, (1, 40, 120)),
]
# name, dtype, alpha, K, R, batches
SQ_CASES = [('sq_a050_bf16', 'bf16', 0.5, 128, 32, 3), ('sq_a075_f16', 'f16', 0.75, 128, 32, 2),
            ('sq_a050_f32', 'f32', 0.5, 120, 32, 2), ('sq_a075_f32', 'f32', 0.75, 128, 32, 2)]


def run_osplus(name, dt, wcfg, acfg, has_bias, kind, K, R, shape, gen, out):
    wq, aq = make_q(*wcfg), make_q(*acfg)
    mod = init_module((GatedMLP if kind == 'mlp' else Stack)(K, R, has_bias), gen, dt)
    x = make_x(gen, shape, dt, has_bias)
    layers = mod.searched()
    p = name + '/'
    out[p + 'x_bits'] = bits(x)
    out[p + 'x_shape'] = np.array(shape, np.int64)
    for n, t in mod.state_dict().items():
        out[p + 'sd/' + n] = bits(t)
    # statistics as osplus.py:61-102 forms them
    red = (0, 1) if x.dim() == 3 else 0
    if has_bias:
        shift = (torch.amax(x, dim=red) + torch.amin(x, dim=red)) / 2
        xs = x - shift
    else:
        shift, xs = None, x.clone()
    cmx, cmn = torch.amax(xs, dim=red), torch.amin(xs, dim=red)
    amx = max(xs.max(), torch.tensor(0.0, dtype=xs.dtype))
    amn = min(xs.min(), torch.tensor(0.0, dtype=xs.dtype))
    thr = thresholds(amx.item(), amn.item())
    sample = [0, len(thr) // 3, len(thr) - 1]

    def cur_scale(st):
        one = torch.tensor(1.0, dtype=xs.dtype)
        mx = torch.where(cmx > torch.tensor(st, dtype=xs.dtype), cmx / torch.tensor(st, dtype=xs.dtype), one)
        mn = torch.where(cmn < torch.tensor(-st, dtype=xs.dtype), cmn / torch.tensor(-st, dtype=xs.dtype), one)
        return torch.max(mx, mn)

    calls, keep = [], {}
    g_star = sample[1] + 1                           # call 0 is get_original_out

    def pre(m, args):
        if len(calls) == g_star:
            keep['q_x'] = args[0].detach().clone()
            keep['wq'] = layers[0].weight.data.detach().clone()
            if has_bias:
                keep['bias'] = layers[0].bias.data.detach().clone()

    def post(m, args, o):
        calls.append((o[0] if isinstance(o, tuple) else o).detach().clone())

    h1, h2 = mod.register_forward_pre_hook(pre), mod.register_forward_hook(post)
    ns = osplus_ns(wq, aq, has_bias)
    sd0 = {k: v.clone() for k, v in mod.state_dict().items()}
    orig_cpu = torch.Tensor.cpu
    torch.Tensor.cpu = lambda self, *a, **k: self.clone()
    try:
        scale, shift_ret = ns.search_scale_shift_subset(layers, [x.clone()], mod, {})
    finally:
        torch.Tensor.cpu = orig_cpu
        h1.remove()
        h2.remove()
    for k, v in mod.state_dict().items():
        assert torch.equal(v, sd0[k]), f'{name}: {k} not restored'
    assert len(calls) == len(thr) + 1, (name, len(calls), len(thr))
    org = calls[0]
    loss = torch.stack([(org - o).pow(2).sum(-1).mean() for o in calls[1:]])
    loss32 = torch.stack([(org.float() - o.float()).pow(2).sum(-1).mean() for o in calls[1:]])
    best, win = None, 0
    for i, l in enumerate(loss):                      # osplus.py:165
        if best is None or best > l:
            best, win = l, i
    assert torch.equal(scale, cur_scale(thr[win])), f'{name}: returned scale is not the winner\'s'
    lf = loss.float()
    unique = int((lf == lf[win]).sum()) == 1
    o32 = torch.sort(loss32).values
    gap = float((o32[1] - o32[0]) / o32[0])
    clear = bool(unique and gap >= 1e-3 and int(torch.argmin(loss32)) == win)
    out[p + 'dt'] = np.array(dt)
    out[p + 'cfg'] = np.array(json.dumps(dict(weight=wcfg, act=acfg, has_bias=has_bias, module=kind, K=K, R=R)))
    out[p + 'cmx'], out[p + 'cmn'] = bits(cmx), bits(cmn)
    out[p + 'amx'], out[p + 'amn'] = np.array(amx.item(), np.float64), np.array(amn.item(), np.float64)
    if has_bias:
        out[p + 'shift'] = bits(shift)
        assert torch.equal(shift, shift_ret)
        out[p + 'bias_shifted'] = bits(keep['bias'])
    else:
        assert shift_ret is None
    out[p + 'thresholds'] = np.array(thr, np.float64)
    out[p + 'sample_idx'] = np.array(sample, np.int64)
    out[p + 'cur_scale'] = np.stack([bits(cur_scale(thr[i])) for i in sample])
    out[p + 'g_star'] = np.array(sample[1], np.int64)
    out[p + 'wq_bits'], out[p + 'q_x_bits'] = bits(keep['wq']), bits(keep['q_x'])
    out[p + 'loss'], out[p + 'loss32'] = f32(loss), f32(loss32)
    out[p + 'win'] = np.array(win, np.int64)
    out[p + 'clear'] = np.array(int(clear))
    out[p + 'gap32'] = np.array(gap)
    out[p + 'scale'] = bits(scale)
    print(f'{name}: {len(thr)} points, winner {win}, unique {unique}, fp32 gap {gap:.2e}, clear {clear}')
    return clear


def run_smooth(name, dt, alpha, K, R, nb, gen, out):
    fcs = [init_module(torch.nn.Linear(K, R, bias=False), gen, dt) for _ in range(2)]
    fcs[0].weight.data[:, 5] = 0.0
    fcs[1].weight.data[:, 5] = 0.0                   # w_max clamps at 1e-5 there
    xs = [make_x(gen, (2, 12, K), dt, False) for _ in range(nb)]
    ns = types.SimpleNamespace(alpha=alpha)
    for n in ('get_weight_scale', 'get_act_scale', 'search_scale_subset'):
        setattr(ns, n, types.MethodType(getattr(SmoothQuant, n), ns))
    ns.collect_layers_weights = types.MethodType(RefBase.collect_layers_weights, ns)
    p = name + '/'
    out[p + 'dt'], out[p + 'alpha'] = np.array(dt), np.array(alpha)
    for i, fc in enumerate(fcs):
        out[p + f'w{i}_bits'] = bits(fc.weight.data)
    for i, x in enumerate(xs):
        out[p + f'x{i}_bits'] = bits(x)
    out[p + 'x_shape'] = np.array([2, 12, K], np.int64)
    out[p + 'n_batches'] = np.array(nb)
    out[p + 'w_max'] = bits(ns.get_weight_scale(fcs))
    out[p + 'x_max'] = f32(ns.get_act_scale([x.clone() for x in xs]))
    out[p + 'scale'] = bits(ns.search_scale_subset(fcs, [x.clone() for x in xs]))
    print(f'{name}: done')


def run_transform(gen, out):
    """OsPlus.subset_transform (search, apply_shift, apply_scale) on the fc1 subset of an OPT-shaped block, f16"""
    dt, H, F = 'f16', 128, 128
    blk = init_module(OptShaped(H, F), gen, dt)
    blk.final_layer_norm.weight.data = (1 + 0.1 * torch.randn(H, generator=gen)).to(DT[dt])
    x = make_x(gen, (1, 32, H), dt, True) * 0.1
    feat = blk.final_layer_norm(x)
    p = 'transform/'
    out[p + 'x_bits'] = bits(x)
    for n, t in blk.state_dict().items():
        out[p + 'sd/' + n] = bits(t)
    before = blk(x).float()
    ns = osplus_ns(make_q(*W8), make_q('int', 8, True, 'per_token'), True)
    subset = {'layers': {'fc1': blk.fc1}, 'prev_op': [blk.final_layer_norm], 'input': ['fc1'], 'inspect': blk.fc1,
              'has_kwargs': False}
    orig_cpu = torch.Tensor.cpu
    torch.Tensor.cpu = lambda self, *a, **k: self.clone()
    try:
        ns.subset_transform(subset, {'fc1': [feat.clone()]}, {})
    finally:
        torch.Tensor.cpu = orig_cpu
    after = blk(x).float()
    for n, t in blk.state_dict().items():
        out[p + 'sd_after/' + n] = bits(t)
    out[p + 'before_after_maxabs'] = np.array(float((before - after).detach().abs().max()))
    out[p + 'out_absmax'] = np.array(float(before.detach().abs().max()))
    print(f'transform: max |before - after| = {float((before - after).detach().abs().max()):.3e} of {float(before.detach().abs().max()):.3e}')


def configs():
    import yaml
    res = {}
    for f in sorted(glob.glob(REF_CONFIGS + '/**/*.y*ml', recursive=True)):
        try:
            c = yaml.safe_load(open(f))
        except Exception:       # noqa: BLE001
            continue
        q = (c or {}).get('quant') or {}
        # the method sits in `quant`, or one level down under a modality key (quant.video_gen of the video_gen files)
        sections = [q] + [v for v in q.values() if isinstance(v, dict)] if isinstance(q, dict) else []
        if any(s.get('method') in ('SmoothQuant', 'OsPlus') for s in sections):
            rel = os.path.relpath(f, REF_CONFIGS)
            assert json.loads(json.dumps(c)) == c, f'{rel} does not survive JSON'
            res[rel] = c
    path = os.path.join(GOLD, 'ref_smooth_osplus_configs.json')
    with open(path, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(f'wrote {path}: {len(res)} files')


def main():
    gen = torch.Generator().manual_seed(20261016)
    out = {}
    n_clear = 0
    for c in OS_CASES:
        n_clear += run_osplus(*c, gen, out)
    assert n_clear >= 3, f'only {n_clear} clear cases'
    for c in SQ_CASES:
        run_smooth(*c, gen, out)
    run_transform(gen, out)
    out['os_names'] = np.array([c[0] for c in OS_CASES])
    out['sq_names'] = np.array([c[0] for c in SQ_CASES])
    out['note'] = np.array(NOTE)
    save('smooth_osplus', **out)
    configs()


if __name__ == '__main__':
    main()
