"""Functional wrappers over the mixed int / fp column entry point of libllmc_hip.so (csrc/mixed_quant.hip): the pass behind
IntegerQuantizer.fake_quant_act_dynamic / fake_quant_weight_dynamic with `int_indices` / `fp_indices` (quant.py:754-783,
833-869), which QUIK and LLM.int8() run on every forward of every FakeQuantLinear.

fake_quant_mixed runs one kernel: a row is read once, the gather by `int_indices` and the write-back happen in LDS, the row
is written once. fake_quant_mixed_composed is the reference's own sequence on the existing kernels (index_select ->
IntegerQuantizer._dynamic -> index_copy_ into zeros -> index_copy_ of the fp columns); it serves rows the resident kernel
refuses (llmc_quant_dynamic_mixed_fits) and is what the tests compare the kernel against, bit for bit.

Dispatch: the kernel measured 1.7x - 6.1x faster than the composition at every shape timed (activations [2048, 4096 .. 28672]
per_token, 4096 x 4096 weights per_channel and per_group g = 128 in scale order; profiles/mixed_quant.txt, tools/bench_mixed_quant.py),
so every width the kernel takes goes to it and no case is routed to the composition for speed.

Duplicate entries inside `int_indices` are undefined, as they are for torch's scatter (the reference's `mix[:, idx] = q`):
which of the duplicates' values lands is not specified. They are refused (ValueError) only where that costs nothing: more
integer columns than the tensor has columns. A column named in both lists passes through, and still counts in its group's
min / max, as in the reference, whose fp scatter comes second. Indices outside [0, K) are ignored by the kernel."""
import torch

from llmc_amd import _ffi

ROLE_ZERO, ROLE_INT, ROLE_FP = 0, 1, 2


def _check(x2d, int_indices, g):
    if x2d.dim() != 2:
        raise ValueError('fake_quant_mixed takes a 2-D [N, K] tensor')
    n_int = int(int_indices.numel())
    if n_int == 0:
        raise ValueError('int_indices is empty: nothing to quantize (the reference fails in amax on an empty dimension)')
    if n_int > x2d.shape[1]:
        raise ValueError(f'{n_int} integer columns for a tensor of {x2d.shape[1]} columns: int_indices has duplicates')
    if g <= 0 or n_int % g:
        raise ValueError(f'{n_int} integer columns are not a whole number of groups of {g}')
    return n_int


def _quantizer(g, sym, round_zp, qmin, qmax):
    """An IntegerQuantizer whose [G, g] rows are the groups (per_channel: one group per row of the tensor it is given)."""
    from .quant import IntegerQuantizer
    return IntegerQuantizer(8, bool(sym), 'per_channel', int_range=[float(qmin), float(qmax)], round_zp=bool(round_zp))


def make_roles(K, int_indices, fp_indices, device):
    """uint8 [K] for the kernel, built on the device without a host synchronisation: 1 on the integer columns, +2 on the fp
    columns (so 3 = named in both lists: passes through, counts in its group's range), 0 elsewhere."""
    role = torch.zeros(K, dtype=torch.uint8, device=device)
    role[int_indices.to(device=device, dtype=torch.long)] = ROLE_INT
    if fp_indices is not None and fp_indices.numel():
        fp = fp_indices.to(device=device, dtype=torch.long)
        role[fp] = role[fp] + ROLE_FP
    return role


def fake_quant_mixed_composed(x2d, int_indices, fp_indices, g, sym, round_zp, qmin, qmax):
    """The reference's sequence (quant.py:754-783) on the existing kernels: gather, quantize the contiguous copy in groups of g
    (llmc_quant_dynamic; with round_zp off, llmc_minmax_qparams + llmc_quant_static, the reference's get_tensor_qparams +
    quant_dequant), scatter into zeros, scatter the fp columns over it."""
    _ffi.require_gpu(x2d)
    _check(x2d, int_indices, g)
    dev = x2d.device
    ii = int_indices.to(device=dev, dtype=torch.long)
    q = _quantizer(g, sym, round_zp, qmin, qmax)
    gathered = x2d.index_select(1, ii).reshape(-1, g)
    if q.round_zp:
        qd, _, _ = q._dynamic(gathered, _ffi.OUT_FAKE, False)
    else:
        t, scales, zeros, mx, mn = q.get_tensor_qparams(gathered)
        qd = q.quant_dequant(t, scales, zeros, mx, mn)
    out = torch.zeros_like(x2d)
    out.index_copy_(1, ii, qd.reshape(x2d.shape[0], -1))
    if fp_indices is not None and fp_indices.numel():
        fi = fp_indices.to(device=dev, dtype=torch.long)
        out.index_copy_(1, fi, x2d.index_select(1, fi))
    return out


def kernel_takes(x2d):
    """Whether the resident kernel takes rows of this width and dtype (a pure host call)."""
    return x2d.dtype in _ffi._DT and bool(_ffi.lib().llmc_quant_dynamic_mixed_fits(_ffi.dt(x2d), int(x2d.shape[1])))


def fake_quant_mixed(x2d, int_indices, fp_indices, g, sym, round_zp, qmin, qmax, out=None):
    """x2d [N, K] on the GPU -> fake-quantized integer columns (groups of g in the order of int_indices), the fp columns' own
    bits, +0 elsewhere. `out` may be x2d itself."""
    _ffi.require_gpu(x2d)
    n_int = _check(x2d, int_indices, g)
    if not kernel_takes(x2d):
        res = fake_quant_mixed_composed(x2d, int_indices, fp_indices, g, sym, round_zp, qmin, qmax)
        if out is not None:
            out.copy_(res)
            return out
        return res
    x2 = x2d.contiguous()
    N, K = x2.shape
    role = make_roles(K, int_indices, fp_indices, x2.device)
    # one group per row needs no order: the mask alone drives the kernel
    idx = None if g == n_int else int_indices.to(device=x2.device, dtype=torch.int32).contiguous()
    if out is None:
        out = torch.empty_like(x2)
    elif out.shape != x2.shape or out.dtype != x2.dtype or not out.is_contiguous():
        raise ValueError('fake_quant_mixed: out must be a contiguous tensor of x2d\'s shape and dtype')
    _ffi.check(_ffi.lib().llmc_quant_dynamic_mixed(
        _ffi.ptr(x2), _ffi.dt(x2), N, K, _ffi.ptr(role), _ffi.ptr(idx), n_int, int(g), int(bool(sym)), int(bool(round_zp)),
        float(qmin), float(qmax), _ffi.ptr(out), _ffi.stream()), 'llmc_quant_dynamic_mixed')
    return out
