"""Functional wrappers over the column-wise min/max quantizer of libllmc_hip.so (csrc/quant_cols.hip): the pass behind
IntegerQuantizer.fake_quant_weight_dynamic(weight, {'dim': 'ic'}) (quant.py:833-869), which AdaDim runs on every forward of
every FakeQuantLinear whose `buf_qdim` is 0. A group is g consecutive rows of one column of the row-major weight [R, K]; group
index k * (R / g) + r / g, the order of reshape_tensor(weight.T).

fake_quant_cols runs the kernel on the weight as it lies: no transposed copy, the result is contiguous in the weight's own
layout. fake_quant_cols_composed is the reference's sequence on the existing row kernels (contiguous transposed copy ->
llmc_quant_dynamic -> transpose back; with round_zp off llmc_minmax_qparams + llmc_quant_static); it is what the tests
compare the kernel against, bit for bit, and what the quantizer falls back to with HOST_OPTIONS['quant_cols'] = 0.

Dispatch: the kernel measured 0.17x - 0.58x of the composition's time at every shape timed (bf16 4096 x 4096, 1024 x 4096,
14336 x 4096, 4096 x 14336; int8 per_channel on the slab path and int4 g = 128 on the tile path; profiles/quant_cols.txt,
tools/bench_quant_cols.py), with no overlap of the min..max ranges, so every call the quantizer's conditions admit goes to the
kernel and no shape class is routed to the composition for speed."""
import torch

from llmc_amd import _ffi

TILE_MAX_G = 256     # groups up to this many rows take the one-launch tile path (csrc/quant_cols.hip: kTileMaxG)
SLAB_ROWS = 64       # rows per slab of the three-launch path for longer groups (kSlab); tests build ragged slabs from it

_CODE_DTYPES = {_ffi.OUT_I32: torch.int32, _ffi.OUT_I8: torch.int8, _ffi.OUT_U8: torch.uint8}


def _check(w, g):
    if w.dim() != 2:
        raise ValueError('fake_quant_cols takes a 2-D [R, K] weight')
    if g <= 0 or w.shape[0] % g:
        raise ValueError(f'Dimension {w.shape[0]} not divisible by group size {g}')


def _operand(w):
    """the weight as the kernel takes it: unit column stride and a row stride >= K; anything else is copied"""
    if w.stride(1) == 1 and w.stride(0) >= w.shape[1]:
        return w
    return w.contiguous()


def path(w, g):
    """The launch path fake_quant_cols(w, g, ...) takes (a pure host call): 0 tile, 1 slabs, 2 scalar."""
    w = _operand(w)
    p = _ffi.lib().llmc_quant_dynamic_cols_path(_ffi.ptr(w), _ffi.dt(w), w.shape[0], w.shape[1], w.stride(0), int(g))
    _ffi.check(min(p, 0), 'llmc_quant_dynamic_cols_path')
    return p


def _group_order(t, R, K, g):
    """[K * R / g, g] rows of the composition -> [R, K] in the weight's layout"""
    return t.reshape(K, R).T


def fake_quant_cols_composed(w, g, sym, round_zp, qmin, qmax, out_kind=_ffi.OUT_FAKE, want_qparams=False):
    """The composition the kernel replaces, on the existing row kernels: w.T made contiguous, cut into rows of g, quantized
    (llmc_quant_dynamic; with round_zp off, llmc_minmax_qparams + llmc_quant_static, the reference's get_tensor_qparams +
    quant_dequant), transposed back and made contiguous. -> out, or (out, scales, zeros) with qparams [K * R / g] in w's dtype
    (zeros None for a symmetric quantizer)."""
    from .quant import IntegerQuantizer
    _ffi.require_gpu(w)
    _check(w, g)
    R, K = w.shape
    q = IntegerQuantizer(8, bool(sym), 'per_channel', int_range=[float(qmin), float(qmax)], round_zp=bool(round_zp))
    rows = w.T.contiguous().reshape(-1, g)
    if q.round_zp:
        qd, scales, zeros = q._dynamic(rows, out_kind, want_qparams)
    else:
        t, scales, zeros, mx, mn = q.get_tensor_qparams(rows)
        qd = q._static(t, scales, zeros, mx, mn, out_kind)
        scales = scales.reshape(-1)
        zeros = None if q.sym else zeros.reshape(-1)
    out = _group_order(qd, R, K, g).contiguous()
    return (out, scales, zeros) if want_qparams else out


def fake_quant_cols(w, g, sym, round_zp, qmin, qmax, out_kind=_ffi.OUT_FAKE, want_qparams=False):
    """w [R, K] on the GPU (row stride >= K) -> its groups of g rows per column through get_minmax_range + get_qparams +
    quant (+ dequant for OUT_FAKE), contiguous [R, K]: fake values in w's dtype or codes. -> out, or (out, scales, zeros)."""
    _ffi.require_gpu(w)
    _check(w, g)
    L = _ffi.lib()
    w = _operand(w)
    R, K = w.shape
    dev = w.device
    out = torch.empty((R, K), dtype=w.dtype if out_kind == _ffi.OUT_FAKE else _CODE_DTYPES[out_kind], device=dev)
    scales = zeros = None
    if want_qparams:
        scales = torch.empty(K * (R // g), dtype=w.dtype, device=dev)
        if not sym:
            zeros = torch.empty(K * (R // g), dtype=w.dtype, device=dev)
    ws = _ffi.workspace(L.llmc_quant_dynamic_cols_ws_bytes(R, K, int(g)), dev)
    _ffi.check(L.llmc_quant_dynamic_cols(
        _ffi.ptr(w), _ffi.dt(w), R, K, w.stride(0), int(g), int(bool(sym)), int(bool(round_zp)), float(qmin), float(qmax),
        int(out_kind), _ffi.ptr(out), _ffi.ptr(scales), _ffi.ptr(zeros), _ffi.ptr(ws), _ffi.stream()), 'llmc_quant_dynamic_cols')
    return (out, scales, zeros) if want_qparams else out
