"""Functional wrappers over the SmoothQuant / OS+ entry points of libllmc_hip.so (csrc/smooth_osplus.hip)."""
import torch

from llmc_amd import _ffi

from . import awq_ops
from .quant import FloatQuantizer, IntegerQuantizer

ACT_INT, ACT_FP8 = 0, 1


class ColStats:
    """Running per-column max / min / max|x| (fp32 [3, K], exact: the entries are values of the input dtype) over
    any number of [.., K] tensors — calibration batches, or the weights of a subset."""

    def __init__(self, K, device):
        self.K = int(K)
        self.run = torch.empty((3, self.K), dtype=torch.float32, device=device)
        self.glob = torch.empty(2, dtype=torch.float32, device=device)
        self.n = 0

    def update(self, x):
        _ffi.require_gpu(x)
        L = _ffi.lib()
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        N, K = x2.shape
        if K != self.K:
            raise ValueError(f'ColStats: {K} columns, expected {self.K}')
        ws = _ffi.workspace(L.llmc_col_stats_ws_bytes(N, K), x2.device)
        _ffi.check(L.llmc_col_stats(_ffi.ptr(x2), _ffi.dt(x2), N, K, int(self.n == 0), _ffi.ptr(self.run),
                                    _ffi.ptr(self.glob), _ffi.ptr(ws), _ffi.stream()), 'llmc_col_stats')
        self.n += 1
        return self

    @property
    def max(self):
        return self.run[0]

    @property
    def min(self):
        return self.run[1]

    @property
    def absmax(self):
        return self.run[2]


def col_stats(x):
    """-> ColStats of one tensor: .max / .min / .absmax fp32 [K]; .glob = (max(0, x.max()), min(0, x.min()))."""
    return ColStats(x.shape[-1], x.device).update(x)


def smooth_scales(x_absmax, w_absmax, alpha, dtype):
    """SmoothQuant.search_scale_subset (smoothquant.py:54-59) from fp32 [K] column statistics; result in `dtype`."""
    _ffi.require_gpu(x_absmax, w_absmax)
    K = x_absmax.numel()
    out = torch.empty(K, dtype=dtype, device=x_absmax.device)
    _ffi.check(_ffi.lib().llmc_smooth_scales(_ffi.ptr(x_absmax.contiguous()), _ffi.ptr(w_absmax.contiguous()), _ffi.dt(dtype),
                                             K, float(alpha), float(1 - alpha), _ffi.ptr(out), _ffi.stream()),
               'llmc_smooth_scales')
    return out


def osplus_thresholds(amx, amn):
    """The threshold sequence of osplus.py:104-117, 170, in Python floats exactly as the reference forms it (the number of
    points depends on the fp64 accumulation of `st -= step`). amx / amn: Python floats, already clamped against 0."""
    num = 100 if amx != amx else max(100, int(amx / 0.5))
    bounds = (1.0, max(-amn, amx))
    step = (bounds[1] - bounds[0]) / num
    st, out = bounds[1], []
    while st >= bounds[0]:
        out.append(st)
        st -= step
    return out


def osplus_scale(cmx, cmn, thresholds, index, out=None):
    """cur_scale of grid point `index` (osplus.py:118-131); thresholds: a device tensor in the activation dtype."""
    _ffi.require_gpu(cmx, cmn, thresholds)
    K = cmx.numel()
    if out is None:
        out = torch.empty(K, dtype=thresholds.dtype, device=cmx.device)
    _ffi.check(_ffi.lib().llmc_osplus_scale(_ffi.ptr(cmx), _ffi.ptr(cmn), _ffi.ptr(thresholds), int(index),
                                            _ffi.dt(thresholds), K, _ffi.ptr(out), _ffi.stream()), 'llmc_osplus_scale')
    return out


def act_step_tier(dtype, K):
    """Vectors per thread (2 / 4 / 8 / 14) the fused activation kernel is compiled for at this width; 0: it does not take it
    (K not a whole number of 16-byte vectors, or above 28672 16-bit / 14336 fp32 columns)."""
    return _ffi.lib().llmc_osplus_act_step_tier(_ffi.dt(dtype), int(K))


def act_step_fused_ok(x, aquantizer):
    """The quantizers the fused kernel evaluates: per_token, minmax ranges, integer (sym / asym, rounded zero point) or
    FP8 (e4m3 / e5m2, both rounding semantics)."""
    if aquantizer.granularity != 'per_token' or aquantizer.calib_algo != 'minmax' or x.dtype not in _ffi._DT:
        return False
    if isinstance(aquantizer, IntegerQuantizer) and not aquantizer.round_zp:
        return False
    if not isinstance(aquantizer, (IntegerQuantizer, FloatQuantizer)):
        return False
    return act_step_tier(x.dtype, x.shape[-1]) > 0


def act_step(x, scales, aquantizer, force_two_kernels=False):
    """aquantizer.fake_quant_act_dynamic(x / scales.view(1, -1)) (osplus.py:156-157). One kernel where act_step_fused_ok, else
    awq_ops.div_cols followed by the quantizer (same bits)."""
    _ffi.require_gpu(x, scales)
    if getattr(aquantizer, 'narrow', False):
        raise NotImplementedError(f'act_step with a float quantizer bit={aquantizer.bit}: the fused activation step knows the e4m3 '
                                  'and e5m2 formats only')
    if force_two_kernels or not act_step_fused_ok(x, aquantizer):
        return aquantizer.fake_quant_act_dynamic(awq_ops.div_cols(x, scales))
    L = _ffi.lib()
    x2 = x.reshape(-1, x.shape[-1]).contiguous()
    N, K = x2.shape
    out = torch.empty_like(x2)
    if isinstance(aquantizer, FloatQuantizer):
        kind, mode, sym = ACT_FP8, aquantizer._mode, 1
    else:
        kind, mode, sym = ACT_INT, 0, int(aquantizer.sym)
    _ffi.check(L.llmc_osplus_act_step(_ffi.ptr(x2), _ffi.ptr(scales.contiguous()), _ffi.dt(x2), N, K, kind, sym,
                                      float(aquantizer.qmin), float(aquantizer.qmax), int(mode), _ffi.ptr(out), _ffi.stream()),
               'llmc_osplus_act_step')
    return out.reshape(x.shape)
