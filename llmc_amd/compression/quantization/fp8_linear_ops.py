"""The plain W8A8-FP8 Linear on gfx950's fp8 matrix instructions (csrc/fp8_linear.hip): the consumers of the stored form that
deploy('vllm_quant' | 'sgl_quant' | 'lightllm_quant' | 'lightx2v_quant') writes for the reference's backend/{vllm,sglang}/fp8
configurations — a float8_e4m3fn weight [R, K] with a per-channel or per-tensor `weight_scale`, activations quantized per token
on the fly or per tensor with a calibrated `input_scale`. Both scales are constant along K and are applied to the fp32
accumulator in the GEMM's epilogue. An extension: the reference's real-quant Linears raise in forward."""
import torch

from llmc_amd import _ffi

from . import scaled8_ops
from .quant import FloatQuantizer
from .scaled8_ops import _FALLBACK_SEEN, _announce          # noqa: F401  (awq_gemm_ops, module_utils and the tests take them here)

FP8 = torch.float8_e4m3fn
RUNGS = {'decode': 0, 'tile128': 1}         # llmc_fp8_scaled_gemm's launch rungs (include/llmc_hip.h)


def act_mode(act_cfg):
    """What a Linear does with its input under the `act` section of a quant configuration: None (no section: weight-only),
    'dynamic_per_token' or 'static_per_tensor' — the two pairings the FP8 GEMM's epilogue scales cover. NotImplementedError
    names anything else."""
    if act_cfg is None:
        return None
    if act_cfg.get('quant_type', 'int-quant') != 'float-quant' or act_cfg.get('bit') != 'e4m3':
        raise NotImplementedError(f"the FP8 Linear takes e4m3 float-quant activations, got quant_type "
                                  f"{act_cfg.get('quant_type', 'int-quant')!r}, bit {act_cfg.get('bit')!r} (int8 and e5m2 are not provided)")
    static, gran = bool(act_cfg.get('static', False)), act_cfg.get('granularity')
    if not static and gran == 'per_token':
        return 'dynamic_per_token'
    if static and gran == 'per_tensor':
        return 'static_per_tensor'
    raise NotImplementedError(f"the FP8 Linear takes dynamic per_token or static per_tensor activation scales, got "
                              f"{'static' if static else 'dynamic'} {gran}")


def _quantizer(act_cfg):
    if isinstance(act_cfg, FloatQuantizer):
        return act_cfg
    cfg = dict(act_cfg)
    if cfg.pop('quant_type', 'float-quant') != 'float-quant':
        raise NotImplementedError("the FP8 Linear takes float-quant activations (quant_type: float-quant)")
    return FloatQuantizer(**cfg)


def fp8_act_quant(x, act_cfg, input_scale=None):
    """x [..., K] -> (codes float8_e4m3fn [..., K], scales fp32: [..., 1] per token, [1] per tensor) by the FloatQuantizer the
    `act` section describes (or that quantizer itself), through its real-quant route on the [M, K] view: llmc_fp8_quant's codes
    and scales bit for bit, so decode(code) * scale is the fake-quant activation. Dynamic per_token: one scale per row. Static
    per_tensor: `input_scale` is used as given."""
    _ffi.require_gpu(x, input_scale)
    q = _quantizer(act_cfg)
    static = bool(q.kwargs.get('static', input_scale is not None))
    mode = act_mode({'quant_type': 'float-quant', 'bit': q.bit, 'granularity': q.granularity, 'static': static})
    x2 = x.reshape(-1, x.shape[-1])
    if mode == 'static_per_tensor':
        if input_scale is None or input_scale.numel() != 1:
            raise ValueError('fp8_act_quant: static per_tensor activations need the calibrated input_scale (one element), got '
                             f'{None if input_scale is None else tuple(input_scale.shape)}')
        codes, scales, _ = q.real_quant_weight_static(x2, {'scales': input_scale})
        scales = scales.reshape(1)
    else:
        codes, scales, _ = q.real_quant_weight_dynamic(x2)
        scales = scales.reshape(*x.shape[:-1], 1)
    return codes.reshape(x.shape), scales.float()           # widening a 16-bit scale is exact


def fp8_scaled_gemm(a8, a_s, w8, w_s, dtype=torch.bfloat16, bias=None, rung=None):
    """c[..., N] = rnd(((a8 . w8^T) * a_s) * w_s) (+ bias in `dtype`): a8 [..., K] and w8 [N, K] e4m3fn codes, a_s one scale per
    token or one, w_s one per output channel or one; fp32 accumulation of exact products, the two scale products in this order,
    one rounding. K % 128 == 0 (else NotImplementedError: fp8_linear_forward has the fallback). rung: None (the library's
    table), or 'decode' / 'tile128' to name the launch rung (tools, tests)."""
    M, N, K = scaled8_ops.check_gemm('fp8_scaled_gemm', (FP8, torch.uint8), 'e4m3fn codes (float8_e4m3fn or uint8)', a8, a_s, w8, w_s, dtype, bias)
    _ffi.require_gpu(a8, a_s, w8, w_s, bias)
    a8, w8 = a8.contiguous(), w8.contiguous()
    a_s, w_s = a_s.reshape(-1).float().contiguous(), w_s.reshape(-1).float().contiguous()
    c = torch.empty(*a8.shape[:-1], N, dtype=dtype, device=a8.device)
    if bias is not None:
        bias = bias.reshape(-1).to(dtype).contiguous()
    args = (_ffi.ptr(a8), _ffi.ptr(a_s), a_s.numel(), _ffi.ptr(w8), _ffi.ptr(w_s), w_s.numel(), M, N, K, _ffi.dt(dtype), _ffi.ptr(bias), _ffi.ptr(c))
    if rung is None:
        _ffi.check(_ffi.lib().llmc_fp8_scaled_gemm(*args, _ffi.stream()), 'llmc_fp8_scaled_gemm')
    else:
        _ffi.check(_ffi.lib().llmc_fp8_scaled_gemm_on_rung(*args, RUNGS[rung], _ffi.stream()), 'llmc_fp8_scaled_gemm_on_rung')
    return c


def fp8_dequant(codes, scales, dtype):
    """scaled8_ops.dequant; raw bytes (uint8) are e4m3fn codes."""
    return scaled8_ops.dequant(codes.view(FP8) if codes.dtype == torch.uint8 else codes, scales, dtype)


def fp8_linear_forward(x, w8, w_s, act_cfg, input_scale, bias):
    """scaled8_ops.linear_forward on fp8_act_quant and fp8_scaled_gemm; the GEMM does not take K % 128 != 0."""
    return scaled8_ops.linear_forward('fp8_linear', fp8_act_quant, fp8_scaled_gemm, fp8_dequant, x, w8, w_s, act_cfg, input_scale, bias)
