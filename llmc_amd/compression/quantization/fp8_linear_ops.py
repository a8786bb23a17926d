"""The plain W8A8-FP8 Linear on gfx950's fp8 matrix instructions (csrc/fp8_linear.hip): the consumers of the stored form that
deploy('vllm_quant' | 'sgl_quant' | 'lightllm_quant' | 'lightx2v_quant') writes for the reference's backend/{vllm,sglang}/fp8
configurations — a float8_e4m3fn weight [R, K] with a per-channel or per-tensor `weight_scale`, activations quantized per token
on the fly or per tensor with a calibrated `input_scale`. Both scales are constant along K and are applied to the fp32
accumulator in the GEMM's epilogue. An extension: the reference's real-quant Linears raise in forward."""
import sys

import torch

from llmc_amd import _ffi

from .quant import FloatQuantizer

FP8 = torch.float8_e4m3fn
RUNGS = {'decode': 0, 'tile128': 1}         # llmc_fp8_scaled_gemm's launch rungs (include/llmc_hip.h)
_FALLBACK_SEEN = set()


def _announce(what, sig, why, instead):
    if (what, sig) not in _FALLBACK_SEEN:
        _FALLBACK_SEEN.add((what, sig))
        print(f'[llmc_amd] {what} {sig}: {why} -> {instead}', file=sys.stderr)


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


def _check_gemm(a8, a_s, w8, w_s, dtype, bias):
    """Shapes and dtypes of an fp8_scaled_gemm call; returns (M, N, K). Raises before anything touches the GPU."""
    for name, t in (('a8', a8), ('w8', w8)):
        if t.dtype not in (FP8, torch.uint8):
            raise TypeError(f'fp8_scaled_gemm: {name} holds e4m3fn codes (float8_e4m3fn or uint8), got {t.dtype}')
    if w8.dim() != 2 or a8.dim() < 1:
        raise ValueError(f'fp8_scaled_gemm: the weight is [N, K] and the activation [..., K], got {tuple(w8.shape)} and {tuple(a8.shape)}')
    N, K = w8.shape
    if a8.shape[-1] != K:
        raise ValueError(f'fp8_scaled_gemm: activation and weight disagree on K ({a8.shape[-1]} and {K})')
    M = a8.numel() // max(K, 1)
    if M < 1 or N < 1 or K < 1:
        raise ValueError(f'fp8_scaled_gemm: empty operand (M, N, K = {M}, {N}, {K})')
    if a_s.numel() not in (1, M):
        raise ValueError(f'fp8_scaled_gemm: a_s holds one scale per token ({M}) or one, got {a_s.numel()}')
    if w_s.numel() not in (1, N):
        raise ValueError(f'fp8_scaled_gemm: w_s holds one scale per output channel ({N}) or one, got {w_s.numel()}')
    for name, t in (('a_s', a_s), ('w_s', w_s)):
        if t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError(f'fp8_scaled_gemm: {name} is fp32, fp16 or bf16, got {t.dtype}')
    if dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f'fp8_scaled_gemm: the output is fp32, fp16 or bf16, got {dtype}')
    if bias is not None and bias.numel() != N:
        raise ValueError(f'fp8_scaled_gemm: the bias holds {N} elements, got {bias.numel()}')
    return M, N, K


def fp8_scaled_gemm(a8, a_s, w8, w_s, dtype=torch.bfloat16, bias=None, rung=None):
    """c[..., N] = rnd(((a8 . w8^T) * a_s) * w_s) (+ bias in `dtype`): a8 [..., K] and w8 [N, K] e4m3fn codes, a_s one scale per
    token or one, w_s one per output channel or one; fp32 accumulation of exact products, the two scale products in this order,
    one rounding. K % 128 == 0 (else NotImplementedError: fp8_linear_forward has the fallback). rung: None (the library's
    table), or 'decode' / 'tile128' to name the launch rung (tools, tests)."""
    M, N, K = _check_gemm(a8, a_s, w8, w_s, dtype, bias)
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
    """decode(code) * scale, an fp32 product rounded once to `dtype`: the weight (scales [R, 1] or one) or the activation
    (scales [..., 1] or one) back as numbers."""
    if codes.dtype == torch.uint8:
        codes = codes.view(FP8)
    s = scales.float()
    return (codes.float() * (s.reshape(()) if s.numel() == 1 else s.reshape(*codes.shape[:-1], 1))).to(dtype)


def fp8_linear_forward(x, w8, w_s, act_cfg, input_scale, bias):
    """Quantize the activation (fp8_act_quant), multiply by the FP8 weight; the output takes the activation's dtype. A depth the
    GEMM does not take (K % 128 != 0) goes, said once per shape on stderr, through the 16-bit GEMM on the two de-quantized operands:
    the fake-quant Linear of the same codes. Nothing takes that way for speed."""
    codes, scales = fp8_act_quant(x.contiguous(), act_cfg, input_scale)
    try:
        return fp8_scaled_gemm(codes, scales, w8, w_s, dtype=x.dtype, bias=bias)
    except NotImplementedError as e:          # LLMC_ENOTSUP: nothing was launched
        why = str(e)
    from .module_utils import hip_linear
    _announce('fp8_linear', (tuple(x.shape), tuple(w8.shape), str(x.dtype)), why, 'de-quantized operands through the 16-bit HIP GEMM')
    return hip_linear(fp8_dequant(codes, scales, x.dtype), fp8_dequant(w8, w_s, x.dtype), bias)
