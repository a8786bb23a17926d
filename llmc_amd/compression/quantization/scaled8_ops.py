"""What the two W8A8 Linears on the 8-bit matrix instructions (fp8_linear_ops, i8_linear_ops; csrc/scaled8_gemm.h) share on the
Python side: the checks of a scaled GEMM call, the de-quantization of codes with scales constant along K, and the forward's
"quantize, multiply, or say once and take the 16-bit GEMM" scaffold."""
import sys

import torch

_FALLBACK_SEEN = set()          # one "said once" record for every real-quant Linear


def _announce(what, sig, why, instead):
    if (what, sig) not in _FALLBACK_SEEN:
        _FALLBACK_SEEN.add((what, sig))
        print(f'[llmc_amd] {what} {sig}: {why} -> {instead}', file=sys.stderr)


def check_gemm(name, code_dtypes, codes, a8, a_s, w8, w_s, dtype, bias):
    """Shapes and dtypes of a `name` call (fp8_scaled_gemm, i8_scaled_gemm) on codes of one of code_dtypes (`codes`: what
    the message calls them); returns (M, N, K). Raises before anything touches the GPU."""
    for arg, t in (('a8', a8), ('w8', w8)):
        if t.dtype not in code_dtypes:
            raise TypeError(f'{name}: {arg} holds {codes}, got {t.dtype}')
    if w8.dim() != 2 or a8.dim() < 1:
        raise ValueError(f'{name}: the weight is [N, K] and the activation [..., K], got {tuple(w8.shape)} and {tuple(a8.shape)}')
    N, K = w8.shape
    if a8.shape[-1] != K:
        raise ValueError(f'{name}: activation and weight disagree on K ({a8.shape[-1]} and {K})')
    M = a8.numel() // max(K, 1)
    if M < 1 or N < 1 or K < 1:
        raise ValueError(f'{name}: empty operand (M, N, K = {M}, {N}, {K})')
    if a_s.numel() not in (1, M):
        raise ValueError(f'{name}: a_s holds one scale per token ({M}) or one, got {a_s.numel()}')
    if w_s.numel() not in (1, N):
        raise ValueError(f'{name}: w_s holds one scale per output channel ({N}) or one, got {w_s.numel()}')
    for arg, t in (('a_s', a_s), ('w_s', w_s)):
        if t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError(f'{name}: {arg} is fp32, fp16 or bf16, got {t.dtype}')
    if dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f'{name}: the output is fp32, fp16 or bf16, got {dtype}')
    if bias is not None and bias.numel() != N:
        raise ValueError(f'{name}: the bias holds {N} elements, got {bias.numel()}')
    return M, N, K


def dequant(codes, scales, dtype):
    """decode(code) * scale, an fp32 product rounded once to `dtype`: the weight (scales [R, 1] or one) or the activation
    (scales [..., 1] or one) back as numbers."""
    s = scales.float()
    return (codes.float() * (s.reshape(()) if s.numel() == 1 else s.reshape(*codes.shape[:-1], 1))).to(dtype)


def linear_forward(name, act_quant, gemm, dequant, x, w8, w_s, act_cfg, input_scale, bias):
    """Quantize the activation (act_quant), multiply by the 8-bit weight (gemm); the output takes the activation's dtype. A depth
    the GEMM does not take goes, said once per shape on stderr under `name`, through the 16-bit GEMM on the two operands
    de-quantized by `dequant`: the fake-quant Linear of the same codes. Nothing takes that way for speed."""
    codes, scales = act_quant(x.contiguous(), act_cfg, input_scale)
    try:
        return gemm(codes, scales, w8, w_s, dtype=x.dtype, bias=bias)
    except NotImplementedError as e:          # LLMC_ENOTSUP: nothing was launched
        why = str(e)
    from .module_utils import hip_linear
    _announce(name, (tuple(x.shape), tuple(w8.shape), str(x.dtype)), why, 'de-quantized operands through the 16-bit HIP GEMM')
    return hip_linear(dequant(codes, scales, x.dtype), dequant(w8, w_s, x.dtype), bias)
