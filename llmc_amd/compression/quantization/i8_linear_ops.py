"""The W8A8 integer Linear on gfx950's int8 matrix instructions (csrc/i8_linear.hip): the consumers of the stored form that
deploy('vllm_quant' | 'sgl_quant' | 'lightllm_quant' | 'lightx2v_quant') writes for the reference's
backend/{vllm,sglang}/{smoothquant,awq,rtn}_w8a8 configurations — an int8 weight [R, K] with a per-channel or per-tensor
`weight_scale`, activations quantized to symmetric int8 per token on the fly or per tensor with a calibrated `input_scale`. Both
scales are constant along K and are applied to the exact int32 accumulator in the GEMM's epilogue. An extension: the reference's
real-quant Linears raise in forward. Weight-only int8 / int4 and the packed (`need_pack`) form are not run here."""
import torch

from llmc_amd import _ffi

from . import scaled8_ops
from .quant import IntegerQuantizer
from .scaled8_ops import _FALLBACK_SEEN, _announce          # noqa: F401  (the tests take them here)

RUNGS = {'decode': 0, 'tile128': 1, 'decode_split': 2}         # llmc_i8_scaled_gemm's launch rungs (include/llmc_hip.h)
DECODE_MAX_M = 64                                              # the most rows the two decode rungs take
MAX_K = 65536


def act_mode(act_cfg):
    """What a Linear with an int8 weight does with its input under the `act` section of a quant configuration: None (no section:
    weight-only), 'dynamic_per_token' or 'static_per_tensor' — the two pairings the integer GEMM's epilogue scales cover.
    NotImplementedError names anything else."""
    if act_cfg is None:
        return None
    qt, bit = act_cfg.get('quant_type', 'int-quant'), act_cfg.get('bit')
    if qt != 'int-quant' or bit != 8:
        raise NotImplementedError(f'the INT8 Linear takes 8-bit int-quant activations, got quant_type {qt!r}, bit {bit!r} '
                                  '(W8A8 only: other activation widths and float activations on an int8 weight are not provided)')
    if not act_cfg.get('symmetric', False):
        raise NotImplementedError('the INT8 Linear takes symmetric activations, got asymmetric (a zero point does not leave the '
                                  'K loop as a scale does)')
    static, gran = bool(act_cfg.get('static', False)), act_cfg.get('granularity')
    if not static and gran == 'per_token':
        return 'dynamic_per_token'
    if static and gran == 'per_tensor':
        return 'static_per_tensor'
    raise NotImplementedError(f"the INT8 Linear takes dynamic per_token or static per_tensor activation scales, got "
                              f"{'static' if static else 'dynamic'} {gran}")


def _quantizer(act_cfg):
    if isinstance(act_cfg, IntegerQuantizer):
        return act_cfg
    cfg = dict(act_cfg)
    if cfg.pop('quant_type', 'int-quant') != 'int-quant':
        raise NotImplementedError('the INT8 Linear takes int-quant activations (quant_type: int-quant)')
    return IntegerQuantizer(**cfg)


def i8_act_quant(x, act_cfg, input_scale=None):
    """x [..., K] -> (codes int8 [..., K], scales fp32: [..., 1] per token, [1] per tensor) by the IntegerQuantizer the `act`
    section describes (or that quantizer itself), through its real-quant route on the [M, K] view: llmc_quant_dynamic's /
    llmc_quant_static's codes and scales, so codes.float() * scale rounded to x.dtype is the fake-quant activation (an integer
    code has one zero: where the fake-quant value is -0.0 the product is +0.0). Dynamic per_token: one scale per row. Static
    per_tensor: `input_scale` is used as given, as the 0-dim operand the fake-quant route sees."""
    _ffi.require_gpu(x, input_scale)
    q = _quantizer(act_cfg)
    static = bool(q.kwargs.get('static', input_scale is not None))
    mode = act_mode({'quant_type': 'int-quant', 'bit': q.bit, 'symmetric': q.sym, 'granularity': q.granularity, 'static': static})
    x2 = x.reshape(-1, x.shape[-1])
    if mode == 'static_per_tensor':
        if input_scale is None or input_scale.numel() != 1:
            raise ValueError('i8_act_quant: static per_tensor activations need the calibrated input_scale (one element), got '
                             f'{None if input_scale is None else tuple(input_scale.shape)}')
        codes, scales, _ = q.real_quant_weight_static(x2, {'scales': input_scale.reshape(()), 'zeros': torch.tensor(0.0),
                                                           'qmax': q.qmax, 'qmin': q.qmin})
        scales = scales.reshape(1)
    else:
        codes, scales, _ = q.real_quant_weight_dynamic(x2)
        scales = scales.reshape(*x.shape[:-1], 1)
    return codes.reshape(x.shape), scales.float()           # widening a 16-bit scale is exact


def _check_gemm(a8, a_s, w8, w_s, dtype, bias, rung):
    """scaled8_ops.check_gemm and the rung's name and row limit; returns (M, N, K)."""
    M, N, K = scaled8_ops.check_gemm('i8_scaled_gemm', (torch.int8,), 'int8 codes', a8, a_s, w8, w_s, dtype, bias)
    if rung is not None and rung not in RUNGS:
        raise ValueError(f'i8_scaled_gemm: rung is one of {sorted(RUNGS)} or None, got {rung!r}')
    if rung in ('decode', 'decode_split') and M > DECODE_MAX_M:
        raise ValueError(f'i8_scaled_gemm: the {rung} rung takes at most {DECODE_MAX_M} tokens, got {M}')
    return M, N, K


def i8_scaled_gemm(a8, a_s, w8, w_s, dtype=torch.bfloat16, bias=None, rung=None):
    """c[..., N] = rnd(((a8 . w8^T) * a_s) * w_s) (+ bias in `dtype`): a8 [..., K] and w8 [N, K] int8 codes, a_s one scale per
    token or one, w_s one per output channel or one; exact int32 accumulation, converted to fp32 (round to nearest even), the two
    scale products in this order, one rounding. K % 16 == 0 and K <= 65536 (else NotImplementedError: i8_linear_forward has the
    fallback). rung: None (the library's table), or 'decode' / 'tile128' / 'decode_split' to name the launch rung (tools, tests).
    The workspace of the decode_split rung is allocated here, from the library's query."""
    M, N, K = _check_gemm(a8, a_s, w8, w_s, dtype, bias, rung)
    _ffi.require_gpu(a8, a_s, w8, w_s, bias)
    L = _ffi.lib()
    a8, w8 = a8.contiguous(), w8.contiguous()
    a_s, w_s = a_s.reshape(-1).float().contiguous(), w_s.reshape(-1).float().contiguous()
    c = torch.empty(*a8.shape[:-1], N, dtype=dtype, device=a8.device)
    if bias is not None:
        bias = bias.reshape(-1).to(dtype).contiguous()
    r = L.llmc_i8_scaled_gemm_rung(M, N, K) if rung is None else RUNGS[rung]
    nbytes = L.llmc_i8_scaled_gemm_ws_bytes(M, N, K) if r == RUNGS['decode_split'] else 0
    ws = _ffi.workspace(nbytes, a8.device)
    _ffi.check(L.llmc_i8_scaled_gemm_on_rung(_ffi.ptr(a8), _ffi.ptr(a_s), a_s.numel(), _ffi.ptr(w8), _ffi.ptr(w_s), w_s.numel(), M, N, K,
                                             _ffi.dt(dtype), _ffi.ptr(bias), _ffi.ptr(c), _ffi.ptr(ws), nbytes, -1 if rung is None else r,
                                             _ffi.stream()), 'llmc_i8_scaled_gemm')
    return c


i8_dequant = scaled8_ops.dequant


def i8_linear_forward(x, w8, w_s, act_cfg, input_scale, bias):
    """scaled8_ops.linear_forward on i8_act_quant and i8_scaled_gemm; the GEMM does not take K % 16 != 0 or K > 65536."""
    return scaled8_ops.linear_forward('i8_linear', i8_act_quant, i8_scaled_gemm, i8_dequant, x, w8, w_s, act_cfg, input_scale, bias)
