"""The W4A16 Linear on AutoAWQ's GEMM layout (csrc/awq_gemm.hip): the consumers of the stored form deploy('autoawq_quant') writes —
qweight int32 [K, R/8], qzeros int32 [K/g, R/8], scales f16 [K/g, R], nibble order 0,2,4,6,1,3,5,7 (module_utils.pack_awq_gemm).
W~[k][n] = rnd((code - zero) * scale), one rounding to the activation dtype; y = x . W~ (+ bias) with fp32 accumulation and one
rounding. An extension: the reference's AutoawqRealQuantLinear raises in forward.
The W4A8 forward of the same stored form (csrc/awq_i8_gemm.hip) is here too: awq_i8_gemm multiplies the packed nibbles by int8
activation codes on the int8 MFMA with one fp32 fma per group, awq_i8_linear_forward quantizes the activation first."""
import math

import torch

from llmc_amd import _ffi

from .fp8_linear_ops import _announce

RUNGS = {'stream': 0, 'tile': 1}            # llmc_awq_gemm's launch rungs (include/llmc_hip.h)

# Which way a product of M tokens by R output columns goes: the first row (max tokens, min columns, way) whose bounds hold.
# 'stream' and 'tile' are the fused kernel's rungs, 'dequant' is awq_dequant + hip_linear (the 16-bit GEMM on the unpacked weight).
# Set from tools/bench_awq_gemm.py (profiles/awq_gemm.txt, f16 and bf16): no measured shape goes to a rung that loses to 'dequant'
# with the min..max ranges apart. Up to 64 tokens the stream rung is 1.7 to 8 times faster than 'dequant' on every shape; at 256 it
# loses at R = 4096 and 6144. The tile rung wins only where there are many strips (R = 28672: 3.1 x at 256 tokens, 1.2 to 1.4 x at
# 1024) and loses at 4096 tokens everywhere; between 65 and 255 tokens nothing is measured, so nothing is claimed.
LADDER = (
    (64, 0, 'stream'),
    (1024, 28672, 'tile'),
    (math.inf, 0, 'dequant'),
)

I8_RUNGS = {'stream': 0, 'tile': 1}         # llmc_awq_i8_gemm_on_rung's launch rungs (csrc/awq_i8_gemm.hip)

# The W4A8 forward's way for M tokens: the first row (max tokens, min depth K, max columns R, way) whose bounds hold. 'stream' and
# 'tile' are the int8-MFMA kernel's rungs, 'w4a16' is i8_dequant of the activation codes + awq_linear_forward (the parent's path on
# the same codes). Set from tools/bench_awq_i8.py (profiles/awq_i8_gemm.txt; bf16, g = 128, the four Llama-3-8B shapes at 1, 16, 64,
# 256, 1024 and 4096 tokens): no measured shape goes to a rung that loses to 'w4a16' with the min..max ranges apart. Up to 16
# tokens the stream rung wins on every shape (1.03 to 1.7 x); at 64 it wins up to R = 6144 (1.4 x) and both rungs lose at R = 28672.
# At 256 tokens the tile rung wins at K = 4096 (1.03 to 1.6 x) but starves on the deep narrow shape (K = 14336, R = 4096: 32
# workgroups), where the stream rung wins (1.6 x); that shape's tile rung wins again at 1024 tokens, and between the two nothing is
# measured. At 1024 tokens the tile rung wins everywhere (1.1 to 1.7 x), at 4096 up to R = 6144 and on the deep shape (1.4 x), and
# loses at R = 28672 (0.9 x). Past 4096 tokens nothing is measured, so nothing is claimed.
I8_LADDER = (
    (16, 0, math.inf, 'stream'),
    (64, 0, 6144, 'stream'),
    (64, 0, math.inf, 'w4a16'),
    (256, 14336, 4096, 'stream'),
    (1023, 14336, 4096, 'w4a16'),
    (1024, 0, math.inf, 'tile'),
    (4096, 0, 6144, 'tile'),
    (math.inf, 0, math.inf, 'w4a16'),
)

_SHIFTS = (0, 16, 4, 20, 8, 24, 12, 28)     # 4 * INV[j]: column 8 c + j of word c sits in nibble INV[j] = 0,4,1,5,2,6,3,7


def route(M, K, R):
    """The LADDER's answer for M tokens; a depth the tile rung does not take (K % 64 != 0) goes to 'dequant'."""
    way = next(w for max_m, min_r, w in LADDER if M <= max_m and R >= min_r)
    return 'dequant' if way == 'tile' and K % 64 else way


def _unpack(words):
    """int32 [..., C] -> the nibbles as stored, int32 [..., 8 C] in column order."""
    sh = torch.tensor(_SHIFTS, dtype=torch.int32, device=words.device)
    return ((words.unsqueeze(-1) >> sh) & 15).reshape(*words.shape[:-1], -1)


def awq_dequant_composed(qweight, qzeros, scales, group_size, dtype):
    """W~ transposed, [R, K] in `dtype`, from torch ops on any device: the arithmetic llmc_awq_dequant and the GEMM state
    (fp32 product of the exact integer difference and the widened scale, one rounding)."""
    d = _unpack(qweight) - _unpack(qzeros).repeat_interleave(group_size, 0)
    return (d.float() * scales.float().repeat_interleave(group_size, 0)).to(dtype).t().contiguous()


def _check(qweight, qzeros, scales, group_size):
    """Shapes and dtypes of the stored form; returns (K, R). Raises before anything touches the GPU."""
    if qweight.dtype != torch.int32 or qzeros.dtype != torch.int32 or scales.dtype != torch.float16:
        raise TypeError(f'awq: qweight and qzeros are int32 and scales f16, got {qweight.dtype}, {qzeros.dtype}, {scales.dtype}')
    if qweight.dim() != 2 or group_size < 1 or qweight.shape[0] % group_size:
        raise ValueError(f'awq: qweight is [K, R/8] with K a multiple of the group size, got {tuple(qweight.shape)}, g = {group_size}')
    K, R = qweight.shape[0], qweight.shape[1] * 8
    if tuple(qzeros.shape) != (K // group_size, R // 8) or tuple(scales.shape) != (K // group_size, R):
        raise ValueError(f'awq: qzeros is [K/g, R/8] and scales [K/g, R], got {tuple(qzeros.shape)} and {tuple(scales.shape)} '
                         f'for K, R, g = {K}, {R}, {group_size}')
    return K, R


def awq_dequant(qweight, qzeros, scales, group_size, dtype):
    """W~ transposed, [R, K] in f16, bf16 or fp32 — the layout hip_linear takes — by the streaming kernel. A group size that is
    no multiple of 8 (NotImplementedError from the library) is composed from torch ops: the same bits."""
    K, R = _check(qweight, qzeros, scales, group_size)
    _ffi.require_gpu(qweight, qzeros, scales)
    qweight, qzeros, scales = qweight.contiguous(), qzeros.contiguous(), scales.contiguous()
    out = torch.empty(R, K, dtype=dtype, device=qweight.device)
    try:
        _ffi.check(_ffi.lib().llmc_awq_dequant(_ffi.ptr(qweight), _ffi.ptr(qzeros), _ffi.ptr(scales), K, R, group_size, _ffi.ptr(out),
                                               _ffi.dt(dtype), _ffi.stream()), 'llmc_awq_dequant')
    except NotImplementedError as e:
        _announce('awq_dequant', (K, R, group_size), str(e), 'the unpack from torch ops on the GPU')
        return awq_dequant_composed(qweight, qzeros, scales, group_size, dtype)
    return out


def awq_gemm(x, qweight, qzeros, scales, group_size, bias=None, rung=None):
    """y[..., R] = rnd(x[..., K] . W~ (+ bias)): x f16 or bf16, fp32 accumulation on the MFMA, the bias added to the fp32 sum,
    one rounding. rung: None (the LADDER's kernel rung for this many tokens), or 'stream' / 'tile' by name (tools, tests).
    NotImplementedError: a shape the kernel refuses (group size no multiple of 16, ...); awq_linear_forward has the fallback."""
    K, R = _check(qweight, qzeros, scales, group_size)
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise NotImplementedError(f'awq_gemm: activations are f16 or bf16, got {x.dtype}')
    if x.shape[-1] != K:
        raise ValueError(f'awq_gemm: activation and weight disagree on K ({x.shape[-1]} and {K})')
    if bias is not None and bias.numel() != R:
        raise ValueError(f'awq_gemm: the bias holds {R} elements, got {bias.numel()}')
    _ffi.require_gpu(x, qweight, qzeros, scales, bias)
    M = x.numel() // K
    if M < 1:
        raise ValueError('awq_gemm: empty activation')
    if rung is None:
        rung = route(M, K, R)
        if rung == 'dequant':       # where the LADDER prefers the unpacked weight, the kernel for many tokens
            rung = 'stream' if K % 64 else 'tile'
    x, qweight, qzeros, scales = x.contiguous(), qweight.contiguous(), qzeros.contiguous(), scales.contiguous()
    if bias is not None:
        bias = bias.reshape(-1).to(x.dtype).contiguous()
    y = torch.empty(*x.shape[:-1], R, dtype=x.dtype, device=x.device)
    L = _ffi.lib()
    ws = _ffi.workspace(L.llmc_awq_gemm_ws_bytes(M, K, R), x.device) if rung == 'stream' else None
    _ffi.check(L.llmc_awq_gemm(_ffi.ptr(x), _ffi.dt(x), M, K, R, _ffi.ptr(qweight), _ffi.ptr(qzeros), _ffi.ptr(scales), group_size,
                               _ffi.ptr(bias), _ffi.ptr(y), _ffi.ptr(ws), _ffi.stream(), RUNGS[rung]), 'llmc_awq_gemm')
    return y


def stream_slices(M, K, R):
    """How many K slices the stream rung adds up for this shape (a pure host call: the workspace holds one fp32 [M, R] each)."""
    return _ffi.lib().llmc_awq_gemm_ws_bytes(M, K, R) // (4 * M * R)


def awq_linear_forward(x, qweight, qzeros, scales, group_size, bias=None):
    """The Linear's forward: the LADDER's way for this many tokens. A shape or dtype the fused kernel refuses goes, said once per
    shape on stderr, through awq_dequant + hip_linear: the 16-bit HIP GEMM on the unpacked weight."""
    from .module_utils import hip_linear
    K, R = qweight.shape[0], qweight.shape[1] * 8
    way = route(x.numel() // max(K, 1), K, R)
    if way != 'dequant':
        try:
            return awq_gemm(x, qweight, qzeros, scales, group_size, bias, rung=way)
        except NotImplementedError as e:          # LLMC_ENOTSUP: nothing was launched
            _announce('awq_linear', (tuple(x.shape), tuple(qweight.shape), group_size, str(x.dtype)), str(e),
                      'the de-quantized weight through the 16-bit HIP GEMM')
    return hip_linear(x, awq_dequant(qweight, qzeros, scales, group_size, x.dtype), bias)


def i8_route(M, K, R):
    """The I8_LADDER's answer for M tokens on a [K, R] weight."""
    return next(w for max_m, min_k, max_r, w in I8_LADDER if M <= max_m and K >= min_k and R <= max_r)


def awq_i8_gemm(a8, a_s, qweight, qzeros, scales, group_size, dtype=torch.bfloat16, bias=None, rung=None):
    """y[..., R] = rnd(a_s * sum_g scales[g] * (a8 . (code - zero))_g (+ bias)): a8 [..., K] int8 codes, a_s one scale per token or
    one; a group's integer sum is exact on the int8 MFMA, one fp32 fma per group, the activation scale and the bias in fp32, one
    rounding to `dtype` (f16 or bf16). rung: None (the library's ladder), or 'stream' / 'tile' by name (tools, tests).
    NotImplementedError: a shape the kernel refuses (group size no multiple of 32, ...); awq_i8_linear_forward has the fallback."""
    K, R = _check(qweight, qzeros, scales, group_size)
    if a8.dtype != torch.int8:
        raise TypeError(f'awq_i8_gemm: a8 holds int8 codes, got {a8.dtype}')
    if a8.dim() < 1 or a8.shape[-1] != K:
        raise ValueError(f'awq_i8_gemm: activation and weight disagree on K ({tuple(a8.shape)[-1:]} and {K})')
    M = a8.numel() // K
    if M < 1:
        raise ValueError('awq_i8_gemm: empty activation')
    if a_s.numel() not in (1, M):
        raise ValueError(f'awq_i8_gemm: a_s holds one scale per token ({M}) or one, got {a_s.numel()}')
    if a_s.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f'awq_i8_gemm: a_s is fp32, fp16 or bf16, got {a_s.dtype}')
    if dtype not in (torch.float16, torch.bfloat16):
        raise TypeError(f'awq_i8_gemm: the output is fp16 or bf16, got {dtype}')
    if bias is not None and bias.numel() != R:
        raise ValueError(f'awq_i8_gemm: the bias holds {R} elements, got {bias.numel()}')
    if rung is not None and rung not in I8_RUNGS:
        raise ValueError(f'awq_i8_gemm: rung is one of {sorted(I8_RUNGS)} or None, got {rung!r}')
    _ffi.require_gpu(a8, a_s, qweight, qzeros, scales, bias)
    L = _ffi.lib()
    a8, qweight, qzeros, scales = a8.contiguous(), qweight.contiguous(), qzeros.contiguous(), scales.contiguous()
    a_s = a_s.reshape(-1).float().contiguous()
    if bias is not None:
        bias = bias.reshape(-1).to(dtype).contiguous()
    y = torch.empty(*a8.shape[:-1], R, dtype=dtype, device=a8.device)
    r = L.llmc_awq_i8_gemm_rung(M, K, R) if rung is None else I8_RUNGS[rung]
    nbytes = L.llmc_awq_i8_gemm_ws_bytes(M, K, R, group_size) if r == I8_RUNGS['stream'] else 0
    ws = _ffi.workspace(nbytes, a8.device)
    _ffi.check(L.llmc_awq_i8_gemm_on_rung(_ffi.ptr(a8), _ffi.ptr(a_s), a_s.numel(), M, K, R, _ffi.ptr(qweight), _ffi.ptr(qzeros),
                                          _ffi.ptr(scales), group_size, _ffi.dt(dtype), _ffi.ptr(bias), _ffi.ptr(y), _ffi.ptr(ws), nbytes,
                                          r, _ffi.stream()), 'llmc_awq_i8_gemm')
    return y


def awq_i8_linear_forward(x, qweight, qzeros, scales, group_size, act_cfg, input_scale=None, bias=None):
    """The W4A8 Linear's forward: the activation quantized to int8 by the IntegerQuantizer `act_cfg` describes
    (i8_linear_ops.i8_act_quant: dynamic per token, or static per tensor with `input_scale`), then the I8_LADDER's way for this many
    tokens. 'w4a16', and a shape the int8 kernel refuses (said once per shape on stderr), go through the de-quantized codes and
    awq_linear_forward: the W4A16 path on the fake-quantized activation."""
    from .i8_linear_ops import i8_act_quant, i8_dequant
    codes, a_s = i8_act_quant(x.contiguous(), act_cfg, input_scale)
    K, R = qweight.shape[0], qweight.shape[1] * 8
    way = i8_route(x.numel() // max(K, 1), K, R)
    if way != 'w4a16':
        try:
            return awq_i8_gemm(codes, a_s, qweight, qzeros, scales, group_size, dtype=x.dtype, bias=bias, rung=way)
        except NotImplementedError as e:          # LLMC_ENOTSUP: nothing was launched
            _announce('awq_i8_linear', (tuple(x.shape), tuple(qweight.shape), group_size, str(x.dtype)), str(e),
                      'the de-quantized activation codes through the W4A16 path')
    return awq_linear_forward(i8_dequant(codes, a_s, x.dtype), qweight, qzeros, scales, group_size, bias)
