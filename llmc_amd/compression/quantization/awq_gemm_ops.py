"""The W4A16 Linear on AutoAWQ's GEMM layout (csrc/awq_gemm.hip): the consumers of the stored form deploy('autoawq_quant') writes —
qweight int32 [K, R/8], qzeros int32 [K/g, R/8], scales f16 [K/g, R], nibble order 0,2,4,6,1,3,5,7 (module_utils.pack_awq_gemm).
W~[k][n] = rnd((code - zero) * scale), one rounding to the activation dtype; y = x . W~ (+ bias) with fp32 accumulation and one
rounding. An extension: the reference's AutoawqRealQuantLinear raises in forward."""
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
