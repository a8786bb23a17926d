"""OCP MX operators on gfx950's block-scaled matrix instruction (csrc/mx_gemm.hip): the consumers of the stored form that
FloatQuantizer(bit='e2m1', float_semantics='ocp', scale_format='e8m0', granularity='per_group', group_size=32) writes — e2m1
codes packed two per byte + one e8m0 scale byte per 32 elements. Activations are quantized on the fly into the same form
(MXFP4) or into e4m3 codes with e8m0 block scales (MXFP8; FloatQuantizer itself does not offer that pairing). An extension:
the reference's real-quant Linears raise in forward."""
import torch

from llmc_amd import _ffi

from .quant import dequant_fpx

MX_BLOCK = 32
_FMT = {'e2m1': 2, 'e4m3': 4}


def _fmt(bit):
    if bit not in _FMT:
        raise NotImplementedError(f"MX activations are 'e2m1' or 'e4m3', got {bit!r} (e3m2 has no dense packing, e5m2 and "
                                  'static scales are not provided)')
    return _FMT[bit]


def mx_act_quant(x, bit='e2m1'):
    """x [..., K] bf16 / fp16, K % 32 == 0 -> (codes uint8 [..., K/2] for e2m1 (element 2i in the low nibble) or [..., K] for
    e4m3, scales uint8 [..., K/32] e8m0): per 1 x 32 block scale = 2^(floor(log2 absmax) - emax), element = RNE onto the OCP grid,
    saturating. e2m1 is bit for bit FloatQuantizer's real-quant route, in one pass."""
    _ffi.require_gpu(x)
    fmt = _fmt(bit)
    assert x.is_contiguous(), 'Input tensor must be contiguous'
    K = x.size(-1)
    assert K % MX_BLOCK == 0, f'Last dimension size must be divisible by the MX block ({MX_BLOCK})'
    M = x.numel() // K
    codes = torch.empty(*x.shape[:-1], K // 2 if bit == 'e2m1' else K, dtype=torch.uint8, device=x.device)
    scales = torch.empty(*x.shape[:-1], K // MX_BLOCK, dtype=torch.uint8, device=x.device)
    _ffi.check(_ffi.lib().llmc_mx_act_quant(_ffi.ptr(x), _ffi.dt(x), M, K, fmt, _ffi.ptr(codes), _ffi.ptr(scales), _ffi.stream()),
               'llmc_mx_act_quant')
    return codes, scales


def mx_dequant(codes, scales, bit, dtype):
    """The stored form back to numbers: decode(code) * 2^(scale - 127), an fp32 product rounded once to `dtype`."""
    _ffi.require_gpu(codes, scales)
    _fmt(bit)
    if bit == 'e2m1':
        out = dequant_fpx(codes.reshape(-1, codes.size(-1)), scales, 'e2m1', MX_BLOCK, dtype)
        return out.reshape(*codes.shape[:-1], codes.size(-1) * 2)
    assert codes.dtype == torch.uint8 and codes.size(-1) == scales.size(-1) * MX_BLOCK
    v = codes.view(torch.float8_e4m3fn).float().reshape(*scales.shape, MX_BLOCK)
    s = torch.ldexp(torch.ones((), device=codes.device), scales.to(torch.int32) - 127)
    return (v * s.unsqueeze(-1)).reshape(codes.shape).to(dtype)


def mx_gemm(a, a_s, a_bit, w_packed, w_s, dtype=torch.bfloat16, bias=None):
    """c[..., N] = sum over 32-deep blocks of 2^(a_s + w_s - 254) * (a_blk . w_blk^T): a [..., K/2] packed e2m1 or [..., K] e4m3
    codes with a_s [..., K/32]; w_packed [N, K/2] packed e2m1 with w_s [N, K/32]; K % 128 == 0. fp32 accumulation inside the
    block-scaled MFMA, one rounding to `dtype`, then the bias in `dtype`."""
    _ffi.require_gpu(a, a_s, w_packed, w_s, bias)
    fmt = _fmt(a_bit)
    assert a.is_contiguous() and w_packed.is_contiguous(), 'Input tensors must be contiguous'
    assert a_s.is_contiguous() and w_s.is_contiguous(), 'Scaling factor tensors must be contiguous'
    assert a.dtype == torch.uint8 and w_packed.dtype == torch.uint8 and a_s.dtype == torch.uint8 and w_s.dtype == torch.uint8
    N, K = w_packed.size(0), w_packed.size(1) * 2
    assert a.size(-1) == (K // 2 if a_bit == 'e2m1' else K), 'activation and weight disagree on K'
    assert a_s.size(-1) == K // MX_BLOCK and tuple(w_s.shape) == (N, K // MX_BLOCK), 'one scale byte per 32 elements'
    M = a.numel() // a.size(-1)
    c = torch.empty(*a.shape[:-1], N, dtype=dtype, device=a.device)
    if bias is not None:
        bias = bias.to(dtype).contiguous()
    _ffi.check(_ffi.lib().llmc_mx_gemm(_ffi.ptr(a), fmt, _ffi.ptr(a_s), _ffi.ptr(w_packed), _ffi.ptr(w_s), M, N, K, _ffi.dt(dtype),
                                       _ffi.ptr(bias), _ffi.ptr(c), _ffi.stream()), 'llmc_mx_gemm')
    return c


def mx_linear_forward(x, w_packed, w_s, act_bit, bias):
    """Quantize the activation per 1 x 32 block, multiply by the MXFP4 weight; the output takes the activation's dtype."""
    codes, scales = mx_act_quant(x.contiguous(), act_bit)
    return mx_gemm(codes, scales, act_bit, w_packed, w_s, dtype=x.dtype, bias=bias)
