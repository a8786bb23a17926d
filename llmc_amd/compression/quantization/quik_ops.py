"""The QUIK real-quant Linear on gfx950's matrix instructions (csrc/quik_gemm.hip): the consumers of the stored form that
deploy('quik_quant') writes (module_utils.QuikRealQuantLinear) — the integer input channels as int8 codes [N, Ki] with one
fp32 scale per output channel, the outlier input channels in 16 bit [N, Fp]. A forward is two kernels: quik_act_split (one pass
over the activation: permute, per-token absmax over the integer channels, int8 codes, the outliers' own bits) and quik_gemm
(int8 MFMAs over Ki, the int32 accumulators scaled in place, 16-bit MFMAs over Fp on top). An extension: the reference has
QUIK's fake-quant method only."""
import torch

from llmc_amd import _ffi

from .scaled8_ops import _FALLBACK_SEEN, _announce          # noqa: F401  (the tests take them here)

RUNGS = {'decode': 0, 'tile128': 1}                            # llmc_quik_gemm's launch rungs (include/llmc_hip.h)
DECODE_MAX_M = 64
MAX_KI, MAX_FP = 65536, 32768


def padded(n_int, F):
    """(Ki, Fp): the integer channels rounded up to 64 codes, the outlier channels to 32 elements."""
    return -(-n_int // 64) * 64, -(-F // 32) * 32


def act_split_fits(x, Ki, Fp):
    """Whether the split kernel takes x's rows (bf16 / fp16, K % 8 == 0, the permuted row in the LDS of a CU): a host call."""
    if x.dtype not in (torch.bfloat16, torch.float16):
        return False
    return bool(_ffi.lib().llmc_quik_act_split_fits(_ffi.dt(x), x.shape[-1], Ki, Fp))


def quik_act_split(x, col_map, Ki, Fp):
    """x [..., K] bf16 / fp16 -> (codes int8 [..., Ki], scales fp32 [..., 1], outliers [..., Fp] in x's dtype). col_map int32 [K]
    sends source column c to integer slot col_map[c] < Ki or to outlier slot col_map[c] - Ki. Codes and scales are bit for bit
    IntegerQuantizer(8, True, 'per_token').real_quant_weight_dynamic on the gathered integer columns; padding slots are 0."""
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f'quik_act_split: x is bf16 or fp16, got {x.dtype}')
    if col_map.dtype != torch.int32 or col_map.dim() != 1 or col_map.numel() != x.shape[-1]:
        raise ValueError(f'quik_act_split: col_map is int32 [K = {x.shape[-1]}], got {col_map.dtype} {tuple(col_map.shape)}')
    K = x.shape[-1]
    if Ki < 64 or Ki % 64 or Fp < 0 or Fp % 32 or not (Ki + Fp - 94 <= K <= Ki + Fp):
        raise ValueError(f'quik_act_split: Ki is the integer columns rounded up to 64 and Fp the outlier columns rounded up to 32 '
                         f'(K = {K}), got Ki = {Ki}, Fp = {Fp}')
    _ffi.require_gpu(x, col_map)
    x = x.contiguous()
    M = x.numel() // K
    codes = torch.empty(*x.shape[:-1], Ki, dtype=torch.int8, device=x.device)
    scales = torch.empty(*x.shape[:-1], 1, dtype=torch.float32, device=x.device)
    a_fp = torch.empty(*x.shape[:-1], Fp, dtype=x.dtype, device=x.device)
    _ffi.check(_ffi.lib().llmc_quik_act_split(_ffi.ptr(x), _ffi.dt(x), M, K, _ffi.ptr(col_map.contiguous()), Ki, Fp, _ffi.ptr(codes),
                                              _ffi.ptr(scales), _ffi.ptr(a_fp) if Fp else 0, _ffi.stream()), 'llmc_quik_act_split')
    return codes, scales, a_fp


def _check_gemm(a8, a_s, a_fp, w8, w_s, w_fp, dtype, bias, rung):
    """Shapes and dtypes of a quik_gemm call, before anything touches the GPU; returns (M, N, Ki, Fp)."""
    for arg, t in (('a8', a8), ('w8', w8)):
        if t.dtype != torch.int8:
            raise TypeError(f'quik_gemm: {arg} holds int8 codes, got {t.dtype}')
    if w8.dim() != 2 or w_fp.dim() != 2 or a8.dim() < 1 or w_fp.shape[0] != w8.shape[0]:
        raise ValueError(f'quik_gemm: the weights are [N, Ki] and [N, Fp], got {tuple(w8.shape)} and {tuple(w_fp.shape)}')
    (N, Ki), Fp = w8.shape, w_fp.shape[1]
    if a8.shape[-1] != Ki or a_fp.shape[-1] != Fp or a_fp.shape[:-1] != a8.shape[:-1]:
        raise ValueError(f'quik_gemm: the activation parts are [..., {Ki}] and [..., {Fp}] with the same leading shape, got '
                         f'{tuple(a8.shape)} and {tuple(a_fp.shape)}')
    if a_fp.dtype not in (torch.bfloat16, torch.float16) or w_fp.dtype != a_fp.dtype:
        raise TypeError(f'quik_gemm: the outlier parts are both bf16 or both fp16, got {a_fp.dtype} and {w_fp.dtype}')
    M = a8.numel() // max(Ki, 1)
    if M < 1 or N < 1 or Ki < 1:
        raise ValueError(f'quik_gemm: empty operand (M, N, Ki = {M}, {N}, {Ki})')
    if a_s.numel() != M or w_s.numel() != N:
        raise ValueError(f'quik_gemm: a_s holds one scale per token ({M}) and w_s one per output channel ({N}), got '
                         f'{a_s.numel()} and {w_s.numel()}')
    if dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f'quik_gemm: the output is fp32, fp16 or bf16, got {dtype}')
    if bias is not None and bias.numel() != N:
        raise ValueError(f'quik_gemm: the bias holds {N} elements, got {bias.numel()}')
    if rung is not None and rung not in RUNGS:
        raise ValueError(f'quik_gemm: rung is one of {sorted(RUNGS)} or None, got {rung!r}')
    if rung == 'decode' and M > DECODE_MAX_M:
        raise ValueError(f'quik_gemm: the decode rung takes at most {DECODE_MAX_M} tokens, got {M}')
    return M, N, Ki, Fp


def quik_gemm(a8, a_s, a_fp, w8, w_s, w_fp, dtype=torch.bfloat16, bias=None, rung=None):
    """c[..., N] = rnd(((a8 . w8^T) * a_s) * w_s + a_fp . w_fp^T) (+ bias in `dtype`): exact int32 accumulation over Ki, converted
    to fp32 and scaled, then the 16-bit products accumulated in fp32 on top, one rounding. Ki % 64 == 0, Fp % 32 == 0 (Fp = 0: no
    outliers), Ki <= 65536 (else NotImplementedError). rung: None (the library's table), 'decode' or 'tile128'."""
    M, N, Ki, Fp = _check_gemm(a8, a_s, a_fp, w8, w_s, w_fp, dtype, bias, rung)
    _ffi.require_gpu(a8, a_s, a_fp, w8, w_s, w_fp, bias)
    a8, w8, a_fp, w_fp = a8.contiguous(), w8.contiguous(), a_fp.contiguous(), w_fp.contiguous()
    a_s, w_s = a_s.reshape(-1).float().contiguous(), w_s.reshape(-1).float().contiguous()
    c = torch.empty(*a8.shape[:-1], N, dtype=dtype, device=a8.device)
    if bias is not None:
        bias = bias.reshape(-1).to(dtype).contiguous()
    _ffi.check(_ffi.lib().llmc_quik_gemm_on_rung(_ffi.ptr(a8), _ffi.ptr(a_s), _ffi.ptr(a_fp) if Fp else 0, _ffi.ptr(w8), _ffi.ptr(w_s),
                                                 _ffi.ptr(w_fp) if Fp else 0, M, N, Ki, Fp, _ffi.dt(a_fp), _ffi.dt(dtype), _ffi.ptr(bias),
                                                 _ffi.ptr(c), -1 if rung is None else RUNGS[rung], _ffi.stream()), 'llmc_quik_gemm')
    return c


def quik_linear_composed(x, module):
    """The same product from existing operators, for what the two kernels refuse (fp32 activations, rows too wide for the split):
    gather, i8_act_quant, i8_scaled_gemm into fp32, a 16-bit linear on the outliers, add, round. The outlier product is rounded
    to 16 bit before the add, which the fused kernel does not do."""
    from . import i8_linear_ops as I8
    from .module_utils import hip_linear
    Ki, Fp = module.weight.shape[1], module.weight_fp.shape[1]
    n_int, F = module.int_ids.numel(), module.fp_ids.numel()
    codes, scales = I8.i8_act_quant(x.index_select(-1, module.int_ids.long()), module.aquantizer())
    codes = torch.nn.functional.pad(codes, (0, Ki - n_int))
    y = I8.i8_scaled_gemm(codes, scales, module.weight, module.weight_scale, dtype=torch.float32)
    if F:
        xf = torch.nn.functional.pad(x.index_select(-1, module.fp_ids.long()), (0, Fp - F))
        y = y + hip_linear(xf, module.weight_fp, None).float()
    y = y.to(x.dtype)
    return y if module.bias is None else y + module.bias.to(x.dtype)


def quik_linear_forward(x, module):
    """Split, then GEMM; the output takes the activation's dtype. What the kernels do not take goes, said once per shape on stderr,
    through quik_linear_composed."""
    _ffi.require_gpu(x)
    Ki, Fp = module.weight.shape[1], module.weight_fp.shape[1]
    if x.dtype == module.weight_fp.dtype and Ki <= MAX_KI and Fp <= MAX_FP and act_split_fits(x, Ki, Fp):
        codes, scales, a_fp = quik_act_split(x, module.col_map, Ki, Fp)
        return quik_gemm(codes, scales, a_fp, module.weight, module.weight_scale, module.weight_fp, dtype=x.dtype, bias=module.bias)
    _announce('quik_linear', (tuple(x.shape), tuple(module.weight.shape), str(x.dtype)),
              f'the split kernel takes {module.weight_fp.dtype} rows with K % 8 == 0 that fit the LDS of a CU, Ki <= {MAX_KI}',
              'gather, i8_act_quant, i8_scaled_gemm, a 16-bit linear on the outliers, add')
    return quik_linear_composed(x, module)
