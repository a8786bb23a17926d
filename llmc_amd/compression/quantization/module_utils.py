"""Linear wrappers with llmc's `Cls.new(module, **params)` protocol (llmc/compression/quantization/
module_utils.py:586-1065). Buffers named `buf_*` carry qparams between phases exactly like the reference
(module_utils.py:597-602). Packing runs on the GPU (the reference round-trips through numpy on the host,
module_utils.py:846-860, or loops over columns in Python, :1018-1046)."""
from functools import partial

import torch
import torch.nn as nn

from .quant import pack_awq_gemm, pack_lsb


def hip_linear(x, weight, bias):
    """y = x W^T + b for the fake-quant wrappers (module_utils.py:619-644, 706-741): the HIP MFMA GEMMs
    (awq_ops.linear_auto: the k-tiled one-wave-per-SIMD kernel whenever K % 128 == 0 — a product with fewer 256 x 256 output
    tiles than CUs, e.g. an evaluation forward of 1 x 2048 tokens through a 4096-wide layer = 128 tiles, is cut into k-slices
    so that tiles x slices fills the chip, fp32 partials summed and rounded once; the row-major kernel for K % 64 == 0; fp32
    accumulation, one rounding). Round 5: no product of a supported shape goes to the vendor GEMM any more."""
    from llmc_amd import _ffi

    from . import awq_ops
    _ffi.require_gpu(x, weight)
    if weight.dtype != x.dtype:
        weight = weight.to(x.dtype)
    return awq_ops.linear_auto(x, weight, bias)


def _func_name(f):
    return f.func.__name__ if isinstance(f, partial) else f.__name__


def _copy_buf(dst, src):
    for name, buf in src.named_buffers():
        if name.startswith('buf_'):
            dst.register_buffer(name, buf.data)
    for name, p in src.named_parameters():
        if name.startswith('buf_'):
            dst.register_buffer(name, p.data)


def _keep_rotater(dst, ori_module):
    """module_utils.py:408-411, 604-607, 694-697 of the reference: a wrapper of a RotateLinear (its `buf_rotate` buffer came
    over with _copy_buf) keeps that module's rotater and rotates its input first; any other wrapper has buf_rotate = False.
    (A copied buffer of that name cannot be overwritten by a plain attribute, hence the order.)"""
    if bool(getattr(dst, 'buf_rotate', False)):
        dst.rotater = ori_module.rotater
    else:
        dst.buf_rotate = False
        dst.rotater = None


class LlmcRMSNorm(nn.Module):
    """module_utils.py:321-345: RMSNorm without a scale (QuaRot fuses the scale into the following Linears; `weight` is kept as
    ones so that the module still looks like a norm)."""

    def __init__(self, weight, eps=1e-6):
        super().__init__()
        self.variance_epsilon = eps
        self.weight = nn.Parameter(torch.ones_like(weight))

    def forward(self, hidden_states):
        input_dtype = hidden_states.dtype
        variance = hidden_states.to(torch.float32).pow(2).mean(-1, keepdim=True)
        hidden_states = hidden_states * torch.rsqrt(variance + self.variance_epsilon)
        return hidden_states.to(input_dtype)

    @classmethod
    @torch.no_grad()
    def new(cls, module):
        eps = module.eps if hasattr(module, 'eps') else module.variance_epsilon
        return cls(module.weight, eps)

    def __repr__(self):
        return 'LlmcRMSNorm()'


class Rotater:
    """module_utils.py:460-503: the online Hadamard transform in front of down_proj (full: along the row, K / had_K the factor
    of the intermediate size) and o_proj (partial: across the heads, [tokens, num_heads, had_dim] with the heads in the middle)
    on llmc_hadamard. `fp32_had` decides the dtype handed to the kernel. One difference from the reference: with fp32_had False
    and K > 1 it rounds to 16 bits between the fast transform and the had_K product; this rounds once, at the end (the kernel
    accumulates in fp32 either way)."""

    def __init__(self, online_full_had, online_partial_had, fp32_had, K, had_K=None, had_dim=None):
        self.online_full_had = online_full_had
        self.online_partial_had = online_partial_had
        self.fp32_had = fp32_had
        self.K = K
        self.had_K = had_K
        self.had_dim = had_dim

    def rotate(self, x):
        import math

        from .hadamard_utils import hadamard_transform, matmul_hadU_cuda
        x_dtype = x.dtype
        if self.K > 1 and self.had_K.device != x.device:
            self.had_K = self.had_K.to(x.device)
        if self.online_full_had:
            if self.fp32_had:
                x = matmul_hadU_cuda(x.float(), self.had_K, self.K).to(x_dtype)
            else:
                x = matmul_hadU_cuda(x, self.had_K, self.K)
        elif self.online_partial_had:
            if self.fp32_had:
                x = x.float()
            heads = x.shape[-1] // self.had_dim
            x = hadamard_transform(x, heads, self.had_dim, self.had_K, self.K, 1 / math.sqrt(heads))
            if self.fp32_had:
                x = x.to(x_dtype)
        return x


class RotateLinear(nn.Module):
    """module_utils.py:506-583: rotate the input, then the product (hip_linear)."""

    def __init__(self, weight, bias, ori_module, online_full_had, online_partial_had, fp32_had, K, had_K, had_dim):
        super().__init__()
        self.register_buffer('weight', weight)
        if bias is not None:
            self.register_buffer('bias', bias)
        else:
            self.bias = None
        _copy_buf(self, ori_module)
        self.rotater = Rotater(online_full_had, online_partial_had, fp32_had, K, had_K, had_dim)
        self.register_buffer('buf_rotate', torch.tensor(True))

    def forward(self, x):
        return hip_linear(self.rotater.rotate(x), self.weight, self.bias)

    @classmethod
    @torch.no_grad()
    def new(cls, module, online_full_had, online_partial_had, fp32_had, K, had_K, had_dim):
        bias = module.bias.data if module.bias is not None else None
        m = cls(module.weight.data, bias, ori_module=module, online_full_had=online_full_had,
                online_partial_had=online_partial_had, fp32_had=fp32_had, K=K, had_K=had_K, had_dim=had_dim)
        m.in_features, m.out_features = module.in_features, module.out_features
        return m

    @classmethod
    def get_func_name(cls, any_callable):
        return _func_name(any_callable)

    def register_activation_parameters(self, named_parameters):
        pass

    def __repr__(self):
        return (f'RotateLinear(in_features={self.in_features},out_features={self.out_features},'
                f'bias={self.bias is not None},online_rotate={self.buf_rotate})')


class OriginFloatLinear(nn.Module):
    """module_utils.py OriginFloatLinear: plain float forward, keeps buf_* (used by deploy('origin_float'))."""

    def __init__(self, weight, bias, ori_module):
        super().__init__()
        self.register_buffer('weight', weight)
        if bias is not None:
            self.register_buffer('bias', bias)
        else:
            self.bias = None
        _copy_buf(self, ori_module)
        _keep_rotater(self, ori_module)

    @torch.no_grad()
    def forward(self, x):
        if self.rotater is not None:
            x = self.rotater.rotate(x)
        return hip_linear(x, self.weight, self.bias)

    @classmethod
    @torch.no_grad()
    def new(cls, module):
        bias = module.bias.data if getattr(module, 'bias', None) is not None else None
        m = cls(module.weight.data, bias, module)
        m.in_features, m.out_features = module.in_features, module.out_features
        return m


class FakeQuantLinear(nn.Module):
    """module_utils.py:586-678: quantizes the weight lazily on first forward with w_qdq, activations with a_qdq."""

    def __init__(self, weight, bias, ori_module, w_qdq, a_qdq):
        super().__init__()
        self.register_buffer('weight', weight)
        if bias is not None:
            self.register_buffer('bias', bias)
        else:
            self.bias = None
        self.a_qdq = a_qdq
        self.w_qdq = w_qdq
        _copy_buf(self, ori_module)
        _keep_rotater(self, ori_module)
        self.dynamic_quant_weight = False
        self.dynamic_quant_tmp_weight = False

    def forward(self, x):
        if self.rotater is not None:
            x = self.rotater.rotate(x)
        if self.a_qdq is not None:
            x = self.a_qdq(x, self)
        if not hasattr(self, 'tmp_weight'):
            self.register_buffer('tmp_weight', self.w_qdq(self), persistent=False)
            self.tmp_bias = self.bias
        elif self.dynamic_quant_weight or self.dynamic_quant_tmp_weight:
            self.tmp_weight = self.w_qdq(self)
            self.tmp_bias = self.bias
        return hip_linear(x, self.tmp_weight, self.tmp_bias)

    @classmethod
    @torch.no_grad()
    def new(cls, module, w_qdq, a_qdq):
        bias = module.bias.data if getattr(module, 'bias', None) is not None else None
        m = cls(module.weight.data, bias, ori_module=module, w_qdq=w_qdq, a_qdq=a_qdq)
        m.in_features, m.out_features = module.in_features, module.out_features
        m.w_qdq_name = _func_name(w_qdq)
        m.a_qdq_name = _func_name(a_qdq) if a_qdq is not None else 'None'
        return m

    @classmethod
    def get_func_name(cls, any_callable):
        return _func_name(any_callable)

    def __repr__(self):
        return (f'FakeQuantLinear(in_features={self.in_features},out_features={self.out_features}, '
                f'bias={self.bias is not None},weight_quant={self.w_qdq_name},act_quant={self.a_qdq_name})')


class EffcientFakeQuantLinear(nn.Module):
    """module_utils.py:681-759 (spelling as in the reference): the weight is fake-quantized once at new()."""

    def __init__(self, weight, bias, ori_module, a_qdq):
        super().__init__()
        self.register_buffer('weight', weight)
        if bias is not None:
            self.register_buffer('bias', bias)
        else:
            self.bias = None
        self.a_qdq = a_qdq
        _copy_buf(self, ori_module)
        _keep_rotater(self, ori_module)

    @torch.no_grad()
    def forward(self, x):
        if self.rotater is not None:
            x = self.rotater.rotate(x)
        if self.a_qdq is not None:
            x = self.a_qdq(x, self)
        return hip_linear(x, self.weight, self.bias)

    @classmethod
    @torch.no_grad()
    def new(cls, module, w_qdq, a_qdq, debug_print={}):
        weight = w_qdq(module)
        bias = module.bias.data if module.bias is not None else None
        m = cls(weight, bias, ori_module=module, a_qdq=a_qdq)
        m.in_features, m.out_features = module.in_features, module.out_features
        m.w_qdq_name = _func_name(w_qdq)
        m.a_qdq_name = _func_name(a_qdq) if a_qdq is not None else 'None'
        m.debug_print = debug_print
        return m

    @classmethod
    def get_func_name(cls, any_callable):
        return _func_name(any_callable)

    def __repr__(self):
        return (f'EffcientFakeQuantLinear(in_features={self.in_features},out_features={self.out_features},'
                f'bias={self.bias is not None},weight_quant={self.w_qdq_name},act_quant={self.a_qdq_name})')


class VllmRealQuantLinear(nn.Module):
    """module_utils.py:762-876: compressed-tensors layout (weight_packed int32 [R, K*b/32] or weight int8/fp8,
    weight_scale, input_scale).

    forward (an extension: the reference raises) runs the plain FP8 form — `weight` float8_e4m3fn with a per-channel or
    per-tensor `weight_scale`: with an e4m3 `act` section, dynamic per_token or static per_tensor, the activation is quantized
    and the epilogue-scaled FP8 GEMM runs (fp8_linear_ops.fp8_linear_forward); weight-only, the weight is de-quantized and goes
    through hip_linear. `new` records what that needs from quant_config (act_cfg, act_mode). Every other stored form raises
    NotImplementedError, naming itself."""

    act_cfg = None          # the `act` section `new` saw (None: weight-only, or a module built by hand)
    act_mode = None         # fp8_linear_ops.act_mode(act_cfg), or the NotImplementedError it raised, kept for forward

    def __init__(self, weight, bias, scales, input_scale, need_pack, scales_name):
        super().__init__()
        self.register_buffer('weight_packed' if need_pack else 'weight', weight)
        if bias is not None:
            self.register_buffer('bias', bias)
        else:
            self.bias = None
        self.register_buffer(scales_name, scales)
        self.register_buffer('input_scale', input_scale)

    @torch.no_grad()
    def forward(self, x):
        from . import fp8_linear_ops as F8
        name = type(self).__name__
        if getattr(self, 'weight', None) is None:
            raise NotImplementedError(f'{name}.forward: packed integer weights (weight_packed) are not provided; the INT4 / INT8 '
                                      'de-quantize GEMM is separate work')
        if getattr(self, 'weight_scale', None) is None:
            raise NotImplementedError(f'{name}.forward: per_block scales (weight_scale_inv) are not provided here; block-128 '
                                      'checkpoints run on LlmcFp8Linear')
        if self.weight.dtype != torch.float8_e4m3fn:
            raise NotImplementedError(f'{name}.forward: weight dtype {self.weight.dtype} is not provided (float8_e4m3fn is; int8 '
                                      'and e5m2 are not)')
        if isinstance(self.act_mode, NotImplementedError):
            raise NotImplementedError(f'{name}.forward: {self.act_mode}')
        if self.act_mode is None:
            if self.input_scale is not None:      # a module built by hand or loaded without its configuration
                F8._announce(name, tuple(self.weight.shape), 'the module holds an input_scale but no `act` section was '
                             'recorded (act_cfg is None)', 'weight-only forward, activations NOT quantized; set act_cfg / act_mode')
            return hip_linear(x, F8.fp8_dequant(self.weight, self.weight_scale, x.dtype), self.bias)
        if getattr(self, '_aquantizer', None) is None:
            self._aquantizer = F8._quantizer(self.act_cfg)
        input_scale = self.input_scale if self.act_mode == 'static_per_tensor' else None
        return F8.fp8_linear_forward(x, self.weight, self.weight_scale, self._aquantizer, input_scale, self.bias)

    @classmethod
    @torch.no_grad()
    def new(cls, module, w_q, quant_config):
        weight, scales = cls.quant_pack(module, w_q, quant_config)
        input_scale = getattr(module, 'buf_act_scales_0', None)
        if ('act' in quant_config and quant_config['act'].get('static', False)
                and quant_config.get('quant_type', 'int-quant') == 'int-quant'):
            input_scale = input_scale.unsqueeze(0)
        bias = module.bias.data if module.bias is not None else None
        need_pack = quant_config['weight'].get('need_pack', False)
        scales_name = 'weight_scale_inv' if quant_config['weight']['granularity'] == 'per_block' else 'weight_scale'
        m = cls(weight, bias, scales, input_scale, need_pack, scales_name)
        m.in_features, m.out_features = module.in_features, module.out_features
        m.weight_shape, m.weight_dtype = weight.shape, weight.dtype
        m.scales_shape, m.scales_dtype = scales.shape, scales.dtype
        m.zeros_shape = m.zeros_dtype = None
        # what forward needs from the configuration; a pairing it does not run is kept as the error it will raise
        from .fp8_linear_ops import act_mode
        m.act_cfg = dict(quant_config['act']) if 'act' in quant_config else None
        try:
            m.act_mode = act_mode(m.act_cfg)
        except NotImplementedError as e:
            m.act_mode = e
        return m

    @classmethod
    @torch.no_grad()
    def quant_pack(cls, module, w_q, quant_config):
        weight, scales, zeros = w_q(module)
        if quant_config['weight'].get('need_pack', False):
            weight, scales = cls.pack(weight, scales, quant_config)
        return weight, scales

    @classmethod
    @torch.no_grad()
    def pack(cls, weight, scales, quant_config):
        """module_utils.py:836-862 on the GPU: LSB-first nibbles/bytes of (code + 2^(b-1)) into int32."""
        return pack_lsb(weight, quant_config['weight']['bit']), scales.to(torch.float16)

    def __repr__(self):
        return (f'{type(self).__name__}(in_features={self.in_features}, out_features={self.out_features}, '
                f'bias={self.bias is not None}, weight_shape={self.weight_shape}, weight_dtype={self.weight_dtype}, '
                f'scales_shape={self.scales_shape}, scales_dtype={self.scales_dtype})')


class LightllmRealQuantLinear(VllmRealQuantLinear):
    pass


class Lightx2vRealQuantLinear(VllmRealQuantLinear):
    pass


class SglRealQuantLinear(VllmRealQuantLinear):
    pass


class AutoawqRealQuantLinear(nn.Module):
    """module_utils.py:936-1065: AutoAWQ GEMM layout (qweight [K, R/8], qzeros [K/g, R/8], scales [K/g, R] f16)."""

    def __init__(self, weight, bias, scales, zeros):
        super().__init__()
        self.register_buffer('qweight', weight)
        if bias is not None:
            self.register_buffer('bias', bias)
        else:
            self.bias = None
        self.register_buffer('scales', scales)
        if zeros is not None:
            self.register_buffer('qzeros', zeros)
        else:
            self.qzeros = None

    @torch.no_grad()
    def forward(self, x):
        raise NotImplementedError

    @classmethod
    @torch.no_grad()
    def new(cls, module, w_q, quant_config):
        weight, scales, zeros = cls.quant_pack(module, w_q, quant_config)
        bias = module.bias.data if module.bias is not None else None
        m = cls(weight, bias, scales, zeros)
        m.in_features, m.out_features = module.in_features, module.out_features
        m.weight_shape, m.weight_dtype = weight.shape, weight.dtype
        m.scales_shape, m.scales_dtype = scales.shape, scales.dtype
        m.zeros_shape = zeros.shape if zeros is not None else None
        m.zeros_dtype = zeros.dtype if zeros is not None else None
        return m

    @classmethod
    @torch.no_grad()
    def quant_pack(cls, module, w_q, quant_config):
        _, scales, zeros = w_q(module)
        pack_version = quant_config['weight']['pack_version']
        if pack_version != 'gemm_pack':
            raise NotImplementedError(f'Not support {pack_version}.')
        return cls.gemm_pack(module, module.weight.data, scales, zeros, quant_config)

    @classmethod
    @torch.no_grad()
    def gemm_pack(cls, module, weight, scales, zeros, quant_config):
        assert scales is not None and zeros is not None
        if quant_config['weight']['bit'] != 4:
            raise NotImplementedError('Only 4-bit are supported for now.')
        return pack_awq_gemm(weight, scales, zeros, quant_config['weight']['group_size'])


class MlcllmRealQuantLinear(AutoawqRealQuantLinear):
    pass


class LlmcFp8Linear(nn.Module):
    """module_utils.py:130-191: a Linear whose checkpoint weight is block-scaled FP8 (DeepSeek-V3): `weight`
    float8_e4m3fn [R, K] + `weight_scale_inv` fp32 [ceil(R/b), ceil(K/b)]. forward quantizes the activation per
    1 x b block and runs the block-scaled fp8 GEMM (kernel.block_wise_fp8_forward_func) — on gfx950 the HIP kernels
    replace the reference's Hopper-only Triton path, so its bf16 de-quantize-and-F.linear fallback is not needed."""

    def __init__(self, in_features, out_features, bias, block_size):
        super().__init__()
        self.block_size, self.in_features, self.out_features = block_size, in_features, out_features
        if bias is not None:
            self.bias = nn.Parameter(torch.empty(out_features))
        else:
            self.register_parameter('bias', None)
        self.weight = nn.Parameter(torch.empty(out_features, in_features, dtype=torch.float8_e4m3fn), requires_grad=False)
        so, si = -(-out_features // block_size), -(-in_features // block_size)
        self.weight_scale_inv = nn.Parameter(torch.empty(so, si, dtype=torch.float32), requires_grad=False)

    def forward(self, x):
        from .kernel import block_wise_fp8_forward_func, weight_cast_to_bf16
        if self.weight.data.dtype == torch.float8_e4m3fn:
            if self.block_size == 128 and x.shape[-1] % 128 == 0:
                return block_wise_fp8_forward_func(x, self.weight.data, self.weight_scale_inv.data, self.block_size,
                                                   None if self.bias is None else self.bias.data)
            w = weight_cast_to_bf16(self.weight.data, self.weight_scale_inv.data, self.block_size)
            return hip_linear(x, w, self.bias)
        return hip_linear(x, self.weight, self.bias)

    @classmethod
    @torch.no_grad()
    def new(cls, module, block_size):
        return cls(module.in_features, module.out_features, module.bias, block_size)

    def __repr__(self):
        return (f'LlmcFp8Linear(in_features={self.in_features}, out_features={self.out_features}, '
                f'bias={self.bias is not None}, weight_shape={self.weight.shape}, weight_dtype={self.weight.dtype}, '
                f'block_size={self.block_size})')


class MxFp4RealQuantLinear(nn.Module):
    """A Linear on the OCP MXFP4 stored form (no reference counterpart: its real-quant Linears raise in forward):
    `weight_packed` uint8 [R, K/2] (e2m1, element 2i in the low nibble) + `weight_scale` uint8 [R, K/32] (e8m0), what
    FloatQuantizer(bit='e2m1', float_semantics='ocp', scale_format='e8m0', per_group, group_size=32) returns. With an activation
    section (`bit` e2m1 or e4m3, dynamic) forward quantizes the activation per 1 x 32 block and runs the block-scaled MFMA GEMM
    (mx_ops.mx_linear_forward); weight-only, or in_features % 128 != 0: the weight is de-quantized and goes through hip_linear."""

    _WEIGHT = {'bit': 'e2m1', 'granularity': 'per_group', 'group_size': 32, 'float_semantics': 'ocp', 'scale_format': 'e8m0'}
    _ACT_BITS = ('e2m1', 'e4m3')

    def __init__(self, weight, bias, scales, act_bit):
        super().__init__()
        self.register_buffer('weight_packed', weight)
        self.register_buffer('weight_scale', scales)
        if bias is not None:
            self.register_buffer('bias', bias)
        else:
            self.bias = None
        self.act_bit = act_bit

    @classmethod
    def check_config(cls, quant_config):
        """The activation format (None: weight-only) of a configuration this module takes; ValueError with the reason otherwise."""
        w = quant_config['weight']
        for k, want in cls._WEIGHT.items():
            if w.get(k) != want:
                raise ValueError(f"mxfp4_quant: the weight section needs {k}: {want} (the OCP MX stored form: e2m1 codes, one "
                                 f"e8m0 scale per 32 elements), got {k}: {w.get(k)!r}")
        a = quant_config.get('act')
        if a is None:
            return None
        if a.get('bit') not in cls._ACT_BITS:
            raise ValueError(f"mxfp4_quant: activations are quantized per 1 x 32 block to e2m1 or e4m3 with e8m0 scales, got act bit: "
                             f"{a.get('bit')!r} (e3m2 has no dense packing, e5m2 is not provided)")
        if a.get('static', False):
            raise ValueError('mxfp4_quant: static activation scales are not provided (the MX block scales are dynamic)')
        return a['bit']

    @torch.no_grad()
    def forward(self, x):
        from .quant import dequant_fpx
        if self.act_bit is not None and self.in_features % 128 == 0:
            from .mx_ops import mx_linear_forward
            return mx_linear_forward(x, self.weight_packed, self.weight_scale, self.act_bit, self.bias)
        w = dequant_fpx(self.weight_packed, self.weight_scale, 'e2m1', 32, x.dtype)
        return hip_linear(x, w, self.bias)

    @classmethod
    @torch.no_grad()
    def new(cls, module, w_q, quant_config):
        act_bit = cls.check_config(quant_config)
        weight, scales, _ = w_q(module)
        bias = module.bias.data if module.bias is not None else None
        m = cls(weight.contiguous(), bias, scales.reshape(weight.shape[0], -1).contiguous(), act_bit)
        m.in_features, m.out_features = module.in_features, module.out_features
        m.weight_shape, m.weight_dtype = weight.shape, weight.dtype
        m.scales_shape, m.scales_dtype = m.weight_scale.shape, m.weight_scale.dtype
        m.zeros_shape = m.zeros_dtype = None
        return m

    def __repr__(self):
        return (f'MxFp4RealQuantLinear(in_features={self.in_features}, out_features={self.out_features}, '
                f'bias={self.bias is not None}, weight_shape={self.weight_shape}, weight_dtype={self.weight_dtype}, '
                f'scales_shape={self.scales_shape}, scales_dtype={self.scales_dtype}, act_bit={self.act_bit})')


_TRANSFORMERS_LINEAR_TYPES_ = [nn.Linear]
_TRANSFORMERS_LN_TYPES_ = [nn.LayerNorm]
try:  # RMSNorm-style layers of HF models count as LN types for apply_scale
    from transformers.pytorch_utils import ALL_LAYERNORM_LAYERS
    _TRANSFORMERS_LN_TYPES_ = list(ALL_LAYERNORM_LAYERS)
except Exception:  # pragma: no cover
    pass
if hasattr(nn, 'RMSNorm') and nn.RMSNorm not in _TRANSFORMERS_LN_TYPES_:
    _TRANSFORMERS_LN_TYPES_.append(nn.RMSNorm)

_LLMC_LN_TYPES_ = [LlmcRMSNorm]
_LLMC_LINEAR_TYPES_ = [LlmcFp8Linear, RotateLinear, OriginFloatLinear, FakeQuantLinear, EffcientFakeQuantLinear, VllmRealQuantLinear,
                       SglRealQuantLinear, AutoawqRealQuantLinear, MlcllmRealQuantLinear, LightllmRealQuantLinear, MxFp4RealQuantLinear]
_REALQUANT_LINEAR_MAP_ = {
    'vllm_quant': VllmRealQuantLinear,
    'lightllm_quant': LightllmRealQuantLinear,
    'sgl_quant': SglRealQuantLinear,
    'autoawq_quant': AutoawqRealQuantLinear,
    'mlcllm_quant': MlcllmRealQuantLinear,
    'lightx2v_quant': Lightx2vRealQuantLinear,
    'mxfp4_quant': MxFp4RealQuantLinear,
}
