"""SmoothQuant with llmc's operator surface (llmc/compression/quantization/smoothquant.py:13-79), statistics in HIP.

A subset whose `prev_op[0]` is a norm gets one scale per input channel, scale = x_max^alpha / w_max^(1 - alpha), folded
into the norm (weight / scale) and the subset's Linears (weight * scale); every other subset is left alone
(smoothquant.py:72-74). x_max is the running per-channel max |x| over all calibration batches, w_max the max over the
subset's layers of |W|.max(dim=0): both come from one kernel (llmc_col_stats: one pass per tensor, running fp32 [K] buffers,
no atomics), the pow / div / clamp chain from another (llmc_smooth_scales) with the reference's rounding to the weight dtype
after every op. Block-wise FP8 checkpoint weights are de-blocked first, as collect_layers_weights does. Cached inputs are
rescaled only for static activation quantization (smoothquant.py:78-79)."""
import torch

from llmc_amd.utils.registry_factory import ALGO_REGISTRY

from . import smooth_ops
from .base_blockwise_quantization import BaseBlockwiseQuantization, is_norm_module


@ALGO_REGISTRY
class SmoothQuant(BaseBlockwiseQuantization):
    def __init__(self, model, quant_config, input, padding_mask, config):
        super().__init__(model, quant_config, input, padding_mask, config)
        special_config = self.quant_config.get('special', {}) or {}
        self.alpha = special_config.get('alpha', 0.5)

    @torch.no_grad()
    def filter_subset(self, prev_op):
        """smoothquant.py:20-25; see is_norm_module"""
        return is_norm_module(prev_op[0])

    @torch.no_grad()
    def get_weight_scale(self, layers):
        """smoothquant.py:27-37: max over the layers of |W|.max(dim=0), clamped at 1e-5, in the weight dtype."""
        stats, dtype = None, None
        for fc in layers:
            w = self._fp8_to_bf16(fc.weight, fc.weight_scale_inv) if self._is_fp8(fc) else fc.weight.data
            if stats is None:
                stats, dtype = smooth_ops.ColStats(w.shape[-1], w.device), w.dtype
            stats.update(w)
        return stats.absmax.to(dtype).clamp(min=1e-5)

    @torch.no_grad()
    def get_act_scale(self, tensors):
        """smoothquant.py:39-51: running per-channel max |x| over the batches, fp32."""
        stats = None
        dev = self.dev
        for x in tensors:
            x = x.to(dev)
            if stats is None:
                stats = smooth_ops.ColStats(x.shape[-1], x.device)
            stats.update(x)
        return stats.absmax.clone()

    @torch.no_grad()
    def search_scale_subset(self, layers, tensors):
        """smoothquant.py:53-59"""
        w_max = self.get_weight_scale(layers)
        x_max = self.get_act_scale(tensors)
        return smooth_ops.smooth_scales(x_max, w_max.float(), self.alpha, w_max.dtype)

    @torch.no_grad()
    def subset_transform(self, subset, input_feat, subset_kwargs):
        """smoothquant.py:61-79"""
        layers_dict = subset['layers']
        prev_op = subset['prev_op']
        input_name = subset['input'][0]
        if not self.filter_subset(prev_op):
            return
        layers = list(layers_dict.values())
        scale = self.search_scale_subset(layers, input_feat[input_name])
        self.apply_scale(scale, prev_op, layers)
        if self.act_static:
            self.update_input_feat(scale, input_feat, layers_dict, False)
