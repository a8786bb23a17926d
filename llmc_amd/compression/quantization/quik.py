"""QUIK with llmc's operator surface (llmc/compression/quantization/quik.py:13-151): per Linear, the `outlier_num` input
channels of largest calibration activation scale stay in 16 bit, in the activation and in the matching weight columns; the
other channels are fake-quantized (IntegerQuantizer with int_indices / fp_indices: one kernel, mixed_ops.fake_quant_mixed).

get_act_scale_shift runs the blocks forward once with a hook on every nn.Linear and keeps a running per-column max |x| per
layer name on the device (llmc_col_stats through smooth_ops.ColStats, one pass per batch, exact); the reference moves every
batch's statistics to the host. stat='shifts' keeps the reference's 0.99 / 0.01 moving midpoint of the per-batch max / min.
block_opt then registers, per Linear, `buf_int_ids` = the K - outlier_num columns of smallest scale and `buf_fp_ids` = the
outlier_num largest, both in ascending order of scale (so a per_group quantizer groups channels of similar scale).

Decisions where the reference is unreachable or undefined:
  * ties — the reference sorts with torch.sort, whose order among equal values is not defined (it differs from stable=True on
    a tie-heavy input). Ours is the stable order: ascending scale, then ascending column.
  * outlier_num == 0 (`fp_features: 0`, or the layer's largest scale <= fp_threshold) — the reference calls torch.sort(None).
    Ours quantizes every column: int = arange(K), fp empty.
  * fp_relative — the reference reads `block.in_features`, which no block has. Ours reads the Linear's:
    int(m.in_features / hidden_size) * fp_features.
  * last_fc_bit — the reference tests for the key one dictionary level too high, so the shipped config never activates it.
    Ours reads special.last_fc_bit: down_proj / dense_4h_to_h then get the doubled threshold and `buf_current_bit`. Under the
    shipped fp_threshold 0.0, and because current_bit has no arithmetic effect on the fake-quant paths (quant.py), the results
    are identical to the reference's."""
import functools
import gc

import torch
import torch.nn as nn

from llmc_amd.utils.registry_factory import ALGO_REGISTRY

from . import smooth_ops
from .base_blockwise_quantization import BaseBlockwiseQuantization


def choose_indices(layer_scales, outlier_num):
    """-> (int_indices, fp_indices) of a [K] scale table: stable ascending order of scale, the last outlier_num are fp."""
    K = layer_scales.numel()
    if outlier_num <= 0:
        return torch.arange(K, device=layer_scales.device), torch.empty(0, dtype=torch.long, device=layer_scales.device)
    if outlier_num >= K:
        raise ValueError(f'{outlier_num} outlier columns leave nothing to quantize of {K}')
    order = torch.sort(layer_scales, stable=True)[1]
    return order[:K - outlier_num], order[K - outlier_num:]


@ALGO_REGISTRY
class QUIK(BaseBlockwiseQuantization):
    def __init__(self, model, quant_config, input, padding_mask, config):
        super().__init__(model, quant_config, input, padding_mask, config)
        self.add_quant_config()

    def add_quant_config(self):
        special = self.quant_config['special']
        self.prefix = self.model.block_name_prefix
        self.fp_relative = special['fp_relative']
        self.fp_features = special['fp_features']
        self.fp_threshold = special['fp_threshold']
        if 'last_fc_bit' in special:
            self.last_fc_bit = special['last_fc_bit']
        self.act_scales = self.get_act_scale_shift(stat='scales')
        self.int_ids = {}
        self.fp_ids = {}

    @torch.no_grad()
    def get_act_scale_shift(self, stat='scales'):
        """quik.py:30-89 -> {layer name: fp32 [K] on the device}."""
        if stat not in ('scales', 'shifts'):
            raise ValueError(f"stat must be 'scales' or 'shifts', got {stat!r}")
        if self.data_free:
            raise ValueError('QUIK chooses its outlier channels from calibration activations: it needs calibration data')
        net = self.model.get_model()
        net.eval()
        running, act_stat = {}, {}

        def stat_input_hook(m, x, y, name):
            if isinstance(x, tuple):
                x = x[0]
            x = x.detach()
            if stat == 'scales':
                if name not in running:
                    running[name] = smooth_ops.ColStats(x.shape[-1], x.device)
                running[name].update(x)
            else:
                cs = smooth_ops.col_stats(x)
                mid = (cs.max + cs.min) / 2
                act_stat[name] = 0.99 * act_stat[name] + 0.01 * mid if name in act_stat else mid

        hooks = [m.register_forward_hook(functools.partial(stat_input_hook, name=name))
                 for name, m in net.named_modules() if isinstance(m, nn.Linear)]
        try:
            fp_inps = None
            for block in self.blocks:
                block.cuda()
                fp_inps = self.block_forward(block, fp_inps)
                block.cpu()
        finally:
            for h in hooks:
                h.remove()
        gc.collect()
        torch.cuda.empty_cache()
        if stat == 'scales':
            act_stat = {name: cs.absmax for name, cs in running.items()}
        return act_stat

    @torch.no_grad()
    def block_opt(self, block):
        hidden_size = getattr(self, 'hidden_size', None)
        for n, m in self.model.get_block_linears(block).items():
            layer_name = f'{self.prefix}.{self.block_idx}.{n}'
            if self.fp_relative:
                outlier_num = int(m.in_features / hidden_size) * self.fp_features
            else:
                outlier_num = self.fp_features
            layer_scales = self.act_scales[layer_name]
            if outlier_num > 0:
                max_val = layer_scales.abs().max()
                fp_threshold = self.fp_threshold
                if hasattr(self, 'last_fc_bit'):
                    if 'dense_4h_to_h' in n or 'down_proj' in n:
                        fp_threshold = self.fp_threshold * 2
                        m.register_buffer('buf_current_bit', torch.tensor(self.last_fc_bit))
                if max_val <= fp_threshold:
                    outlier_num = 0
            int_indices, fp_indices = choose_indices(layer_scales, outlier_num)
            m.register_buffer('buf_int_ids', int_indices)
            m.register_buffer('buf_fp_ids', fp_indices)
            del self.act_scales[layer_name]

    def _mixed_args(self, module):
        args = {'int_indices': module.buf_int_ids, 'fp_indices': module.buf_fp_ids}
        if hasattr(module, 'buf_current_bit'):
            args['current_bit'] = module.buf_current_bit
        return args

    @torch.no_grad()
    def w_qdq(self, module, wquantizer):
        return wquantizer.fake_quant_weight_dynamic(module.weight, self._mixed_args(module))

    @torch.no_grad()
    def a_qdq(self, act, module, aquantizer, input_index=0):
        return aquantizer.fake_quant_act_dynamic(act, self._mixed_args(module))
