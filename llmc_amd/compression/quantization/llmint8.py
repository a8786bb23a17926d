"""LLM.int8() with llmc's operator surface (llmc/compression/quantization/llmint8.py:11-75): the input channels whose
magnitude reaches `special.threshold` anywhere in the current activation stay in 16 bit, in the activation and in the matching
weight columns; everything else is fake-quantized. Nothing is calibrated (`block_opt` is a no-op): `a_qdq` picks the outlier
columns of each activation it sees and leaves them on the module (`buf_int_ids` / `buf_fp_ids`) for `w_qdq`, which is why
`deploy` takes `fake_quant` only and wraps the Linears in FakeQuantLinear (weight quantized on the forward, after a_qdq).

The per-column max |x| over all tokens and batch rows is one pass of llmc_col_stats (exact: its entries are values of the
activation dtype); the comparison `absmax.to(act.dtype) >= threshold` is torch's own, so its scalar-comparison rule is
inherited. The mixed pass itself is one kernel (mixed_ops.fake_quant_mixed).

Where ours differs from the reference, on purpose: for a batch of B > 1 rows the reference's `torch.where(tmp >= t)[1]` lists a
column once per batch row that exceeds the threshold, so its fp_indices can hold duplicates; ours lists every outlier column
once, in ascending order (the result of the scatter is the same). int_indices is the complement in ascending order."""
import torch

from llmc_amd.utils.registry_factory import ALGO_REGISTRY

from . import smooth_ops
from .base_blockwise_quantization import BaseBlockwiseQuantization
from .module_utils import FakeQuantLinear


@ALGO_REGISTRY
class LlmInt8(BaseBlockwiseQuantization):
    def __init__(self, model, quant_config, input, padding_mask, config):
        super().__init__(model, quant_config, input, padding_mask, config)
        self.add_quant_config()

    @torch.no_grad()
    def add_quant_config(self):
        self.threshold = self.quant_config['special']['threshold']

    @torch.no_grad()
    def block_opt(self, *opt_kwargs):
        pass

    @torch.no_grad()
    def get_outlier_indices(self, act):
        """llmint8.py:25-34 -> (int_indices, fp_indices), int64 on act's device, each ascending and without duplicates."""
        absmax = smooth_ops.col_stats(act).absmax.to(act.dtype)
        is_fp = absmax >= self.threshold
        all_idx = torch.arange(act.shape[-1], device=act.device)
        return all_idx[~is_fp], all_idx[is_fp]

    @torch.no_grad()
    def w_qdq(self, module, wquantizer):
        args = {'int_indices': module.buf_int_ids, 'fp_indices': module.buf_fp_ids}
        return wquantizer.fake_quant_weight_dynamic(module.weight, args)

    @torch.no_grad()
    def a_qdq(self, act, module, aquantizer, input_index=0):
        int_indices, fp_indices = self.get_outlier_indices(act)
        module.register_buffer('buf_int_ids', int_indices)
        module.register_buffer('buf_fp_ids', fp_indices)
        return aquantizer.fake_quant_act_dynamic(act, {'int_indices': int_indices, 'fp_indices': fp_indices})

    @torch.no_grad()
    def deploy(self, quant_format, keep_device=False):
        if quant_format != 'fake_quant':
            raise NotImplementedError(f"LlmInt8 deploys 'fake_quant' only (the outlier columns are chosen on the forward), "
                                      f"not '{quant_format}'")
        if self.mixed_precision:
            self.set_no_quant_layer()
        self.model.replace_language_module_all(FakeQuantLinear,
                                               self.get_replacement_params(mode='fake_quant', w_only=self.w_only, name=None),
                                               keep_device=keep_device)
