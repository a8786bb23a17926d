"""AdaDim with llmc's operator surface (llmc/compression/quantization/adadim.py:11-88): per Linear, the weight is fake-quantized
once along the output-channel axis ('oc', the usual one) and once along the input-channel axis ('ic': groups run down a column
of W [R, K]); the axis with the smaller mean((layer(x) - layer_q(x))^2) over the calibration samples is kept in `buf_qdim`
(0 = ic, 1 = oc), and every FakeQuantLinear then re-quantizes its weight along that axis (w_qdq).

The 'ic' quantization is one kernel on the weight as it lies (quant_cols_ops.fake_quant_cols, csrc/quant_cols.hip), on the
search and on every forward. The losses are awq_ops.linear_out / linear_loss_sum (csrc/linear_eval.hip): the difference is
formed in the model dtype, squared and summed in fp32. Per layer the reference output is computed once per sample (the
reference computes it once per axis, with the same bits), the calibration sample is packed k-tiled once for all layers of a
subset and both axes, and the 2 x n_samples sums stay on the device until one host read per layer.

`__init__` follows this package's (model, quant_config, input, padding_mask, config); the reference spells the last two
(config, modality) but receives the same positional values from main().

Decisions where the reference is unreachable or undefined:
  * deploy in a real-quant format — those layouts carry one scale per output channel (or per group along a row); the reference
    silently packs per-'oc' codes for a layer it chose 'ic' for. Ours raises NotImplementedError while any layer has
    buf_qdim == 0.
  * quant_type float-quant — FloatQuantizer.fake_quant_weight_dynamic does not read args['dim'] (in the reference either), so
    both candidates would be the same weight and every layer 'oc' by the tie rule. Ours refuses it at construction.
  * ties and NaN — `loss_ic < loss_oc` is false for both, so they go to 'oc', as in the reference."""
import torch

from llmc_amd import _ffi
from llmc_amd.utils.registry_factory import ALGO_REGISTRY

from . import awq_ops
from .base_blockwise_quantization import BaseBlockwiseQuantization
from .module_utils import _REALQUANT_LINEAR_MAP_, FakeQuantLinear


@ALGO_REGISTRY
class AdaDim(BaseBlockwiseQuantization):
    def __init__(self, model, quant_config, input, padding_mask, config):
        if dict(quant_config['weight']).get('quant_type', 'int-quant') == 'float-quant':
            raise NotImplementedError("AdaDim with quant_type float-quant: FloatQuantizer ignores args['dim'], so the 'ic' and "
                                      "'oc' candidates would be the same weight")
        super().__init__(model, quant_config, input, padding_mask, config)
        self.dim_losses = {}          # layer name -> (loss_oc, loss_ic) of the last search, for tests and logs

    def get_layer_out(self, x, layer):
        with torch.no_grad():
            org_out = layer(x)
            if isinstance(org_out, tuple):
                org_out = org_out[0]
        return org_out

    @torch.no_grad()
    def layer_sample_means(self, layer, input, xpacks):
        """-> fp32 [2, len(input)] on the host: mean((layer(x_i) - layer_q(x_i))^2) per sample, row 0 for 'oc', row 1 for 'ic'.
        The sums are accumulated on the device and read once. `xpacks` (a dict owned by search_dim_subset) keeps the k-tiled
        image of each sample for the other layers of the subset."""
        W = layer.weight.data
        bias = layer.bias.data if getattr(layer, 'bias', None) is not None else None
        q_oc = self.wquantizer.fake_quant_weight_dynamic(W, {'dim': 'oc'})
        q_ic = self.wquantizer.fake_quant_weight_dynamic(W, {'dim': 'ic'})
        n = len(input)
        sums = torch.zeros((2, n), dtype=torch.float32, device=W.device)
        numel = torch.empty(n, dtype=torch.float32)
        packed = None
        for i, x in enumerate(input):
            tokens = x.numel() // x.shape[-1]
            numel[i] = tokens * W.shape[0]
            if bias is None and awq_ops.ktile_supported(x, W) and tokens >= awq_ops.KTILE_MIN_TOKENS \
                    and _ffi.HOST_OPTIONS['awq_kt']:
                if packed is None:
                    packed = [awq_ops.ktile_pack(t) for t in (W, q_oc, q_ic)]
                if i not in xpacks:
                    xpacks[i] = awq_ops.ktile_pack(x)
                xt = xpacks[i]
                y0 = awq_ops.linear_out(xt, packed[0], tiled=True, blocked=True)
                for a in (0, 1):
                    awq_ops.linear_loss_sum(xt, packed[1 + a], y0, sums[a, i:i + 1], tiled=True, y0_blocked=True)
            elif bias is None and awq_ops.linear_supported(x, W):
                y0 = awq_ops.linear_out(x, W)
                for a, q in enumerate((q_oc, q_ic)):
                    awq_ops.linear_loss_sum(x, q, y0, sums[a, i:i + 1])
            else:
                y0 = awq_ops.linear_auto(x, W, bias)
                for a, q in enumerate((q_oc, q_ic)):
                    sums[a, i] = (y0 - awq_ops.linear_auto(x, q, bias)).float().pow(2).sum()
        return sums.cpu() / numel

    @torch.no_grad()
    def search_dim_subset(self, layers_dict, input):
        xpacks = {}
        for name in layers_dict:
            layer = layers_dict[name]
            for i in range(len(input)):
                input[i] = input[i].to(layer.weight.data.device)
            means = self.layer_sample_means(layer, input, xpacks)
            loss_dict = {}
            for row, dim in enumerate(('oc', 'ic')):
                loss_mean = 0
                for i in range(len(input)):
                    loss_mean += input[i].shape[0] * 1.0 / self.n_samples * float(means[row, i])
                loss_dict[dim] = loss_mean
            self.dim_losses[name] = (loss_dict['oc'], loss_dict['ic'])
            qdim = 0 if loss_dict['ic'] < loss_dict['oc'] else 1
            layer.register_buffer('buf_qdim', torch.tensor(qdim))

    @torch.no_grad()
    def block_transform(self, block, input_feat, block_kwargs):
        subsets = self.model.get_subsets_in_block(block)
        for index, subset in enumerate(subsets):
            layers_dict = subset['layers']
            input_name = subset['input'][0]
            self.search_dim_subset(layers_dict, input_feat[input_name])
            self.model.replace_module_subset(FakeQuantLinear, block, subset, self.block_idx,
                                             self.get_replacement_params(mode='fake_quant', w_only=self.w_only, name=None))

    @torch.no_grad()
    def w_qdq(self, module, wquantizer):
        weight = module.weight
        args = {}
        args['dim'] = 'ic' if module.buf_qdim == 0 else 'oc'
        return wquantizer.fake_quant_weight_dynamic(weight, args)

    @torch.no_grad()
    def deploy(self, quant_format, keep_device=False):
        if quant_format in _REALQUANT_LINEAR_MAP_:
            ic = [n for n, m in self.model.get_model().named_modules()
                  if getattr(m, 'buf_qdim', None) is not None and int(m.buf_qdim) == 0]
            if ic:
                raise NotImplementedError(f"AdaDim cannot deploy '{quant_format}': {len(ic)} layers quantize along the input "
                                          f'channels (first: {ic[0]}) and the real-quant layouts have no per-input-channel scales')
        super().deploy(quant_format, keep_device=keep_device)
