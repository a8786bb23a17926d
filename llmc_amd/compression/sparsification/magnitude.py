"""Magnitude pruning with llmc's operator surface (llmc/compression/sparsification/magnitude.py:9-31): the data-free baseline.
Per layer, thresh = the |W| of rank int(numel * sparsity) over the whole tensor, and every |W| <= thresh becomes 0 (all ties of
the threshold go). One kernel call per layer (sparse_ops.magnitude_prune, csrc/prune.hip): a histogram of the bit patterns
instead of a sort of the tensor, no host read.

Where this differs from the reference, and why:
  * magnitude.py:31 applies `W[W_mask] = 0` AFTER its `for` loop, so only the last layer of a subset would be pruned. Ours
    prunes every layer of the subset, each with its own threshold.
  * magnitude.py:28 reads self.sparser.sparsity, which the reference never defines; the base class defines it here.
  * sparsity 1.0 indexes past the sorted tensor in the reference (IndexError); ours raises ValueError.
  * it reads no activations: with input=None it runs data-free, and with calibration data it registers no hooks (the block
    forward still runs, so that the block loop hands on the same inputs as for any other method).
  * weight.sparsity_type 'n:m' is Wanda's; here it raises NotImplementedError."""
import torch

from llmc_amd.utils.registry_factory import ALGO_REGISTRY

from . import sparse_ops
from .base_blockwise_sparsification import BaseBlockwiseSparsification


@ALGO_REGISTRY
class Magnitude(BaseBlockwiseSparsification):
    needs_input_feat = False

    def __init__(self, model, sparsity_config, input, padding_mask, config):
        super().__init__(model, sparsity_config, input, padding_mask, config)
        if self.nm is not None:
            raise NotImplementedError("Magnitude prunes by one global threshold per layer; sparsity_type 'n:m' is Wanda's")
        if not hasattr(self, 'sparsity'):
            raise ValueError('Magnitude needs sparse.weight.sparsity')

    @torch.no_grad()
    def subset_transform(self, subset, input_feat, subset_kwargs):
        layers_dict = subset['layers']
        layers = list(layers_dict.values())
        for layer in layers:
            W = layer.weight.data
            sparse_ops.magnitude_prune(W, int(W.numel() * self.sparser.sparsity))
