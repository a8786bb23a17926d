"""Dense with llmc's operator surface (llmc/compression/sparsification/dense.py:8-16): the method that changes no weight. It is
what the KV-sparse configs name (configs/sparsification/methods/Kvsparse/sinkkv.yml: `sparse.method: Dense` plus a `kvcache`
section): the block loop only hangs the shared cache on every block's attention module, and the cache works at inference time.

Where this differs from the reference, and why:
  * the reference's block_opt runs every calibration sample through the block, hooks and cache included, when it is given
    input: all samples land in one shared, never-reset window before the evaluation starts. Ours runs no forward: Dense has
    nothing to calibrate, so the cache is empty when the evaluation begins, with and without calibration data.
  * dense.py:13 declares block_transform(self, block), which the base's data path calls with three arguments (TypeError); ours
    takes the protocol's three and does nothing."""
import torch

from llmc_amd.utils.registry_factory import ALGO_REGISTRY

from .base_blockwise_sparsification import BaseBlockwiseSparsification


@ALGO_REGISTRY
class Dense(BaseBlockwiseSparsification):
    needs_input_feat = False
    accepts_kvcache = True

    def __init__(self, model, sparsity_config, input, padding_mask, config):
        super().__init__(model, sparsity_config, input, padding_mask, config)

    @torch.no_grad()
    def block_opt(self, block):
        if self.sparse_kvcache:
            self.register_kv_cache(block)
        self.block_transform(block, {}, [])

    def block_transform(self, block, input_feat=None, block_kwargs=None):
        return None

    def subset_transform(self, subset, input_feat, subset_kwargs):
        return None
