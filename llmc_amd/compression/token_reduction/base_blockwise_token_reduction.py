"""`sparse.method: TokenReduction` with the surface of llmc's class
(llmc/compression/token_reduction/base_blockwise_token_reduction.py:13-31): the third family beside quantization and
sparsification. A token-reduction method changes no weight: constructing it patches the model's forward so that fewer vision tokens
reach the language model, the block loop has nothing to do per block, and deploy reports the configuration.

Config (the `sparse` section, configs/sparsification/methods/DivPrune/divprune.yml):
  special.method   the method's key in TOKEN_REDUCTION_REGISTRY. Built: DivPrune. The reference's other twelve (BUILT / UNBUILT
                   below) are refused by name with NotImplementedError: they are forward patches of particular VLMs whose
                   arithmetic is attention scores the model already computes, and none has a kernel here yet.
  special.*        the method's own keys (DivPrune: rate)."""
import sys

import torch

from llmc_amd.utils.registry_factory import ALGO_REGISTRY, TOKEN_REDUCTION_REGISTRY

from ..blockwise_optimization import BlockwiseOpt

BUILT = ('DivPrune',)
UNBUILT = ('DART', 'DyCoke', 'FasterVLM', 'FastV', 'FastVID', 'HoliTom', 'MustDrop', 'PruneVid', 'PyramidDrop', 'SparseVLM', 'ToMe',
           'VisionZip')


@ALGO_REGISTRY
class TokenReduction(BlockwiseOpt):
    def __init__(self, model, sparsity_config, input, padding_mask, config):
        super().__init__(model, sparsity_config, input, padding_mask, config)
        self.register_reduction_modules()

    def register_reduction_modules(self):
        special = self.sparsity_config.get('special') or {}
        method = special.get('method')
        if method in UNBUILT:
            raise NotImplementedError(f'token-reduction method {method} is not built (built: {", ".join(BUILT)}; not built: '
                                      f'{", ".join(UNBUILT)})')
        if method not in TOKEN_REDUCTION_REGISTRY:
            raise NotImplementedError(f'sparse.special.method = {method!r} is no token-reduction method (built: {", ".join(BUILT)})')
        self.reduction_module = TOKEN_REDUCTION_REGISTRY[method](self.sparsity_config, self.model, self.blocks)

    def block_opt(self, block):
        pass

    @torch.no_grad()
    def deploy(self, deploy_format):
        print('[llmc_amd] -- deploy_token_reduction_model start --', file=sys.stderr)
        print(f'[llmc_amd] sparsity_config : {self.sparsity_config}', file=sys.stderr)
        print('[llmc_amd] -- deploy_token_reduction_model done --', file=sys.stderr)
