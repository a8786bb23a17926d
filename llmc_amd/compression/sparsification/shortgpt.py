"""ShortGPT with llmc's operator surface (llmc/compression/sparsification/shortgpt.py:18-113): the structured method of the
family. A decoder block's importance is its Block Influence, the sum over the calibration tokens of 1 - cos(input, output), and
the n_prune_layers least important blocks are deleted whole: the saved model is smaller and faster with no sparse kernel.

  bi[t]          = 1 - dot(x_t, y_t) / (||x_t|| * ||y_t||), a NaN cosine (a zero token) counted as 0.5       (compute_bi, :40-55)
  importances[b] = sum over every calibration token of bi[t]                                                 (subset_transform, :58-66)
  remove the n_prune_layers blocks of lowest importance, or an explicit list                                 (remove_layers, :69-83)

The score runs in one HIP kernel (csrc/block_influence.hip through sparse_ops.block_influence): every element of the block's
input and output is read once, where the reference forms the N x N product input @ output.T and keeps its diagonal. The kernel
writes each block's fp64 score into its element of `importances` on the device; the host reads the vector once, in deploy (the
reference synchronises once per block). block_opt is one dense forward whose output feeds the next block: no Linear hooks, no
subsets. Without a GPU the block stays where it is and the score is composed from torch ops (block_influence_composed).

Where this differs from the reference, and why:
  * shortgpt.py:64-66 scores input_feat[0] and output_feat[0] only, the first calibration batch. With the shipped config
    (calib.bs = -1) there is one batch and this is the same statistic; when the calibration data arrives in several batches ours
    sums over all of them, as the method is defined.
  * shortgpt.py:49-55 rounds the two norms, their product, the N x N product, the quotient and 1 - sim to the model dtype. In bf16
    the spacing near 1 is 2^-8, so a deep block whose per-token influence is about 0.01 is scored in steps of 0.004. Ours keeps
    fp32 from the products to 1 - sim and sums the tokens in fp64 (the order: include/llmc_hip.h; the bound:
    tests/shortgpt_oracle.py). On fp32 inputs the two agree within that bound plus the reference's own distance from the fp64
    value; on 16-bit inputs ours is the one nearer to it (tests/golden/shortgpt.npz, tools/make_golden_shortgpt.py).
  * shortgpt.py:74 ranks with np.argsort's default sort, which is not stable: among equal importances the reference's choice is
    unspecified. Ours is stable: ties go to the lower block index.
  * remove_layers deletes from the container the model owns (the reference deletes from self.blocks, which for an adapter that
    returns a copy changes nothing in the model), then renumbers what is left: model_config.num_hidden_layers (and a per-layer
    `layer_types` list) where the model has them, and `layer_idx` on the kept blocks' modules that carry one, so the in-memory
    model runs with a KV cache. The reference only patches num_hidden_layers in the saved config.json; save_model does that too."""
import gc
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

from llmc_amd.utils.registry_factory import ALGO_REGISTRY

from . import sparse_ops
from .base_blockwise_sparsification import BaseBlockwiseSparsification


@ALGO_REGISTRY
class ShortGPT(BaseBlockwiseSparsification):
    needs_input_feat = False

    def __init__(self, model, sparsity_config, input, padding_mask, config):
        super().__init__(model, sparsity_config, input, padding_mask, config)
        if not hasattr(self, 'n_prune_layers'):
            raise ValueError('ShortGPT needs sparse.weight.n_prune_layers (and no sparse.weight.sparsity): the number of blocks '
                             'to remove')
        n = self.n_prune_layers
        if isinstance(n, bool) or int(n) != n or not 0 <= int(n) < self.num_blocks:
            raise ValueError(f'sparse.weight.n_prune_layers = {n!r} outside [0, {self.num_blocks}): the model has '
                             f'{self.num_blocks} blocks and at least one must stay')
        self.n_prune_layers = int(n)
        if self.data_free:
            raise ValueError('ShortGPT scores a block by the change it makes to the calibration tokens: it needs calibration data')
        self.device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
        self.importances = torch.zeros(self.num_blocks, dtype=torch.float64, device=self.device)

    @torch.no_grad()
    def block_opt(self, block):
        block = block.to(self.device)
        output_feat = self.block_forward(block)
        self.block_transform(self.input['data'], output_feat)
        self.input['data'] = output_feat
        block = block.cpu()
        gc.collect()
        if self.device.type == 'cuda':
            torch.cuda.empty_cache()

    def block_transform(self, input_feat, output_feat):
        self.subset_transform(input_feat, output_feat)

    @torch.no_grad()
    def compute_bi(self, input_feat, output_feat):
        """The per-token 1 - sim of [..., d] input and output features -> fp32 [N]."""
        return sparse_ops.block_influence(input_feat, output_feat)[0]

    @torch.no_grad()
    def subset_transform(self, input_feat, output_feat):
        """The block's score over every batch, written into its element of `importances` on the device."""
        if len(input_feat) != len(output_feat) or not len(input_feat):
            raise ValueError(f'ShortGPT: {len(input_feat)} input and {len(output_feat)} output batches')
        total = self.importances[self.block_idx]
        for i, (x, y) in enumerate(zip(input_feat, output_feat)):
            sparse_ops.block_influence(x.to(self.device), y.to(self.device), total, init=i == 0)

    def _container(self):
        """The nn.ModuleList of the model that holds the blocks: what an adapter's get_blocks() returns, or, where that is a
        copy, the ModuleList with exactly these modules."""
        blocks = self.model.get_blocks()
        if isinstance(blocks, nn.ModuleList):
            return blocks
        for m in self.model.get_model().modules():
            if isinstance(m, nn.ModuleList) and len(m) == len(blocks) and all(a is b for a, b in zip(m, blocks)):
                return m
        raise NotImplementedError('ShortGPT: the model holds its blocks in no nn.ModuleList; there is nothing to delete from')

    @torch.no_grad()
    def remove_layers(self, layers_to_remove=[]):
        """Delete blocks from the model: the given indices, or the n_prune_layers of lowest importance (ties: lower index).
        An index that does not exist is skipped with a message. -> the list."""
        if not layers_to_remove and self.n_prune_layers:
            scores = self.importances.detach().cpu().numpy()
            layers_to_remove = np.argsort(scores, kind='stable')[:self.n_prune_layers].tolist()
        container = self._container()
        before = list(container)
        for idx in sorted(layers_to_remove, reverse=True):
            try:
                del container[idx]
            except IndexError:
                print(f'[llmc_amd] ShortGPT: layer {idx} does not exist', file=sys.stderr)
        self.blocks = self.model.get_blocks()
        self.num_blocks = len(self.blocks)
        if self.num_blocks != len(before):
            self._renumber(before)
        return layers_to_remove

    def _renumber(self, before):
        """What counts or names the blocks follows the removal: num_hidden_layers and a per-layer layer_types list of the
        model's config(s), layer_idx on the kept blocks' modules (the slot of an attention module in a KV cache)."""
        kept = [i for i, b in enumerate(before) if any(b is k for k in self.blocks)]
        seen = []
        for cfg in (getattr(self.model, 'model_config', None), getattr(self.model.get_model(), 'config', None)):
            if cfg is None or any(cfg is c for c in seen) or getattr(cfg, 'num_hidden_layers', None) is None:
                continue
            seen.append(cfg)
            types = getattr(cfg, 'layer_types', None)
            if isinstance(types, (list, tuple)) and len(types) == len(before):
                cfg.layer_types = [types[i] for i in kept]
            cfg.num_hidden_layers = self.num_blocks
        for i, block in enumerate(self.blocks):
            for m in block.modules():
                if isinstance(getattr(m, 'layer_idx', None), int):
                    m.layer_idx = i

    @torch.no_grad()
    def deploy(self, deploy_format):
        """The one host read of the scores, then the removal."""
        return self.remove_layers()

    @torch.no_grad()
    def save_model(self, path):
        """The base's writer, then num_hidden_layers in the written config.json (shortgpt.py:104-113)."""
        super().save_model(path)
        config_file = os.path.join(path, 'config.json')
        if os.path.exists(config_file) and int(os.environ.get('RANK', '0')) == 0:
            with open(config_file, 'r') as fh:
                config_new = json.load(fh)
            config_new['num_hidden_layers'] = len(self.blocks)
            with open(config_file, 'w') as fh:
                json.dump(config_new, fh, indent=4)
