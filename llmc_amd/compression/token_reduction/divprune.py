"""DivPrune with llmc's operator surface (llmc/compression/token_reduction/divprune.py:13-149): of the L image tokens of a prompt
keep the int(round(rate * L)) that are most diverse, chosen greedily by the max-min rule on the pairwise cosine distance.

  D[i][j]  = 1 - cos(token_i, token_j)                                                       (pairwise_cosine_similarity, :13-27)
  step 0:    the token whose second smallest distance in its column is greatest              (:44-47)
  step i:    the token whose smallest distance to the tokens chosen so far is greatest       (:48-52)

The reference runs k steps of index_select + min + argmax + a scalar write, and its step i gathers all i chosen rows again. Here the
matrix is one Gram kernel on the matrix pipe and the k steps are one launch that reads one row per step (token_ops.py,
csrc/token_select.hip); the running minimum with the row chosen last is exactly the minimum over the chosen rows. The choice never
leaves the device. CPU tensors run the reference's sequence from torch ops.

Where this differs from the reference, and why:
  * the matrix divprune() returns is fp32, not the feature dtype. In fp16 the reference's distances near 1 are spaced 2^-11 apart
    (bf16: 2^-8), so many of its choices are ties that the summation order of the BLAS library decides; the fp32 matrix keeps the
    distances apart. A `cosine_matrix` the caller supplies is used as it is, in its own dtype.
  * IMAGE_TOKEN_INDEX comes from pruning_config['image_token_index'] (through special['vision_token_index']); `llava.constants` is
    imported only when the adapter leaves that key out, so the method needs no `llava` package where the adapter states the index.
  * for a model class other than `Llava` the reference registers nothing without a word; here that is said once on stderr.
  * divprune_post_hook slices position_ids along dim 1 whatever their rank (the reference's [:, keep, :] takes 3-D ids only; LLaVA's
    are [batch, length] or None)."""
import sys
from functools import wraps
from types import MethodType

import torch

from llmc_amd.utils.registry_factory import TOKEN_REDUCTION_REGISTRY

from . import token_ops
from .token_reduction_module import TokenReductionModule

_SAID = set()


def pairwise_cosine_similarity(matrix):
    """[N, d] -> fp32 [N, N] of cosines: 1 - the distance the kernel writes (exact for |cos| >= 0.5, a rounding otherwise)."""
    return 1.0 - token_ops.cosine_distance(matrix)


def divprune(visual_feature_vectors, image_feature_length, cosine_matrix=None, threshold_ratio=0.1):
    """-> (int64 [k] indices in the order chosen, the distance matrix), k = int(round(threshold_ratio * image_feature_length))."""
    threshold_terms = int(round(threshold_ratio * image_feature_length))
    if cosine_matrix is None:
        cosine_matrix = token_ops.cosine_distance(visual_feature_vectors)
    s = token_ops.maxmin_select(cosine_matrix, threshold_terms)
    return s, cosine_matrix


def divprune_post_hook(input_ids, position_ids, attention_mask, past_key_values, inputs_embeds, labels, pruning_paras=None):
    rate = pruning_paras['rate']
    SYS_TOKEN_LEN = pruning_paras['image_token_start_index']
    img_feature_len = pruning_paras['image_token_length']
    device = inputs_embeds.device
    visual_tokens = inputs_embeds[0][SYS_TOKEN_LEN: SYS_TOKEN_LEN + img_feature_len]
    selected_visual_tokens, cosine_matrix = divprune(visual_tokens, img_feature_len, None, threshold_ratio=rate)

    selected_visual_tokens = selected_visual_tokens + SYS_TOKEN_LEN
    keep_indexs = torch.cat((
        torch.arange(SYS_TOKEN_LEN, device=device),
        selected_visual_tokens,
        torch.arange(SYS_TOKEN_LEN + img_feature_len, inputs_embeds.shape[1], device=device),
    ))
    keep_indexs = keep_indexs.sort().values

    inputs_embeds = inputs_embeds[:, keep_indexs]
    if position_ids is not None:
        position_ids = position_ids[:, keep_indexs]
    if attention_mask is not None:
        attention_mask = attention_mask[:, keep_indexs]

    return input_ids, position_ids, attention_mask, past_key_values, inputs_embeds, labels


@TOKEN_REDUCTION_REGISTRY.register('DivPrune')
class DivPrune(TokenReductionModule):
    def __init__(self, config, model, blocks):
        super().__init__(config, model, blocks)
        self.add_sparse_config()
        self.register_reduction_modules()

    def add_sparse_config(self):
        self.special_config['image_token_length'] = self.model.pruning_config['image_token_length']
        self.pruning_paras = self.special_config

    def register_reduction_modules(self):

        def input_hook_llava(fn, pruning_paras, image_token_index):
            @wraps(fn)
            def wrapper(self, *args, **kwargs):
                if len(args) == 0:
                    return fn(*args, **kwargs)
                input_args = args[0]
                if hasattr(input_args[0], 'shape') and input_args[0].shape[0] == 1:      # a decode step: one token
                    return fn(*args, **kwargs)

                input_ids = args[0]
                attention_mask = args[2] if len(args) > 2 else None
                ids = input_ids[0] if attention_mask is None else input_ids[0][attention_mask[0].bool()]
                token_indices = ids == image_token_index
                pruning_paras['image_token_start_index'] = torch.where(token_indices)[0].item()

                outputs = fn(*args, **kwargs)

                return divprune_post_hook(*outputs, pruning_paras=pruning_paras)

            return wrapper

        name = self.model.__class__.__name__
        if name == 'Llava':
            image_token_index = self.pruning_paras.get('vision_token_index')
            if image_token_index is None:
                from llava.constants import IMAGE_TOKEN_INDEX as image_token_index

            hook_fn = input_hook_llava(self.model.vlm_model.prepare_inputs_labels_for_multimodal, self.pruning_paras,
                                       image_token_index)
            self.model.vlm_model.prepare_inputs_labels_for_multimodal = MethodType(hook_fn, self.model.vlm_model)
        elif name not in _SAID:
            _SAID.add(name)
            print(f'[llmc_amd] DivPrune: model class {name} is not Llava: nothing is registered and every image token stays',
                  file=sys.stderr)
