"""HFLlama (tests/hf_adapters.py) with the members QuaRot calls on llmc's model adapters (llmc/models/base_model.py, llama.py):
embedding / head / final-norm accessors and norm replacement (LlmcRMSNorm). Sizes: hidden 256 (= 4^4, so sqrt(n) is exact),
4 heads, 2 KV heads, intermediate 448 = 28 * 16 (the order-28 Paley factor). Test infrastructure."""
import torch

from hf_adapters import HFLlama


class RotLlama(HFLlama):
    def get_embed_layers(self):
        return [self.model.model.embed_tokens]

    def get_head_layers(self):
        return [self.model.lm_head]

    def get_pre_head_layernorm_layers(self):
        return [self.model.model.norm]

    def get_extra_rot_module_besides_embed_layers(self):
        return []

    @staticmethod
    def _is_norm(m):
        w = getattr(m, 'weight', None)
        return type(m).__name__.endswith('Norm') and torch.is_tensor(w) and w.dim() == 1

    def _replace_norms(self, cls, root, named, params):
        for name, m in named.items():
            parent_name, _, child = name.rpartition('.')
            parent = root.get_submodule(parent_name) if parent_name else root
            setattr(parent, child, cls.new(m, **params))

    def replace_module_subset(self, cls, block, subset, block_idx, params):
        if cls.__name__ == 'LlmcRMSNorm':          # models/base_model.py:424-431 replaces norms by their own rule
            named = {n: m for n, m in subset['layers'].items() if self._is_norm(m)}
            # `block` is the whole model for the final norm ({'model.norm': ...}): names are relative to it
            return self._replace_norms(cls, block, named, params)
        return super().replace_module_subset(cls, block, subset, block_idx, params)

    def replace_module_block(self, cls, block, block_idx, params):
        if cls.__name__ == 'LlmcRMSNorm':
            named = {n: m for n, m in block.named_modules() if self._is_norm(m) and type(m).__name__ != 'LlmcRMSNorm'}
            return self._replace_norms(cls, block, named, params)
        return super().replace_module_block(cls, block, block_idx, params)


def rot_llama(dtype=torch.bfloat16, seed=0, layers=2, tie=False):
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(seed)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=448, num_hidden_layers=layers, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=160, max_position_embeddings=256, attn_implementation='eager',
                      tie_word_embeddings=tie)
    cfg.use_cache = False
    net = LlamaForCausalLM(cfg)
    g = torch.Generator().manual_seed(seed + 1)
    for n, p in net.named_parameters():            # norms with a real scale, so that fuse_ln_fcs has something to fuse
        if p.dim() == 1:
            p.data = 1.0 + 0.25 * torch.randn(p.shape, generator=g)
    return RotLlama(net, dtype)
