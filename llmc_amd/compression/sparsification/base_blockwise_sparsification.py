"""Block loop of the sparsification methods, with the surface of llmc's BaseBlockwiseSparsification
(llmc/compression/sparsification/base_blockwise_sparsification.py:15-204): per block, the inputs of its Linear layers are
captured through forward hooks while the calibration batches run through it, `block_transform` hands every subset to the
method's `subset_transform`, and the block's output becomes the next block's input.

Config (the `sparse` section, configs/sparsification/methods/Wanda/wanda.yml):
  sparsity_out            False (default): the next block's input is this block's DENSE output (the forward that captured the
                          inputs); True: a second forward runs after pruning and feeds the next block.
  weight.sparsity         the fraction of every row (Wanda), of every tensor (Magnitude) or of every 128-column block of a
                          tensor (SparseGPT) that is zeroed.
  weight.n_prune_layers   ShortGPT's key (shortgpt.py): the number of whole blocks it removes; read when the section has no
                          `sparsity`, as in the reference. ShortGPT refuses a section without it or a count outside
                          [0, number of blocks).
  weight.sparsity_type    new key. 'unstructured' (default), or 'n:m' — zero n of every m consecutive input channels, m in
                          {2, 4, 8, 16} ('2:4' is the pattern the CDNA sparse matrix instructions consume). With n:m, `sparsity`
                          must be absent or equal to n / m.
  kvcache                 the KV-sparse caches (configs/sparsification/methods/Kvsparse/*.yml). Only `method: Dense` accepts the
                          section. method SinkKV with window_length and num_sink_tokens (each refused by name when absent)
                          builds a kvsparse.SinkKVCache, appends it to model.kvcache_buffer and sets sparse_kvcache; block_opt
                          then hangs it on every block's attention module (register_kv_cache). method ShadowKV is refused by
                          name: it needs an SVD of the keys, a replaced attention module and a gathered low-rank GEMM, none of
                          which is built. Under Wanda, Magnitude and SparseGPT the section is refused: they run every
                          calibration sample through the hooked attention, which in the reference feeds all samples into one
                          shared, never-reset window.

Departures from the reference, which does not run as shipped:
  * block_transform (base_blockwise_sparsification.py:156-177) calls subset_transform with six positional arguments
    (layers_dict, input_feat, prev_op, input_name, inspect_module, subset_kwargs); Wanda and Magnitude declare three (wanda.py:34-39,
    magnitude.py:15-20). Ours calls subset_transform(subset, input_feat, subset_kwargs): the protocol the two classes
    declare, and the quantization base's.
  * Wanda.subset_transform and Magnitude.subset_transform read self.sparser.sparsity (wanda.py:54, magnitude.py:28); nothing in
    the reference tree defines `sparser`. set_sparsity_config sets self.sparser = SimpleNamespace(sparsity=self.sparsity), so
    subclasses written against that attribute work.
  * the data-free branch (base_blockwise_sparsification.py:153-154) calls block_transform(block) without its two required
    arguments; ours passes input_feat = {} and block_kwargs = [].
  * block_forward moves every tensor in the captured kwargs to the block's device (the quantization base's loop), not only
    `attention_mask` with a bare .cuda() (base_blockwise_sparsification.py:101-106)."""
import functools
import gc
from collections import defaultdict
from types import SimpleNamespace

import torch

from ..blockwise_optimization import BlockwiseOpt
from .sparse_ops import NM_GROUPS


def _has(cfg, key):
    return cfg is not None and key in cfg


def parse_sparsity_type(value):
    """'unstructured' -> None; 'n:m' -> (n, m) with m in NM_GROUPS and 0 <= n <= m."""
    if value is None or value == 'unstructured':
        return None
    try:
        n, m = (int(p) for p in str(value).split(':'))
    except ValueError:
        raise ValueError(f"sparse.weight.sparsity_type must be 'unstructured' or 'n:m', got {value!r}") from None
    if m not in NM_GROUPS or not 0 <= n <= m:
        raise ValueError(f'sparse.weight.sparsity_type {value!r}: m must be one of {NM_GROUPS} and 0 <= n <= m')
    return n, m


class BaseBlockwiseSparsification(BlockwiseOpt):
    needs_input_feat = True          # a method that reads no activations (Magnitude) registers no hooks
    accepts_kvcache = False          # only Dense: it runs no calibration forward through the hooked attention

    def __init__(self, model, sparsity_config, input, padding_mask, config):
        super().__init__(model, sparsity_config, input, padding_mask, config)
        self.set_sparsity_config()

    def block_init(self, block):
        pass

    def set_sparsity_config(self):
        cfg = self.sparsity_config
        self.sparsity_out = bool(_has(cfg, 'sparsity_out') and cfg['sparsity_out'])
        self.sparse_kvcache = False
        if _has(cfg, 'kvcache'):
            self.set_kv_sparse_config()
        self.nm = None
        if _has(cfg, 'weight'):
            w = cfg['weight']
            self.nm = parse_sparsity_type(w['sparsity_type'] if _has(w, 'sparsity_type') else None)
            if self.nm is not None:
                n, m = self.nm
                if _has(w, 'sparsity') and float(w['sparsity']) != n / m:
                    raise ValueError(f"sparse.weight.sparsity {w['sparsity']} contradicts sparsity_type {n}:{m} (= {n / m})")
                self.sparsity = n / m
                self.W_mask = None
            elif _has(w, 'sparsity'):
                self.sparsity = w['sparsity']
                self.W_mask = None
            elif _has(w, 'n_prune_layers'):
                self.n_prune_layers = w['n_prune_layers']
        if hasattr(self, 'sparsity'):
            self.sparser = SimpleNamespace(sparsity=self.sparsity)

    def set_kv_sparse_config(self):
        """base_…:46-62: the `kvcache` section builds the cache named by its method and hands it to the model's kvcache_buffer."""
        kv = self.sparsity_config['kvcache']
        method = kv['method'] if _has(kv, 'method') else None
        if not self.accepts_kvcache:
            raise NotImplementedError(
                f'a KV-cache section under sparse.method {type(self).__name__}: only Dense accepts it. A weight-pruning method runs '
                "every calibration sample through the hooked attention, which in the reference feeds all samples into one shared, "
                'never-reset window')
        if method == 'ShadowKV':
            raise NotImplementedError('KV-cache method ShadowKV is not built: it needs an SVD of the prompt keys, a replaced attention '
                                      'module (replace_attention) and a gathered low-rank GEMM; SinkKV is the KV-sparse cache built here')
        from llmc_amd.utils.registry_factory import KV_REGISTRY
        from . import kvsparse
        if method not in KV_REGISTRY or not issubclass(KV_REGISTRY[method], kvsparse.SinkKVCache):
            raise NotImplementedError(f'KV-cache method {method!r} is not a KV-sparse cache (have: SinkKV)')
        missing = [k for k in ('window_length', 'num_sink_tokens') if not _has(kv, k) or kv[k] is None]
        if missing:
            raise NotImplementedError(f"KV-cache method SinkKV needs kvcache.{' / kvcache.'.join(missing)}: the section has no "
                                      'defaults for them')
        if _has(kv, 'replace_attn') and kv['replace_attn']:
            self.replace_attention(None)
        mc = getattr(self.model, 'model_config', None)
        num_layers = getattr(mc, 'num_hidden_layers', None) or self.num_blocks
        self.kv_module = KV_REGISTRY[method](num_layers, kv['window_length'], kv['num_sink_tokens'])
        self.sparse_kvcache = True
        self.model.kvcache_buffer.append(self.kv_module)

    def replace_attention(self, block):
        raise NotImplementedError('replace_attention belongs to the KV-sparse caches, which are outside the weight-compression path')

    def block_forward(self, block, input_data=None):
        output = []
        if input_data is None:
            input_data = self.input['data']
        dev = next(block.parameters()).device
        for i in range(len(input_data)):
            input_data[i] = input_data[i].to(device=dev)
            kw = self.input['kwargs'][i]
            for k, v in kw.items():
                if torch.is_tensor(v):
                    kw[k] = v.to(device=dev)
                elif isinstance(v, tuple):
                    kw[k] = tuple(t.to(device=dev) if torch.is_tensor(t) else t for t in v)
            with torch.no_grad():
                out = block(input_data[i], **kw)
            output.append(out[0] if isinstance(out, tuple) else out)
        return output

    def block_opt(self, block):
        block = block.cuda()
        if not self.data_free:
            named_linears = self.model.get_block_linears(block)
            input_feat = defaultdict(list)
            handles = []
            self.block_init(block)
            if self.needs_input_feat:
                for name in named_linears:
                    handles.append(named_linears[name].register_forward_hook(
                        functools.partial(self.cache_input_hook, name=name, feat_dict=input_feat)))
            if not self.sparsity_out:
                self.input['data'] = self.block_forward(block)
            else:
                self.block_forward(block)
            for h in handles:
                h.remove()
            self.block_transform(block, input_feat, self.input['kwargs'])
            if self.sparsity_out:
                self.input['data'] = self.block_forward(block)
            del input_feat
        else:
            self.block_transform(block, {}, [])
        block = block.cpu()
        gc.collect()
        torch.cuda.empty_cache()

    def block_transform(self, block, input_feat, block_kwargs):
        subsets = self.model.get_subsets_in_block(block)
        for index, subset in enumerate(subsets):
            if not self.filter_subset(subset):
                continue
            subset_kwargs = block_kwargs if subset['has_kwargs'] else {}
            self.subset_transform(subset, input_feat, subset_kwargs)

    def filter_subset(self, subset):
        return True

    @torch.no_grad()
    def deploy(self, deploy_format):
        """The pruned weights already sit in the model's own Linear layers: there is no module to swap
        (base_blockwise_sparsification.py:182-186 only logs)."""
        return None

    @torch.no_grad()
    def copy_tokenizer(self, path):
        self.model.tokenizer.save_pretrained(path)

    @torch.no_grad()
    def save_model(self, path):
        """model + tokenizer, through the writer of the quantization base (save_pretrained where the model has it, safetensors
        + config.json otherwise)."""
        from ..quantization.base_blockwise_quantization import BaseBlockwiseQuantization
        BaseBlockwiseQuantization.save_model(self, path)
