"""Quantized KV caches with llmc's surface (llmc/compression/quantization/kvquant.py): NaiveQuantKVCache ('Naive') and
KiviQuantKVCache ('Kivi'), registered in KV_REGISTRY.

The reference's decode step is dequant(whole cache) -> cat(new token) -> contiguous -> amax / amin -> quant(whole cache) on codes
kept as 16-bit floats: about ten passes over [B, H, T, D] per layer and step, and no memory saved. The requantization cannot be
dropped: a stored bf16 code re-derived from its own dequantized value is not always the same code. Here the codes live one per
byte in per-layer stores [B * H, capacity, D] that double when they run full, qparams beside them, and one kernel call per update
(llmc_kv_cache_update, csrc/kv_cache.hip) does keys and values together: 1 byte read and 2 + 1 bytes written per stored element,
the reference's bits.

Two paths per layer, chosen at its prefill:
  fused     int-quant, bit <= 8, per_token / per_group, round_zp, calib_algo minmax, a group of 16 bytes times a power of two
  composed  everything the kernel refuses (llmc_kv_cache_update returns LLMC_ENOTSUP: D = 80 per_token, per_tensor, round_zp =
            False, bit > 8 ...) and quant_type float-quant: the reference's sequence written with the quantizer's own methods
            (reshape_tensor, get_tensor_range, get_qparams, quant, dequant, restore_tensor), float codes as the reference keeps
            them. Slow but complete.

All state is in attributes of this class: transformers' DynamicCache (subclassed when it imports, so that attention code's
isinstance checks pass) no longer has the _seen_tokens / key_cache / value_cache the reference leans on. `use_org_kv = True`
(deploy formats origin_float and fake_quant_wo_kv) keeps a plain concatenating cache, also local.

static=True (per-tensor qparams calibrated over the prompts) raises NotImplementedError: the reference's own config route to
it cannot be constructed (base_blockwise_quantization.py:206 calls dict.update with an int).
"""
import torch

from llmc_amd import _ffi
from llmc_amd.utils.registry_factory import KV_REGISTRY

from .quant import FloatQuantizer, IntegerQuantizer

try:
    from transformers import DynamicCache as _CacheBase
except Exception:      # noqa: BLE001  (transformers is optional for the library; the caches work without it)
    _CacheBase = object


def _get(cfg, key, default=None):
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


class _Store:
    """The fused path's store of one tensor of one layer: codes [B * H, cap, D] int8 / uint8, scales and zeros
    [B * H, cap, D / g] of the tensor dtype. Doubles in capacity when a row count exceeds it."""

    def __init__(self, BH, cap, D, gpr, dtype, device, signed, sym):
        self.BH, self.cap, self.D, self.gpr, self.sym = BH, cap, D, gpr, sym
        self.codes = torch.empty((BH, cap, D), dtype=torch.int8 if signed else torch.uint8, device=device)
        self.scales = torch.empty((BH, cap, gpr), dtype=dtype, device=device)
        self.zeros = None if sym else torch.empty((BH, cap, gpr), dtype=dtype, device=device)

    def reserve(self, rows, used):
        if rows <= self.cap:
            return
        cap = self.cap
        while cap < rows:
            cap *= 2
        for name in ('codes', 'scales', 'zeros'):
            old = getattr(self, name)
            if old is None:
                continue
            new = torch.empty((self.BH, cap, old.shape[2]), dtype=old.dtype, device=old.device)
            new[:, :used] = old[:, :used]
            setattr(self, name, new)
        self.cap = cap


class _Layer:
    """One layer's cache: `fused` with two _Store, or composed with the reference's two dicts; T stored rows; Kivi's residual."""

    def __init__(self):
        self.fused = False
        self.k = self.v = None
        self.T = 0
        self.shape = None           # (B, H, D) of the states
        self.g = None
        self.resid_k = self.resid_v = None


@KV_REGISTRY.register('Naive')
class NaiveQuantKVCache(_CacheBase):
    def __init__(self, quant_type, kvquant_cfg, num_hidden_layers, num_samples=128, bsz=1, initial_capacity=256):
        super().__init__()
        granularity = _get(kvquant_cfg, 'granularity')
        assert granularity in ['per_token', 'per_tensor', 'per_group']
        self.num_hidden_layers, self.num_samples, self.bsz = num_hidden_layers, num_samples, bsz
        self.static = _get(kvquant_cfg, 'static', False)
        if self.static:
            raise NotImplementedError(
                'KV-cache quantization with static qparams (kvcache.static / act.static) is outside the hot path: the '
                "reference's own config route to it cannot be constructed (base_blockwise_quantization.py:206 calls "
                'dict.update with an int)')
        qcfg = {k: v for k, v in dict(kvquant_cfg).items() if k not in ('method', 'quant_type', 'special')}
        if quant_type == 'int-quant':
            self.kvquantizer = IntegerQuantizer(**qcfg)
        elif quant_type == 'float-quant':
            self.kvquantizer = FloatQuantizer(**qcfg)
        else:
            raise ValueError(f'unknown quant_type {quant_type}')
        self.quant_type = quant_type
        self.kvquant_cfg = kvquant_cfg
        self.calib = False
        self.use_org_kv = False
        self.initial_capacity = max(1, int(initial_capacity))
        q = self.kvquantizer
        # what the kernel can take, as far as the configuration says; the geometry is the kernel's to refuse (LLMC_ENOTSUP)
        self._fusable = (quant_type == 'int-quant' and granularity in ('per_token', 'per_group') and q.round_zp
                         and q.calib_algo == 'minmax' and float(q.qmin) >= -128 and float(q.qmax) <= (127 if q.qmin < 0 else 255))
        self._reset_states()

    # ---- state --------------------------------------------------------------------------------------------------------------
    def _reset_states(self):
        self._layers = {}
        self._org = {}
        self._seen = 0

    def get_seq_length(self, layer_idx=0):
        if self.use_org_kv:
            return self._org[layer_idx][0].shape[-2] if layer_idx in self._org else 0
        if layer_idx not in self._layers:
            return 0
        return self._seen if layer_idx == 0 else self._seen - 1

    def get_mask_sizes(self, cache_position, layer_idx=0):
        """(kv_length, kv_offset) for transformers' mask construction: the rows already held plus the query's."""
        n = cache_position.shape[0] if torch.is_tensor(cache_position) else int(cache_position)
        if self.use_org_kv:
            return self.get_seq_length(layer_idx) + n, 0
        return (self._seen if layer_idx in self._layers else 0) + n, 0

    def _update_org(self, key_states, value_states, layer_idx):
        if layer_idx in self._org:
            k, v = self._org[layer_idx]
            key_states, value_states = torch.cat([k, key_states], dim=-2), torch.cat([v, value_states], dim=-2)
        self._org[layer_idx] = (key_states, value_states)
        return key_states, value_states

    # ---- the composed path: the reference's _quantize / _dequantize (kvquant.py:136-186) ------------------------------------------
    def _quantize(self, tensor):
        q = self.kvquantizer
        org_shape = tensor.shape
        tensor = q.reshape_tensor(tensor)
        tensor_range = q.get_tensor_range(tensor, {})
        scales, zeros, qmax, qmin = q.get_qparams(tensor_range, tensor.device)
        q_tensor = q.quant(tensor, scales, zeros, qmax, qmin)
        if self.quant_type == 'int-quant':
            # the reference's codes come out of torch ops on the tensor: a 0-dim qparam does not promote them
            q_tensor = q_tensor.to(torch.result_type(tensor, scales))
        return {'q_tensor': q.restore_tensor(q_tensor, org_shape), 'scales': scales, 'zeros': zeros}

    def _dequantize(self, q_tensors):
        q = self.kvquantizer
        q_tensor, scales, zeros = q_tensors['q_tensor'], q_tensors['scales'], q_tensors['zeros']
        org_shape = q_tensor.shape
        q_tensor = q.reshape_tensor(q_tensor)
        if scales.dim() == 0 and q_tensor.dim() > 0:
            # per_tensor: the reference's CPU ops take a 0-dim operand as a scalar of its own precision. A 0-dim tensor on the
            # host is the same to a GPU op; one on the device would be cast to the tensor dtype first.
            scales = scales.cpu()
            zeros = zeros.cpu() if torch.is_tensor(zeros) else zeros
        return q.restore_tensor(q.dequant(q_tensor, scales, zeros), org_shape)

    # ---- the fused path -----------------------------------------------------------------------------------------------------------
    def _launch(self, L, k_new, v_new, T_old, flags, want_out):
        """One llmc_kv_cache_update for keys and values (values may be None). Raises NotImplementedError when the kernel
        refuses, before anything is written. Returns (k_out, v_out)."""
        B, H, D = L.shape
        n_new = 0 if k_new is None else k_new.shape[-2]
        if k_new is not None:
            vec = 16 // k_new.element_size()

            def ok(t):      # what the kernel reads in place: unit stride along D, every row 16-byte aligned
                return t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all(s % vec == 0 for s in t.stride()[:3])
            if not (ok(k_new) and (v_new is None or (ok(v_new) and v_new.stride() == k_new.stride()))):
                k_new = k_new.contiguous()
                v_new = None if v_new is None else v_new.contiguous()
        ref = k_new if k_new is not None else L.k.scales
        T = T_old + n_new
        k_out = v_out = None
        if want_out:
            k_out = torch.empty((B, H, T, D), dtype=ref.dtype, device=ref.device)
            v_out = torch.empty_like(k_out) if L.v is not None else None
        q = self.kvquantizer
        sb, sh, st = (k_new.stride(0), k_new.stride(1), k_new.stride(2)) if k_new is not None else (0, 0, 0)
        _ffi.check(_ffi.lib().llmc_kv_cache_update(
            _ffi.dt(L.k.scales), B, H, T_old, n_new, L.k.cap, D, L.g, int(q.sym), int(q.round_zp), float(q.qmin), float(q.qmax),
            flags, _ffi.ptr(L.k.codes), _ffi.ptr(L.k.scales), _ffi.ptr(L.k.zeros), _ffi.ptr(k_new), _ffi.ptr(k_out),
            _ffi.ptr(L.v.codes if L.v else None), _ffi.ptr(L.v.scales if L.v else None), _ffi.ptr(L.v.zeros if L.v else None),
            _ffi.ptr(v_new if L.v else None), _ffi.ptr(v_out), sb, sh, st, _ffi.stream()), 'llmc_kv_cache_update')
        return k_out, v_out

    def _group(self, D):
        q = self.kvquantizer
        if q.granularity == 'per_group' and D >= q.group_size:
            if D % q.group_size != 0:
                raise ValueError(f'Dimension {D} not divisible by group size {q.group_size}')
            return q.group_size
        return D

    def _new_layer(self, key_states, value_states):
        """A layer at its prefill: fused when the configuration and the kernel allow it."""
        L = _Layer()
        B, H, T, D = key_states.shape
        L.shape = (B, H, D)
        if self._fusable and key_states.dtype in _ffi._DT:
            _ffi.require_gpu(key_states, value_states)
            L.g = self._group(D)
            q = self.kvquantizer
            cap = self.initial_capacity
            while cap < T:
                cap *= 2
            mk = lambda: _Store(B * H, cap, D, D // L.g, key_states.dtype, key_states.device, bool(q.qmin < 0), q.sym)  # noqa: E731
            L.k, L.v = mk(), (mk() if value_states is not None else None)
            L.fused = True
        return L

    def _append_fused(self, L, k_new, v_new, flags, want_out=True):
        rows = L.T + k_new.shape[-2]
        for s in (L.k, L.v):
            if s is not None:
                s.reserve(rows, L.T)
        out = self._launch(L, k_new, v_new, L.T, flags, want_out)
        L.T = rows
        return out

    def _prefill(self, key_states, value_states, layer_idx, fake):
        """Quantize the prompt's states into a new layer. Returns what the fused kernel wrote as `out` (None on the composed
        path or when `fake` is False)."""
        L = self._new_layer(key_states, value_states)
        out = None
        if L.fused:
            try:
                flags = _ffi.KV_REQUANT | (_ffi.KV_NEW_FAKE if fake else 0)
                out = self._append_fused(L, key_states, value_states, flags, want_out=fake)
            except NotImplementedError:          # LLMC_ENOTSUP, before anything was launched: this layer is composed
                L = _Layer()
                L.shape = (key_states.shape[0], key_states.shape[1], key_states.shape[3])
        if not L.fused:
            L.k = self._quantize(key_states.contiguous())
            L.v = self._quantize(value_states.contiguous()) if value_states is not None else None
            L.T = key_states.shape[-2]
        self._layers[layer_idx] = L
        return L, out

    # ---- update (kvquant.py:44-87) ----------------------------------------------------------------------------------------------
    def update(self, key_states, value_states, layer_idx, cache_kwargs=None):
        if self.use_org_kv:
            return self._update_org(key_states, value_states, layer_idx)
        if layer_idx == 0:
            self._seen += key_states.shape[-2]
        if layer_idx not in self._layers:
            L, out = self._prefill(key_states, value_states, layer_idx, fake=True)
            if L.fused:
                return out
            return self._dequantize(L.k), (self._dequantize(L.v) if L.v is not None else None)
        L = self._layers[layer_idx]
        if L.fused:
            return self._append_fused(L, key_states, value_states, _ffi.KV_REQUANT)
        keys = torch.cat([self._dequantize(L.k), key_states], dim=-2)
        L.k = self._quantize(keys.contiguous())
        values = None
        if L.v is not None:
            values = torch.cat([self._dequantize(L.v), value_states], dim=-2)
            L.v = self._quantize(values.contiguous())
        L.T = keys.shape[-2]
        return keys, values

    # ---- what the reference keeps per layer, in its dtypes and shapes ----------------------------------------------------------------
    def quantized(self, layer_idx, is_key=True):
        """{'q_tensor', 'scales', 'zeros'} of a layer's keys or values as the reference's _quantized_*_cache[layer_idx] holds
        them: codes in the tensor dtype [B, H, T, D]; scales [B, H, T, 1] (per_token), [B * H * T * D / g, 1] (per_group) or
        0-dim (per_tensor); zeros like scales, a 0-dim 0.0 when symmetric."""
        L = self._layers[layer_idx]
        s = L.k if is_key else L.v
        if not L.fused:
            return s
        B, H, D = L.shape
        T = L.T
        q = self.kvquantizer
        grouped = q.granularity == 'per_group' and D >= q.group_size       # reshape_tensor flattened the rows into groups
        shp = (-1, 1) if grouped else (B, H, T, 1)
        return {'q_tensor': s.codes[:, :T].to(s.scales.dtype).reshape(B, H, T, D),
                'scales': s.scales[:, :T].reshape(shp),
                'zeros': torch.tensor(0.0) if s.sym else s.zeros[:, :T].reshape(shp)}


@KV_REGISTRY.register('Kivi')
class KiviQuantKVCache(NaiveQuantKVCache):
    def __init__(self, quant_type, kvquant_cfg, num_hidden_layers, num_samples=128, bsz=1, initial_capacity=256):
        if _get(kvquant_cfg, 'static', False):
            raise NotImplementedError('Only support dynamic quantization for KIVI (kvquant.py:230): a static KV-cache section is '
                                      'refused')
        super().__init__(quant_type, kvquant_cfg, num_hidden_layers, num_samples, bsz, initial_capacity=initial_capacity)
        self.residual_length = _get(kvquant_cfg, 'residual_length', 128)

    def residual(self, layer_idx, is_key=True):
        """The unquantized rows behind the store (None right after the prefill or a flush)."""
        L = self._layers[layer_idx]
        return L.resid_k if is_key else L.resid_v

    def update(self, key_states, value_states, layer_idx, cache_kwargs=None):
        """kvquant.py:233-289: the prompt is quantized and returned raw; later rows wait unquantized in a residual, and when
        it is about to reach residual_length rows the whole of cat(dequant(store), residual, new) is quantized again."""
        if self.use_org_kv:
            return self._update_org(key_states, value_states, layer_idx)
        if layer_idx == 0:
            self._seen += key_states.shape[-2]
        if layer_idx not in self._layers:
            self._prefill(key_states, value_states, layer_idx, fake=False)
            return key_states, value_states
        L = self._layers[layer_idx]
        # the reference's residual is a 1-D empty tensor after the prefill and after a flush, which never triggers the next one
        flush = L.resid_k is not None and L.resid_k.shape[-2] + 1 >= self.residual_length
        k_new = key_states if L.resid_k is None else torch.cat([L.resid_k, key_states], dim=-2)
        v_new = value_states if L.resid_v is None else torch.cat([L.resid_v, value_states], dim=-2)
        if value_states is None:
            v_new = None
        if L.fused:
            if flush:
                keys, values = self._append_fused(L, k_new, v_new, _ffi.KV_REQUANT)
            else:
                keys, values = self._launch(L, k_new, v_new, L.T, 0, True)
        else:
            keys = torch.cat([self._dequantize(L.k), k_new], dim=-2)
            values = None if v_new is None else torch.cat([self._dequantize(L.v), v_new], dim=-2)
            if flush:
                L.k, L.v = self._quantize(keys.contiguous()), (None if values is None else self._quantize(values.contiguous()))
                L.T = keys.shape[-2]
        L.resid_k, L.resid_v = (None, None) if flush else (k_new, v_new)
        return keys, values
