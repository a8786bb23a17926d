"""The attention-sink KV cache with llmc's surface (llmc/compression/sparsification/kvsparse.py:507-653): SinkKVCache ('SinkKV'),
StreamingLLM's window of `num_sink_tokens` first rows plus the most recent rows, `window_length` rows in all, registered in
KV_REGISTRY.

Once the window is full, every update of every layer drops the oldest rows behind the sink, rotates the kept keys again by the
number of rows they moved (their RoPE position becomes their place in the window) and appends the new rows. The reference does
that with a slice, a multiply by cos, a rotate_half built with a cat, a multiply by sin, an add and a cat of [sink, kept, new],
then slices and cats the values: about a dozen launches and five passes over [B, H, W, D]. The arithmetic cannot be folded: a
kept key is rotated on every step and rounded to the 16-bit dtype each time, so a key that survived k steps carries k
roundings, and one rotation of the original by the total shift gives other bits. What goes is the traffic: one kernel call per
update (llmc_kv_sink_update, csrc/kv_sink.hip) reads and writes every cached element once, keys and values together.

Two paths per layer, chosen at its first update:
  fused     keys and values each own a pair of [B * H, cap, D] buffers. While the window grows the new rows are appended in
            place; every shift writes into the other buffer of the pair (the kept rows move down, so a shift cannot run in
            place). update() returns [B, H, len, D] VIEWS of the current buffer: they stay valid until the SECOND following
            update of that layer, which writes the buffer they live in. Compare or clone them before that. The cost is twice the
            window's memory (the second buffer is allocated at the first shift).
  composed  everything the kernel refuses (LLMC_ENOTSUP: rot / 2 or D not whole 16-byte vectors, such as D = 72 in bf16) and any
            tensor that is not on the GPU: the reference's sequence written with torch ops, device-agnostic.
A refusal comes before anything is written; the layer then continues composed from the rows it holds.

All state is in attributes of this class: transformers' DynamicCache (subclassed when it imports, so that attention code's
isinstance checks pass) no longer has the _seen_tokens / key_cache / value_cache the reference leans on.

Kept from the reference as measured on it: with n + len == window_length the shifting branch runs, drops nothing and still
rotates the kept rows; a prompt longer than the window is stored whole and cut to the window by the first update after it.
Where it differs: n new rows >= window_length - num_sink_tokens in the shifting branch fail in the reference with a shape error
of the cat; here that is a ValueError naming both numbers, as is num_sink_tokens >= window_length at construction and a
rerotation table whose shape does not fit the kept keys."""
import torch

from llmc_amd import _ffi
from llmc_amd.utils.registry_factory import KV_REGISTRY

try:
    from transformers import DynamicCache as _CacheBase
except Exception:      # noqa: BLE001  (transformers is optional for the library; the cache works without it)
    _CacheBase = object


class _SinkLayer:
    """One layer's window: `fused` with two buffer pairs ([B * H, cap, D], `cur` the pair member that holds the n rows), or
    composed with two tensors [B, H, n, D]."""

    def __init__(self):
        self.fused = False
        self.n = 0
        self.shape = None           # (B, H, D) of the states
        self.kbuf, self.vbuf, self.cur = [None, None], [None, None], 0
        self.k = self.v = None

    def view(self, buf):
        B, H, D = self.shape
        return buf.view(B, H, buf.shape[1], D)[:, :, :self.n]


@KV_REGISTRY.register('SinkKV')
class SinkKVCache(_CacheBase):
    def __init__(self, num_hidden_layers, window_length, num_sink_tokens):
        super().__init__()
        if not 0 <= num_sink_tokens < window_length:
            raise ValueError(f'SinkKV: num_sink_tokens {num_sink_tokens} must be below window_length {window_length}')
        self.num_hidden_layers = num_hidden_layers
        self.window_length = window_length
        self.num_sink_tokens = num_sink_tokens
        self.cos_sin_rerotation_cache = {}
        self._cos_cache = None
        self._sin_cache = None
        self._fusable = True          # False: every layer composed (tools/bench_kvsparse.py times the two paths on one GPU)
        self._reset_states()

    # ---- state --------------------------------------------------------------------------------------------------------------
    def _reset_states(self):
        self._layers = {}
        self._seen = 0

    def get_seq_length(self, layer_idx=0):
        """The rows the layer holds (kvsparse.py:555-562): at most window_length once the first shift has run."""
        return self._layers[layer_idx].n if layer_idx in self._layers else 0

    def get_max_cache_shape(self):
        return self.window_length

    def get_mask_sizes(self, cache_position, layer_idx=0):
        """(kv_length, kv_offset) for transformers' mask construction: the rows update() will return for this query."""
        n = cache_position.shape[0] if torch.is_tensor(cache_position) else int(cache_position)
        held = self.get_seq_length(layer_idx)
        if held == 0 or held + n < self.window_length:
            return held + n, 0
        return self.window_length, 0

    # ---- rope bookkeeping (kvsparse.py:522-553, 582-596) -------------------------------------------------------------------------
    @staticmethod
    def _rotate_half(x):
        x1 = x[..., :x.shape[-1] // 2]
        x2 = x[..., x.shape[-1] // 2:]
        return torch.cat((-x2, x1), dim=-1)

    def _apply_key_rotary_pos_emb(self, key_states, cos, sin):
        return (key_states * cos) + (self._rotate_half(key_states) * sin)

    def _get_rerotation_cos_sin(self, key_states, cos, sin):
        """The tables that turn a key at window place sink + n + i into one at sink + i: cos / sin of the difference angle,
        computed in fp32, cast to the key dtype, [1, window - sink - n, rot]; cached per n = the number of new rows."""
        n = key_states.shape[-2]
        if n not in self.cos_sin_rerotation_cache:
            cos = cos.to(torch.float32)
            sin = sin.to(torch.float32)
            original_cos = cos[self.num_sink_tokens + n:]
            shifted_cos = cos[self.num_sink_tokens:-n]
            original_sin = sin[self.num_sink_tokens + n:]
            shifted_sin = sin[self.num_sink_tokens:-n]
            rerotation_cos = original_cos * shifted_cos + original_sin * shifted_sin
            rerotation_sin = -original_sin * shifted_cos + original_cos * shifted_sin
            self.cos_sin_rerotation_cache[n] = (rerotation_cos.to(key_states.dtype).unsqueeze(0),
                                                rerotation_sin.to(key_states.dtype).unsqueeze(0))
        return self.cos_sin_rerotation_cache[n]

    def _note_cos_sin(self, cos, sin):
        if cos.dim() == 2:
            self._cos_cache = cos
            self._sin_cache = sin
        elif self._cos_cache is None:
            self._cos_cache = cos[0, ...]
            self._sin_cache = sin[0, ...]
        elif self._cos_cache.shape[0] < self.window_length:
            self._cos_cache = torch.cat([self._cos_cache, cos[0, ...]], dim=0)
            self._sin_cache = torch.cat([self._sin_cache, sin[0, ...]], dim=0)

    # ---- the fused path -----------------------------------------------------------------------------------------------------------
    def _launch(self, L, src, dst, k_new, v_new, n_sink, keep_from, n_keep, dst_row0, rot, cos, sin):
        """One llmc_kv_sink_update for keys and values. Raises NotImplementedError when the kernel refuses, before anything is
        written."""
        B, H, D = L.shape
        vec = 16 // k_new.element_size()

        def ok(t):      # what the kernel reads in place: unit stride along D, every row 16-byte aligned
            return t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all(s % vec == 0 for s in t.stride()[:3])
        if not (ok(k_new) and ok(v_new) and v_new.stride() == k_new.stride()):
            k_new, v_new = k_new.contiguous(), v_new.contiguous()
        if cos is not None:
            cos, sin = cos.to(k_new.device).contiguous(), sin.to(k_new.device).contiguous()
        ks, vs = (L.kbuf[src], L.vbuf[src]) if src is not None else (None, None)
        _ffi.check(_ffi.lib().llmc_kv_sink_update(
            _ffi.dt(k_new), B, H, D, n_sink, keep_from, n_keep, k_new.shape[-2], ks.shape[1] if ks is not None else 0,
            L.kbuf[dst].shape[1], dst_row0, rot, _ffi.ptr(cos), _ffi.ptr(sin), _ffi.ptr(ks), _ffi.ptr(L.kbuf[dst]), _ffi.ptr(k_new),
            _ffi.ptr(vs), _ffi.ptr(L.vbuf[dst]), _ffi.ptr(v_new), k_new.stride(0), k_new.stride(1), k_new.stride(2),
            _ffi.stream()), 'llmc_kv_sink_update')

    @staticmethod
    def _buffers(L, i, cap, like):
        B, H, D = L.shape
        L.kbuf[i] = torch.empty((B * H, cap, D), dtype=like.dtype, device=like.device)
        L.vbuf[i] = torch.empty_like(L.kbuf[i])

    def _new_layer(self, key_states, value_states):
        """A layer at its first update: fused when the states are on the GPU and the kernel takes them."""
        L = _SinkLayer()
        B, H, T, D = key_states.shape
        L.shape = (B, H, D)
        if self._fusable and key_states.is_cuda and value_states.is_cuda and key_states.dtype in _ffi._DT and value_states.dtype == key_states.dtype \
                and value_states.shape == key_states.shape:
            _ffi.require_gpu(key_states, value_states)
            self._buffers(L, 0, max(self.window_length, T), key_states)       # a prompt longer than the window is stored whole
            try:
                self._launch(L, None, 0, key_states, value_states, 0, 0, 0, 0, 0, None, None)
                L.fused = True
            except NotImplementedError:          # LLMC_ENOTSUP, before anything was launched: this layer is composed
                L.kbuf, L.vbuf = [None, None], [None, None]
        if not L.fused:
            L.k, L.v = key_states, value_states
        L.n = T
        return L

    def _to_composed(self, L):
        """The kernel refused a later update (rot / 2 that is not whole vectors shows at the first shift): go on from the held rows."""
        L.k, L.v = L.view(L.kbuf[L.cur]), L.view(L.vbuf[L.cur])
        L.kbuf, L.vbuf, L.fused = [None, None], [None, None], False

    # ---- update (kvsparse.py:569-648) ---------------------------------------------------------------------------------------------
    def update(self, key_states, value_states, layer_idx, cache_kwargs=None):
        cache_kwargs = cache_kwargs or {}
        sin = cache_kwargs.get('sin')
        cos = cache_kwargs.get('cos')
        partial_rotation_size = cache_kwargs.get('partial_rotation_size')
        using_rope = cos is not None and sin is not None
        n = key_states.shape[-2]
        if layer_idx == 0:
            self._seen += n
            if using_rope:
                self._note_cos_sin(cos, sin)

        if layer_idx not in self._layers:                                   # empty
            L = self._layers[layer_idx] = self._new_layer(key_states, value_states)
        elif n + self._layers[layer_idx].n < self.window_length:            # growing
            L = self._layers[layer_idx]
            if L.fused:
                try:
                    self._launch(L, None, L.cur, key_states, value_states, 0, 0, 0, L.n, 0, None, None)
                except NotImplementedError:
                    self._to_composed(L)
            if not L.fused:
                L.k = torch.cat([L.k, key_states], dim=-2)
                L.v = torch.cat([L.v, value_states], dim=-2)
            L.n += n
        else:                                                               # shifting
            L = self._layers[layer_idx]
            W, sink = self.window_length, self.num_sink_tokens
            n_keep = W - sink - n
            if n_keep <= 0:
                raise ValueError(f'SinkKV: {n} new rows do not fit behind the sink: they must be fewer than window_length - '
                                 f'num_sink_tokens = {W} - {sink} = {W - sink}')
            rot, rcos, rsin = 0, None, None
            if using_rope:
                rcos, rsin = self._get_rerotation_cos_sin(key_states, self._cos_cache[:W], self._sin_cache[:W])
                rot = key_states.shape[-1] if partial_rotation_size is None else int(partial_rotation_size)
                if tuple(rcos.shape) != (1, n_keep, rot) or rot > key_states.shape[-1]:
                    raise ValueError(f'SinkKV: the rerotation tables are {tuple(rcos.shape)}, the kept keys need (1, {n_keep}, {rot}): '
                                     f'cos / sin must cover window_length = {W} positions and the rotated width')
            if L.fused:
                dst = 1 - L.cur
                if L.kbuf[dst] is None:
                    self._buffers(L, dst, W, key_states)
                try:
                    self._launch(L, L.cur, dst, key_states, value_states, sink, L.n - n_keep, n_keep, 0, rot, rcos, rsin)
                    L.cur = dst
                except NotImplementedError:
                    self._to_composed(L)
            if not L.fused:
                keys_to_keep = L.k[:, :, -n_keep:]
                if using_rope:
                    if partial_rotation_size is not None:
                        keys_to_keep, keys_pass = keys_to_keep[..., :rot], keys_to_keep[..., rot:]
                    keys_to_keep = self._apply_key_rotary_pos_emb(keys_to_keep, rcos, rsin)
                    if partial_rotation_size is not None:
                        keys_to_keep = torch.cat((keys_to_keep, keys_pass), dim=-1)
                L.k = torch.cat([L.k[:, :, :sink], keys_to_keep, key_states], dim=-2)
                L.v = torch.cat([L.v[:, :, :sink], L.v[:, :, -n_keep:], value_states], dim=-2)
            L.n = W
        if L.fused:
            return L.view(L.kbuf[L.cur]), L.view(L.vbuf[L.cur])
        return L.k, L.v
