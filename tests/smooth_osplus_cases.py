"""The small modules and loaders the SmoothQuant / OS+ golden cases share: tools/make_golden_smooth_osplus.py builds the cases
from these classes, the tests and tools/osplus_parity.py rebuild them from tests/golden/smooth_osplus.npz. Test infrastructure."""
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'smooth_osplus.npz')
DT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}


class GatedMLP(torch.nn.Module):
    def __init__(self, K, R, bias):
        super().__init__()
        self.gate_proj = torch.nn.Linear(K, R, bias=bias)
        self.up_proj = torch.nn.Linear(K, R, bias=bias)
        self.down_proj = torch.nn.Linear(R, K, bias=bias)

    def forward(self, x):
        return self.down_proj(torch.nn.functional.silu(self.gate_proj(x)) * self.up_proj(x))

    def searched(self):
        return [self.gate_proj, self.up_proj]


class Stack(torch.nn.Module):
    """attention-free stack: fc1 -> gelu -> fc2 -> gelu -> fc3; fc1 is the searched layer"""

    def __init__(self, K, R, bias):
        super().__init__()
        self.fc1 = torch.nn.Linear(K, R, bias=bias)
        self.fc2 = torch.nn.Linear(R, R, bias=bias)
        self.fc3 = torch.nn.Linear(R, K, bias=bias)

    def forward(self, x):
        g = torch.nn.functional.gelu
        return self.fc3(g(self.fc2(g(self.fc1(x)))))

    def searched(self):
        return [self.fc1]


class OptShaped(torch.nn.Module):
    """the MLP half of an OPT decoder layer: LayerNorm (with bias) -> fc1 (bias) -> relu -> fc2 (bias), residual"""

    def __init__(self, H, F):
        super().__init__()
        self.final_layer_norm = torch.nn.LayerNorm(H)
        self.fc1 = torch.nn.Linear(H, F)
        self.fc2 = torch.nn.Linear(F, H)

    def forward(self, x):
        return x + self.fc2(torch.relu(self.fc1(self.final_layer_norm(x))))


def gold():
    return np.load(GOLD)


def from_bits(a, dt):
    """the tensor whose bit pattern the golden stores (uint16 for 16-bit dtypes, uint32 for fp32)"""
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32).copy()).view(torch.float32)
    return torch.from_numpy(a.view(np.int16).copy()).view(DT[dt])


def bits_of(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32)
    return t.view(torch.int16).numpy().view(np.uint16)


def load_state(z, prefix, module, dt):
    sd = {k[len(prefix):]: from_bits(z[k], dt) for k in z.files if k.startswith(prefix)}
    module.to(DT[dt])
    module.load_state_dict(sd)
    return module


def os_case(z, name):
    """-> (cfg dict, dt name, module on the CPU with the case's weights, x)"""
    cfg = json.loads(str(z[name + '/cfg']))
    dt = str(z[name + '/dt'])
    cls = GatedMLP if cfg['module'] == 'mlp' else Stack
    mod = load_state(z, name + '/sd/', cls(cfg['K'], cfg['R'], cfg['has_bias']), dt)
    x = from_bits(z[name + '/x_bits'], dt).reshape(tuple(int(v) for v in z[name + '/x_shape']))
    return cfg, dt, mod, x


def quant_section(cfg):
    def one(kind, bit, sym, gran):
        d = dict(bit=bit, symmetric=sym, granularity=gran)
        if kind == 'float':
            d.update(quant_type='float-quant', use_qtorch=True)
        return d
    return {'method': 'OsPlus', 'weight': one(*cfg['weight']), 'act': one(*cfg['act'])}


class OneBlockModel:
    """what the host classes ask of a model adapter when a test drives a subset search by hand"""

    def __init__(self, block, has_bias, config=None):
        self.block, self._has_bias = block, has_bias
        self.model_config = SimpleNamespace(**(config or {}))

    def get_blocks(self):
        return [self.block]

    def has_bias(self):
        return self._has_bias

    def get_num_attention_heads(self):
        return self.model_config.num_attention_heads

    def get_model_config(self):
        return self.model_config
