"""What the ShortGPT end-to-end tests share: a six-block ToyModel whose blocks differ in influence by fixed factors, and the
scores of its blocks computed apart from the class (the blocks' own forward, then tests/shortgpt_oracle.py)."""
import numpy as np
import torch

import shortgpt_oracle as O
from toy_model import ToyModel, calib_input

# down_proj of block b is multiplied by FACTORS[b]: a block's change to the residual stream, and with it its score, scales with
# it, so the ranking has gaps far above any rounding
FACTORS = (1.3, 0.25, 2.0, 0.8, 4.5, 3.0)
DT_NAME = {torch.bfloat16: 'bf16', torch.float16: 'f16', torch.float32: 'f32'}


def toy(dtype):
    model = ToyModel(n_blocks=len(FACTORS), dtype=dtype)
    for block, f in zip(model.model.blocks, FACTORS):
        block.down_proj.weight.data *= f
    return model, calib_input(model)


def features(model, inp, device):
    """per block the list of (input, output) batches of the dense flow, run apart from the class on `device`"""
    data = [t.to(device) for t in inp['data']]
    out = []
    with torch.no_grad():
        for block in model.model.blocks:
            block.to(device)
            nxt = [block(t) for t in data]
            out.append(list(zip(data, nxt)))
            data = nxt
            block.cpu()
    return out


def scores(feats, dt, exact):
    """per block: the fp64 truth's total (exact) or the oracle's folded total in the kernel's order"""
    res = []
    for pairs in feats:
        tot = None
        for x, y in pairs:
            x, y = x.float().cpu().numpy().reshape(-1, x.shape[-1]), y.float().cpu().numpy().reshape(-1, y.shape[-1])
            if exact:
                tot = (0.0 if tot is None else tot) + O.truth(x, y).sum()
            else:
                tot = O.total(O.block_influence(x, y, dt), tot)
        res.append(tot)
    return np.array(res, np.float64)
