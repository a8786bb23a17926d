"""Plain torch restatement of the sparsification arithmetic (llmc/compression/sparsification/wanda.py:16-56,
magnitude.py:24-31), for the tests: the reference's own expressions with a stable sort per group. Runs wherever its tensors
live; the kernel tests call it on CPU copies."""
import numpy as np
import torch


def bits(t):
    """integer view of a float tensor: comparisons that must see -0, NaN payloads and infinities"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def row_scale(act):
    """Wanda.get_row_scale (wanda.py:16-31) for a [n, T, K] (or [T, K]) act -> fp32 [K]"""
    if act.dim() == 2:
        act = act.unsqueeze(0)
    nsamples = act.shape[0]
    act = act.reshape((-1, act.shape[-1])).t().type(torch.float32)
    return torch.norm(act, p=2, dim=1) ** 2 / nsamples


def col_sqsum64(x):
    x = x.reshape(-1, x.shape[-1]).double()
    return (x * x).sum(0)


def col_sqsum_ordered(x, dt, waves=4, v=None):
    """llmc_col_sqsum's batch sum in the order include/llmc_hip.h promises, in numpy: x [N, K] (values of dt) -> fp32 [K]. The
    rows are cut into C = min(ceil(N / 64), max(1, 2048 // ceil(K / (64 v)))) chunks of ceil(N / C) rows, v the elements of a
    16-byte vector of dt; in a chunk starting at row r0, wave w sums the rows r0 + w, r0 + w + waves, ... from 0, the chunk's
    value is ((s0 + s1) + s2) + s3, the chunks are added in chunk order; every square and every add is rounded to fp32.
    `waves` and `v` are the ABI's 4 and 16 / sizeof(dt); another value is another order (the tests show that it differs)."""
    f = x.reshape(-1, x.shape[-1]).float().numpy()
    N, K = f.shape
    v = 16 // torch.empty(0, dtype=dt).element_size() if v is None else v
    C = min(-(-N // 64), max(1, 2048 // -(-K // (64 * v))))
    rpc = -(-N // C)
    total = None
    for r0 in range(0, C * rpc, rpc):
        r1 = min(r0 + rpc, N)
        chunk = None
        for w in range(waves):
            s = np.zeros(K, dtype=np.float32)
            for r in range(r0 + w, r1, waves):
                s = s + f[r] * f[r]
            chunk = s if chunk is None else chunk + s
        total = chunk if total is None else total + chunk
    return torch.from_numpy(total)


# the smallest shapes at which each rule of the order shows: fewer rows than waves (fp32: three squares of bf16 values add up
# exactly in any order); one chunk against two; ragged chunks in the 16-bit dtypes and in fp32; the one shape class where the
# 2048-block cap binds (C = 2, chunks of 65 rows)
SQSUM_ORDER_CASES = [(3, 8, 'f32'), (64, 8, 'bf16'), (65, 8, 'bf16'), (130, 64, 'bf16'), (130, 64, 'f16'), (300, 72, 'f32'),
                     (129, 262144, 'f32')]


def sqsum_order_input(N, K, dt, seed=31):
    """the seeded randn [N, K] of dt that the order tests share"""
    return torch.randn(N, K, generator=torch.Generator().manual_seed(seed)).to(dt)


def metric(w, scaler_row):
    a = torch.abs(w)
    if scaler_row is None:
        return a.float()
    return a * torch.sqrt(scaler_row.reshape((1, -1)))              # wanda.py:46-48: promotes to fp32


def prune_rows(w, scaler_row, n_prune, m=None):
    """-> (pruned copy of w, uint8 mask [R, K]). m None: per row (wanda.py:50-56); else groups of m consecutive columns."""
    R, K = w.shape
    m = K if m is None else m
    W_metric = metric(w, scaler_row).reshape(R * (K // m), m)
    W_mask = torch.zeros_like(W_metric) == 1
    sort_res = torch.sort(W_metric, dim=-1, stable=True)
    indices = sort_res[1][:, :n_prune]
    W_mask.scatter_(1, indices, True)
    W_mask = W_mask.reshape(R, K)
    out = w.clone()
    out[W_mask] = 0
    return out, W_mask.to(torch.uint8)


def magnitude_prune(w, kth):
    """magnitude.py:26-31 -> (pruned copy, thresh (0-dim, w's dtype), uint8 mask)"""
    W_metric = torch.abs(w)
    thresh = torch.sort(W_metric.flatten())[0][kth]
    W_mask = W_metric <= thresh
    out = w.clone()
    out[W_mask] = 0
    return out, thresh, W_mask.to(torch.uint8)


def selection_boundary64(metric64, n_prune, m=None):
    """fp64 metrics [R, K] -> (lo, hi) [R, K]: per group, the largest pruned and the smallest kept metric of the exact selection
    (lo = -inf when nothing is pruned, hi = +inf when everything is)."""
    R, K = metric64.shape
    m = K if m is None else m
    g = metric64.reshape(-1, m)
    s = torch.sort(g, dim=-1)[0]
    inf = torch.full((g.shape[0],), float('inf'), dtype=torch.float64, device=g.device)
    lo = s[:, n_prune - 1] if n_prune > 0 else -inf
    hi = s[:, n_prune] if n_prune < m else inf
    return (lo[:, None].expand(-1, m).reshape(R, K), hi[:, None].expand(-1, m).reshape(R, K))
