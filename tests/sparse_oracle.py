"""Plain torch restatement of the sparsification arithmetic (llmc/compression/sparsification/wanda.py:16-56,
magnitude.py:24-31), for the tests: the reference's own expressions with a stable sort per group. Runs wherever its tensors
live; the kernel tests call it on CPU copies."""
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
