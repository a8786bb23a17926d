"""Functional wrappers over the pruning kernels of libllmc_hip.so (csrc/prune.hip): what Wanda and Magnitude run per layer.

col_sqsum          per-column sum of squares of the calibration activations, folded into a running fp32 [K] buffer
                   (Wanda.get_row_scale, wanda.py:27-31), optionally divided by the number of samples.
prune_rows         in place: in every group of m consecutive columns of a row, the n_prune elements of smallest
                   |w| * sqrt(scaler_row) become +0 (wanda.py:46-56 for m == K; n:m for m in {2, 4, 8, 16}). Bit for bit the
                   reference's stable sort + scatter + masked assignment.
prune_rows_composed  that sequence from torch ops on the device: a stable sort per group, the indices scattered into a boolean
                   mask, a masked assignment. It is what the tests compare the kernel against and what prune_rows falls
                   back to, announced on stderr, for a row too long to stay resident (LLMC_ENOTSUP: K > 32768 with m == K).
magnitude_prune    in place: the global |w| threshold of rank kth and w[|w| <= thresh] = 0 (magnitude.py:26-31).
path               the launch path prune_rows takes, by name (a pure host call).
sparsegpt_prune    SparseGPT's blocked column loop on an upper factor of the inverse Hessian (csrc/sparsegpt_loop.hip): mask by
                   score w^2 / d^2, the pruning error fed to the later columns. Timings: profiles/sparsegpt.txt.
block_influence    ShortGPT's per-token 1 - cos(input, output) of a block and its fp64 sum, one streaming pass
                   (csrc/block_influence.hip); block_influence_composed is the same quantity row-wise from torch ops, on any
                   device. Timings: profiles/shortgpt.txt.

Dispatch: the kernel measured 0.04x - 0.15x of the composition's time per row and 0.002x - 0.007x for 2:4 at every shape timed
(bf16 4096 x 4096, 1024 x 4096, 14336 x 4096, 4096 x 14336; profiles/prune.txt, tools/bench_prune.py), magnitude_prune 0.05x and
col_sqsum 0.13x at 262144 x 4096, with no overlap of the min..max ranges: no shape class is routed to the composition for speed.
The composition only takes the rows the kernel refuses."""
import sys

import torch

from llmc_amd import _ffi

PATH_NAMES = ('wave', 'block256', 'block1024', 'scalar', 'nm', 'nm_scalar')
MAX_RESIDENT_K = 32768          # csrc/prune.hip: PR_MAX_K
NM_GROUPS = (2, 4, 8, 16)

_FALLBACK_SEEN = set()


def _operand(w):
    """does the weight lie as the kernels take it (unit column stride, row stride >= K)? Anything else is copied"""
    return w.dim() == 2 and w.stride(1) == 1 and w.stride(0) >= w.shape[1]


def _check_w(w, what):
    if w.dim() != 2 or w.shape[0] < 1 or w.shape[1] < 1:
        raise ValueError(f'{what} takes a non-empty 2-D [R, K] weight')


def _check_groups(w, scaler_row, n_prune, m):
    _check_w(w, 'prune_rows')
    K = w.shape[1]
    m = K if m is None else int(m)
    if m != K and m not in NM_GROUPS:
        raise NotImplementedError(f'prune_rows: m is K (per row) or one of {NM_GROUPS} (n:m), not {m}')
    if K % m:
        raise ValueError(f'prune_rows: m = {m} does not divide K = {K}')
    if not 0 <= int(n_prune) <= m:
        raise ValueError(f'prune_rows: n_prune = {n_prune} outside [0, {m}]')
    if scaler_row is not None and (scaler_row.dim() != 1 or scaler_row.shape[0] != K):
        raise ValueError(f'prune_rows: scaler_row must be [K] = [{K}], got {tuple(scaler_row.shape)}')
    return m


def col_sqsum(x, acc=None, init=True, nsamples=None):
    """x [..., K] on the GPU -> acc fp32 [K] = sum over all leading positions of fp32(x)^2 (init) or acc + that sum (init
    False: acc is updated in place). With nsamples: -> (acc, acc / float(nsamples)). x is copied only if it is not contiguous."""
    _ffi.require_gpu(x, acc)
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError('col_sqsum takes a non-empty [..., K] tensor')
    K = x.shape[-1]
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    N = x2.shape[0]
    if acc is None:
        if not init:
            raise ValueError('col_sqsum: folding (init=False) needs the running buffer `acc`')
        acc = torch.empty(K, dtype=torch.float32, device=x.device)
    elif acc.dtype != torch.float32 or acc.shape != (K,) or not acc.is_contiguous():
        raise ValueError(f'col_sqsum: acc must be a contiguous fp32 [{K}] tensor')
    out = torch.empty(K, dtype=torch.float32, device=x.device) if nsamples is not None else None
    L = _ffi.lib()
    dt = _ffi.dt(x2)
    ws = _ffi.workspace(L.llmc_col_sqsum_ws_bytes(N, K, dt), x.device)
    _ffi.check(L.llmc_col_sqsum(_ffi.ptr(x2), dt, N, K, int(bool(init)), _ffi.ptr(acc), _ffi.ptr(out),
                                int(nsamples) if nsamples is not None else 1, _ffi.ptr(ws), _ffi.stream()), 'llmc_col_sqsum')
    return (acc, out) if nsamples is not None else acc


def path(w, m=None):
    """The launch path prune_rows(w, ..., m) takes, by name (PATH_NAMES), or 'composed' for a row too long to stay resident."""
    _check_w(w, 'path')
    K = w.shape[1]
    m = K if m is None else int(m)
    if not _operand(w):
        w = w.contiguous()
    p = _ffi.lib().llmc_prune_rows_path(_ffi.dt(w), w.shape[0], K, w.stride(0), m, _ffi.ptr(w))
    if p == -95 and m == K and K > MAX_RESIDENT_K:
        return 'composed'
    _ffi.check(min(p, 0), 'llmc_prune_rows_path')
    return PATH_NAMES[p]


def _metric(w, scaler_row):
    a = torch.abs(w)
    if scaler_row is None:
        return a.float()
    return a * torch.sqrt(scaler_row.reshape((1, -1)))                         # wanda.py:46-48


def prune_rows_composed(w, scaler_row, n_prune, m=None, want_mask=False):
    """The reference's sequence (wanda.py:46-56) from torch ops on the device, in place on w: the fp32 metric, a stable sort of
    every group of m columns, the first n_prune indices scattered into a boolean mask, a masked assignment. -> mask (uint8
    [R, K]) when want_mask, else None."""
    _ffi.require_gpu(w, scaler_row)
    m = _check_groups(w, scaler_row, n_prune, m)
    R, K = w.shape
    metric = _metric(w, scaler_row).reshape(R * (K // m), m)
    mask = torch.zeros_like(metric) == 1
    indices = torch.sort(metric, dim=-1, stable=True)[1][:, :int(n_prune)]
    mask.scatter_(1, indices, True)
    mask = mask.reshape(R, K)
    w[mask] = 0
    return mask.to(torch.uint8) if want_mask else None


def prune_rows(w, scaler_row, n_prune, m=None, want_mask=False):
    """In place on w [R, K] (GPU; unit column stride, row stride >= K — any other layout is pruned through a contiguous copy
    and copied back): zero the n_prune elements of smallest |w| * sqrt(scaler_row) in every group of m columns (m None = K, the
    per-row mode). scaler_row: fp32 [K] or None (the multiplier 1). -> uint8 mask [R, K] when want_mask, else None."""
    _ffi.require_gpu(w, scaler_row)
    m = _check_groups(w, scaler_row, n_prune, m)
    R, K = w.shape
    if m == K and K > MAX_RESIDENT_K:
        sig = (R, K, str(w.dtype))
        if sig not in _FALLBACK_SEEN:
            _FALLBACK_SEEN.add(sig)
            print(f'[llmc_amd] prune_rows {sig}: a row of more than {MAX_RESIDENT_K} columns does not stay resident in the HIP '
                  'kernel -> sort + scatter + masked assignment from torch ops on the GPU', file=sys.stderr)
        return prune_rows_composed(w, scaler_row, n_prune, m, want_mask)
    op = w if _operand(w) else w.contiguous()
    s = None
    if scaler_row is not None:
        s = scaler_row if scaler_row.dtype == torch.float32 and scaler_row.is_contiguous() else scaler_row.float().contiguous()
    mask = torch.empty((R, K), dtype=torch.uint8, device=w.device) if want_mask else None
    _ffi.check(_ffi.lib().llmc_prune_rows(_ffi.ptr(op), _ffi.dt(op), R, K, op.stride(0), _ffi.ptr(s), int(n_prune), m,
                                          _ffi.ptr(mask), _ffi.stream()), 'llmc_prune_rows')
    if op is not w:
        w.copy_(op)
    return mask


def magnitude_prune(w, kth, want_mask=False):
    """In place on w [R, K] (GPU): thresh = the |w| of 0-based rank kth over the whole tensor, every |w| <= thresh becomes +0.
    -> (thresh as a 0-dim tensor of w's dtype, uint8 mask [R, K] or None). Stream-ordered: nothing is read on the host."""
    _ffi.require_gpu(w)
    _check_w(w, 'magnitude_prune')
    R, K = w.shape
    if not 0 <= int(kth) < R * K:
        raise ValueError(f'magnitude_prune: kth = {kth} outside [0, {R * K}) (the reference raises an IndexError at sparsity 1.0)')
    op = w if _operand(w) else w.contiguous()
    L = _ffi.lib()
    dt = _ffi.dt(op)
    thresh = torch.empty((), dtype=w.dtype, device=w.device)
    mask = torch.empty((R, K), dtype=torch.uint8, device=w.device) if want_mask else None
    ws = _ffi.workspace(L.llmc_magnitude_prune_ws_bytes(dt, R, K), w.device)
    _ffi.check(L.llmc_magnitude_prune(_ffi.ptr(op), dt, R, K, op.stride(0), int(kth), _ffi.ptr(thresh), _ffi.ptr(mask),
                                      _ffi.ptr(ws), _ffi.stream()), 'llmc_magnitude_prune')
    if op is not w:
        w.copy_(op)
    return thresh, mask


SPARSEGPT_BLOCKSIZE = 128          # csrc/col_block.h: CB_BS


def sparsegpt_prune(W, Hinv, sparsity=None, nm=None, want_losses=False, want_mask=False):
    """SparseGPT's blocked column loop (csrc/sparsegpt_loop.hip, llmc_sparsegpt_prune). W [R, K] contiguous fp32 on the GPU,
    OVERWRITTEN with the running weights (GPTQ's convention); Hinv [K, K] contiguous fp32, the upper factor U with H^-1 = U^T U.
    Exactly one of sparsity (a float in [0, 1): per 128-column block, every score <= the score of rank int(R * count * sparsity)
    is pruned) and nm = (n, m) with m in {2, 4, 8, 16} (n of every m consecutive columns, scored on the running weights).
    -> (Wout fp32 [R, K], losses fp32 [R, K] | None, mask uint8 [R, K] | None). Stream-ordered: nothing is read on the host."""
    if (sparsity is None) == (nm is None):
        raise ValueError('sparsegpt_prune takes exactly one of sparsity and nm')
    if W.dim() != 2 or W.shape[0] < 1 or W.shape[1] < 1:
        raise ValueError('sparsegpt_prune takes a non-empty 2-D [R, K] weight')
    R, K = W.shape
    if tuple(Hinv.shape) != (K, K):
        raise ValueError(f'sparsegpt_prune: Hinv is {tuple(Hinv.shape)}, W has {K} columns')
    if W.dtype != torch.float32 or Hinv.dtype != torch.float32 or not W.is_contiguous() or not Hinv.is_contiguous():
        raise ValueError('sparsegpt_prune: W and Hinv must be contiguous fp32 (the kernel reads row-major [R, K] and [K, K])')
    n = m = 0
    if nm is None:
        sparsity = float(sparsity)
        if not 0.0 <= sparsity < 1.0:
            raise ValueError(f'sparsegpt_prune: sparsity = {sparsity} outside [0, 1)')
    else:
        n, m = (int(v) for v in nm)
        sparsity = 0.0
        if m not in NM_GROUPS:
            raise NotImplementedError(f'sparsegpt_prune: m is one of {NM_GROUPS}, not {m}')
        if not 0 <= n <= m:
            raise ValueError(f'sparsegpt_prune: n = {n} outside [0, {m}]')
        if K % m:
            raise NotImplementedError(f'sparsegpt_prune: m = {m} does not divide K = {K}')
    if K % 4:
        raise NotImplementedError(f'sparsegpt_prune: K = {K} must be a multiple of 4 (the trailing update\'s GEMM)')
    _ffi.require_gpu(W, Hinv)
    L = _ffi.lib()
    Wout = torch.empty_like(W)
    losses = torch.empty_like(W) if want_losses else None
    mask = torch.empty((R, K), dtype=torch.uint8, device=W.device) if want_mask else None
    ws = _ffi.workspace(L.llmc_sparsegpt_prune_ws_bytes(R, K), W.device)
    _ffi.check(L.llmc_sparsegpt_prune(_ffi.ptr(W), _ffi.ptr(Hinv), R, K, sparsity, n, m, _ffi.ptr(Wout), _ffi.ptr(losses),
                                      _ffi.ptr(mask), SPARSEGPT_BLOCKSIZE, _ffi.ptr(ws), _ffi.stream()), 'llmc_sparsegpt_prune')
    return Wout, losses, mask


def _rows(t, what):
    if t.dim() < 1 or t.numel() == 0:
        raise ValueError(f'{what} takes non-empty [..., d] tensors')
    t2 = t.reshape(-1, t.shape[-1])
    return t2 if _operand(t2) else t2.contiguous()


def block_influence_composed(x, y):
    """ShortGPT's per-token score 1 - cos(x, y) row-wise from torch ops in fp32, on any device: three row sums, two square
    roots, one product, one division, nan_to_num(nan=0.5) (shortgpt.py:49-55 without the N x N product). x, y [..., d] -> fp32
    [N]. It is what the tests compare the kernel against and what CPU tensors run."""
    if x.shape != y.shape:
        raise ValueError(f'block_influence: x is {tuple(x.shape)}, y is {tuple(y.shape)}')
    xf, yf = _rows(x, 'block_influence').float(), _rows(y, 'block_influence').float()
    dot, sx, sy = (xf * yf).sum(-1), (xf * xf).sum(-1), (yf * yf).sum(-1)
    sim = (dot / (sx.sqrt() * sy.sqrt())).nan_to_num(nan=0.5)
    return 1 - sim


def block_influence(x, y, total=None, init=True, max_grid=None):
    """x, y [..., d] of one dtype -> (bi fp32 [N], total): bi[n] = 1 - cos(x[n], y[n]) in fp32 and total, one fp64 element on the
    device, = sum(bi) (init) or total + sum(bi) (init False: `total` is updated in place; a one-element view such as
    importances[i] is written where it lies). On the GPU one pass of llmc_block_influence (csrc/block_influence.hip) in the order
    include/llmc_hip.h states; rows with a non-unit last stride are copied, any row stride >= d is read in place. Stream-ordered:
    nothing is read on the host. max_grid caps the row kernel's grid (tests: the grid-stride loop; same bits). CPU tensors run
    block_influence_composed and torch's fp64 sum.

    Dispatch: no shape is routed to the composition for speed: the kernel's call took 0.08x - 0.09x of its time in bf16 and
    0.20x - 0.22x in fp32 at 65536 x 4096 and 65536 x 8192, 0.23x and 0.38x at 4096 x 4096, with no overlap of the min..max
    ranges (profiles/shortgpt.txt, tools/bench_shortgpt.py)."""
    if x.shape != y.shape or x.dtype != y.dtype or x.device != y.device:
        raise ValueError(f'block_influence: x is {tuple(x.shape)} {x.dtype} on {x.device}, y is {tuple(y.shape)} {y.dtype} on '
                         f'{y.device}')
    x2, y2 = _rows(x, 'block_influence'), _rows(y, 'block_influence')
    N, d = x2.shape
    if total is None:
        if not init:
            raise ValueError('block_influence: folding (init=False) needs the running `total`')
        total = torch.empty((), dtype=torch.float64, device=x.device)
    elif total.dtype != torch.float64 or total.numel() != 1 or total.device != x.device:
        raise ValueError('block_influence: total must be one fp64 element on the device of x')
    if not x.is_cuda:
        bi = block_influence_composed(x2, y2)
        batch = bi.double().sum()
        if init:
            total.copy_(batch.reshape(total.shape))
        else:
            total.add_(batch.reshape(total.shape))
        return bi, total
    _ffi.require_gpu(x2, y2, total)
    L = _ffi.lib()
    bi = torch.empty(N, dtype=torch.float32, device=x.device)
    ws = _ffi.workspace(L.llmc_block_influence_ws_bytes(N), x.device)
    with _ffi.option(block_influence_max_grid=int(max_grid or 0)):
        _ffi.check(L.llmc_block_influence(_ffi.ptr(x2), _ffi.ptr(y2), _ffi.dt(x2), N, d, x2.stride(0), y2.stride(0),
                                          int(bool(init)), _ffi.ptr(bi), _ffi.ptr(total), _ffi.ptr(ws), _ffi.stream()),
                   'llmc_block_influence')
    return bi, total
