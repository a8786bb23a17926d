"""Functional wrappers over the token-selection kernels of libllmc_hip.so (csrc/token_select.hip): what DivPrune runs per prefill,
and the pairwise matrix the other diversity / merging methods of the family form (ToMe, DART, VisionZip, FastVID, DyCoke).

cosine_distance           x [N, d] (bf16, f16, fp32) -> fp32 [N, N], D[i][j] = 1 - cos(x_i, x_j): the Gram matrix on the matrix pipe
                          straight from x (no transposed, no normalised copy), upper tiles only, the mirror copied
                          (llmc_cosine_dist; arithmetic and order: include/llmc_hip.h; error bound: tests/divprune_oracle.py).
cosine_distance_composed  the reference's sequence from torch ops, on any device (divprune.py:13-27): x / x.norm(dim=1,
                          keepdim=True), mm with its transpose, 1.0 -. In fp32: the features are widened first, so that the result
                          is the fp32 matrix cosine_distance returns and not one rounded to 8 or 11 bits after every operation.
maxmin_select             D [N, N] (fp32, bf16, f16, kept as it is), k -> int64 [k]: DivPrune's greedy max-min choice
                          (llmc_maxmin_select), all k steps in one launch, nothing read on the host.
maxmin_select_composed    the reference's loop from torch ops, on any device (divprune.py:29-53), unchanged: about six launches
                          and a gather of every chosen row per step.

CPU tensors run the composed forms. On the GPU the composed forms are the tests' second opinion and what the two wrappers fall
back to, announced once per shape on stderr, where the kernel answers LLMC_ENOTSUP (maxmin_select: N > 16384, the columns one
workgroup keeps resident; cosine_distance: N > 46340).

Dispatch: nothing is routed to the composition for speed. Measured (profiles/divprune.txt, tools/bench_divprune.py; whole calls,
bf16 and f16, d = 4096): divprune() took 0.099 / 0.042 / 0.047 of the time of the two composed functions chained at N = 576 ratio
0.1 / 0.5 and N = 2880 ratio 0.25, cosine_distance alone 0.35 - 0.40 of cosine_distance_composed, maxmin_select alone 0.039 - 0.079
of maxmin_select_composed, with no overlap of the min..max ranges. The launch and traffic counts DESIGN.md quotes for the
reference's loop are computed, not measured."""
import sys

import torch

from llmc_amd import _ffi

MAX_RESIDENT_N = 16384          # csrc/token_select.hip: kMmMaxN
MAX_DIST_N = 46340              # csrc/token_select.hip: kCdMaxN

_FALLBACK_SEEN = set()


def _announce(what, sig, why, instead):
    if (what, sig) not in _FALLBACK_SEEN:
        _FALLBACK_SEEN.add((what, sig))
        print(f'[llmc_amd] {what} {sig}: {why} -> {instead}', file=sys.stderr)


def _operand(t):
    """does the matrix lie as the kernels take it (unit column stride, row stride >= columns)? Anything else is copied"""
    return t.stride(1) == 1 and t.stride(0) >= t.shape[1]


def _check_x(x, what):
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f'{what} takes non-empty [N, d] features, got {tuple(x.shape)}')


def _check_d(D, k, what):
    if D.dim() != 2 or D.shape[0] != D.shape[1]:
        raise ValueError(f'{what} takes a square [N, N] matrix, got {tuple(D.shape)}')
    if D.shape[0] < 2:
        raise ValueError(f'{what}: N = {D.shape[0]} < 2 (the second smallest of a column needs two rows; the reference\'s topk(2) '
                         'raises there)')
    if int(k) < 0:
        raise ValueError(f'{what}: k = {k} < 0')


def cosine_distance_composed(x):
    """The reference's op sequence in fp32, on any device: x [N, d] -> fp32 [N, N]."""
    _check_x(x, 'cosine_distance_composed')
    xf = x.float()
    norm_matrix = xf / xf.norm(dim=1, keepdim=True)
    return 1.0 - torch.mm(norm_matrix, norm_matrix.t())


def cosine_distance(x):
    """x [N, d] -> fp32 [N, N] of 1 - cos. On the GPU one call of llmc_cosine_dist: rows with a non-unit last stride are copied,
    any row stride >= d and any alignment is read in place. Stream-ordered. CPU tensors run cosine_distance_composed."""
    _check_x(x, 'cosine_distance')
    if not x.is_cuda:
        return cosine_distance_composed(x)
    N, d = x.shape
    if N > MAX_DIST_N:
        _announce('cosine_distance', (N, d, str(x.dtype)), f'an element index of the {N} x {N} matrix leaves 32 bits in the HIP kernel',
                  'norm + mm + subtraction from torch ops on the GPU')
        return cosine_distance_composed(x)
    op = x if _operand(x) else x.contiguous()
    _ffi.require_gpu(op)
    L = _ffi.lib()
    dt = _ffi.dt(op)
    D = torch.empty((N, N), dtype=torch.float32, device=x.device)
    ws = _ffi.workspace(L.llmc_cosine_dist_ws_bytes(N, d), x.device)
    _ffi.check(L.llmc_cosine_dist(_ffi.ptr(op), dt, N, d, op.stride(0), _ffi.ptr(D), _ffi.ptr(ws), _ffi.stream()),
               'llmc_cosine_dist')
    return D


def maxmin_select_composed(D, k):
    """The reference's loop (divprune.py:29-53) from torch ops on the device of D: step 0 scores a column by its second smallest
    element, step i gathers the i chosen rows and reduces them with min, every step takes an argmax. -> int64 [k]."""
    _check_d(D, k, 'maxmin_select_composed')
    k = int(k)
    s = torch.empty(k, dtype=torch.long, device=D.device)
    for i in range(k):
        if i == 0:
            scores = torch.topk(D, 2, dim=0, largest=False).values[1, :]
        else:
            m2 = torch.index_select(D, 0, torch.index_select(s, 0, torch.arange(0, i, device=D.device)))
            scores = torch.min(m2, dim=0).values
        s[i] = torch.argmax(scores)
    return s


def maxmin_select(D, k):
    """D [N, N], k -> int64 [k] on the device of D, by the rules include/llmc_hip.h states (llmc_maxmin_select). The matrix keeps
    its dtype; a non-unit column stride is copied, any row stride >= N is read in place. Stream-ordered: the chosen index never
    leaves the device. CPU tensors, and N > 16384 on the GPU (announced once per shape), run maxmin_select_composed."""
    _check_d(D, k, 'maxmin_select')
    k = int(k)
    if not D.is_cuda:
        return maxmin_select_composed(D, k)
    N = D.shape[0]
    if N > MAX_RESIDENT_N:
        _announce('maxmin_select', (N, k, str(D.dtype)), f'more than {MAX_RESIDENT_N} columns do not stay resident in the HIP kernel',
                  'topk + index_select + min + argmax per step from torch ops on the GPU')
        return maxmin_select_composed(D, k)
    op = D if _operand(D) else D.contiguous()
    _ffi.require_gpu(op)
    L = _ffi.lib()
    sel = torch.empty(k, dtype=torch.long, device=D.device)
    if k == 0:
        return sel
    ws = _ffi.workspace(L.llmc_maxmin_select_ws_bytes(N), D.device)
    _ffi.check(L.llmc_maxmin_select(_ffi.ptr(op), _ffi.dt(op), N, op.stride(0), k, _ffi.ptr(sel), _ffi.ptr(ws), _ffi.stream()),
               'llmc_maxmin_select')
    return sel
