"""Hadamard transforms for QuaRot (llmc/compression/quantization/hadamard_utils.py of the reference) on the HIP kernel
llmc_hadamard. Names and returns follow the reference; there is no table of matrices here:

* every helper applies y = x . M_n^T / s with M_n = hadK (x) S_m (Kronecker product, S_m the Sylvester matrix in natural order,
  m = n / K a power of two) and s = fl32(sqrt(n)) — what both `matmul_hadU` (butterfly loop, then `hadK @`) and `matmul_hadU_cuda`
  (fast transform on [-1, K, n / K], then `hadK @`) of the reference compute;
* the small factors hadK are Paley constructions built on the fly (`paley_hadamard`): orders 12, 20, 60 are Paley I with
  q = 11, 19, 59, orders 28, 36 Paley II with q = 13, 17. They equal the matrices the reference tabulates entry for entry.
  Orders 40, 52, 156, 172 of the reference are other constructions (52, 156, 172: Williamson) and orders 108, 140 are larger
  than the 64 x 64 factor the kernel takes: a size that needs one of them raises NotImplementedError;
* `random_hadamard_matrix(n)` of the reference is Q = diag(sigma) . M_n^T / s with sigma drawn by one torch.randint call, so
  W . Q = T(W o sigma) row-wise and Q^T . W = T along the output axis of sigma[:, None] o W: no dense Q is needed, and
  `RandomHadamard` only holds sigma.
"""
import math

import torch

from llmc_amd import _ffi

# divisibility is tested in this order (hadamard_utils.py:19-69 of the reference), so the same n picks the same factor
_FACTOR_ORDER = (172, 156, 140, 108, 60, 52, 36, 28, 40, 20, 12)
_PALEY = {12: (1, 11), 20: (1, 19), 60: (1, 59), 28: (2, 13), 36: (2, 17)}
_REFUSED = {172: 'a Williamson matrix', 156: 'a Williamson matrix', 52: 'a Williamson matrix', 40: 'not a Paley matrix',
            140: 'larger than the 64 x 64 factor the kernel mixes', 108: 'larger than the 64 x 64 factor the kernel mixes'}
_CACHE = {}
_DT = {torch.float16: _ffi.F16, torch.bfloat16: _ffi.BF16, torch.float32: _ffi.F32, torch.float64: _ffi.F64}


def is_pow2(n):
    return (n & (n - 1) == 0) and (n > 0)


def _jacobsthal(q):
    """J[i][j] = chi_q(j - i), chi the quadratic character of the prime field GF(q) (chi(0) = 0)."""
    chi = torch.full((q,), -1, dtype=torch.int64)
    chi[0] = 0
    for a in range(1, q):
        chi[(a * a) % q] = 1
    idx = (torch.arange(q)[None, :] - torch.arange(q)[:, None]) % q
    return chi[idx]


def paley_hadamard(kind, q):
    """Paley's Hadamard matrices for a prime q. kind 1 (q = 3 mod 4), order q + 1: first row (1, -1 ... -1), first column
    +1, core I - J. kind 2 (q = 1 mod 4), order 2 (q + 1): A (x) S + B (x) I with A = [[1, 1], [1, -1]],
    B = [[1, -1], [-1, -1]], S = [[0, 1^T], [1, J]]. int64 matrix of +-1."""
    J = _jacobsthal(q)
    if kind == 1:
        assert q % 4 == 3
        H = torch.ones(q + 1, q + 1, dtype=torch.int64)
        H[0, 1:] = -1
        H[1:, 1:] = torch.eye(q, dtype=torch.int64) - J
        return H
    assert q % 4 == 1
    S = torch.ones(q + 1, q + 1, dtype=torch.int64)
    S[0, 0] = 0
    S[1:, 1:] = J
    A = torch.tensor([[1, 1], [1, -1]])
    B = torch.tensor([[1, -1], [-1, -1]])
    return torch.kron(A, S) + torch.kron(B, torch.eye(q + 1, dtype=torch.int64))


def get_hadK(n, transpose=False):
    """(hadK, K) as the reference returns them: the factor matrix (float32 [K, K], None for K == 1) and its order."""
    for K in _FACTOR_ORDER:
        if n % K == 0:
            if K in _REFUSED:
                raise NotImplementedError(f'Hadamard size {n} needs the order-{K} factor matrix, which is {_REFUSED[K]}: '
                                          'not supported')
            if not is_pow2(n // K):
                raise NotImplementedError(f'Hadamard size {n} = {K} * {n // K}: the cofactor of the order-{K} factor '
                                          'matrix is not a power of two')
            if K not in _CACHE:
                _CACHE[K] = paley_hadamard(*_PALEY[K]).to(torch.float32)
            hadK = _CACHE[K]
            return (hadK.T if transpose else hadK), K
    if not is_pow2(n):
        raise NotImplementedError(f'Hadamard size {n} is neither a power of two nor a supported factor times one')
    return None, 1


def _fl32_sqrt(n):
    return float(torch.tensor(n).sqrt())          # float32 0-dim tensor, as in the reference


def hadamard_transform(x, n, inner=1, hadK=None, K=1, scale=1.0, out=None):
    """llmc_hadamard on a contiguous GPU tensor viewed as [-1, n, inner]; returns a new tensor (or `out`, which may be x)."""
    _ffi.require_gpu(x)
    if x.dtype not in _DT:
        raise ValueError(f'hadamard_transform: unsupported dtype {x.dtype}')
    x = x.contiguous()
    if x.numel() % (n * inner):
        raise ValueError(f'hadamard_transform: {tuple(x.shape)} is no [-1, {n}, {inner}]')
    y = torch.empty_like(x) if out is None else out
    assert y.is_contiguous() and y.shape == x.shape and y.dtype == x.dtype
    hk = None
    if K > 1:
        hk = hadK.to(device=x.device, dtype=torch.float32).contiguous()
        assert hk.shape == (K, K)
    rc = _ffi.lib().llmc_hadamard(_ffi.ptr(x), _ffi.ptr(y), _DT[x.dtype], x.numel() // (n * inner), n, inner, _ffi.ptr(hk), K,
                                  float(scale), _ffi.stream())
    _ffi.check(rc, 'llmc_hadamard')
    return y


def matmul_hadU(X, transpose=False):
    n = X.shape[-1]
    hadK, K = get_hadK(n, transpose)
    return hadamard_transform(X, n, 1, hadK, K, 1.0 / _fl32_sqrt(n))


def matmul_hadUt(X):
    return matmul_hadU(X, transpose=True)


def matmul_hadU_cuda(X, hadK, K):
    n = X.shape[-1]
    return hadamard_transform(X, n, 1, hadK, K, 1.0 / _fl32_sqrt(n))


def matmul_hadUt_cuda(X, hadK, K):
    return matmul_hadU_cuda(X, None if hadK is None else hadK.T, K)


class RandomHadamard:
    """Q = diag(sigma) . M_n^T / fl32(sqrt(n)) without the matrix: sigma (+-1, float64, on `device`) and n."""

    def __init__(self, sigma, device):
        self.n = sigma.numel()
        self.sigma = sigma.to(device)
        self.device = self.sigma.device

    def right(self, W):
        """W . Q for a [..., n] float64 tensor: the row transform of W o sigma."""
        return matmul_hadU(W * self.sigma)

    def left_t(self, W):
        """Q^T . W for a float64 [n] or [n, c] tensor: the transform along the first axis of sigma[:, None] o W."""
        hadK, K = get_hadK(self.n)
        W2 = W.reshape(self.n, -1)
        out = hadamard_transform(W2 * self.sigma[:, None], self.n, W2.shape[1], hadK, K, 1.0 / _fl32_sqrt(self.n))
        return out.reshape(W.shape)

    def dense(self):
        """The float64 [n, n] matrix random_hadamard_matrix of the reference returns."""
        return matmul_hadU(torch.diag(self.sigma))


def random_hadamard_matrix(size, device):
    # the reference's draw (hadamard_utils.py:103-104): the same generator state gives the same signs
    Q = torch.randint(low=0, high=2, size=(size,)).to(torch.float64)
    Q = Q * 2 - 1
    get_hadK(size)                                   # an unsupported size fails here, not at the first rotation
    return RandomHadamard(Q, device)


def rotate_right(W, Q):
    """W @ Q in float64 (W already .double()): through the kernel for a RandomHadamard, a matmul for a dense tensor."""
    if isinstance(Q, RandomHadamard):
        return Q.right(W)
    return torch.matmul(W, Q)


def rotate_left_t(W, Q):
    """Q.T @ W in float64."""
    if isinstance(Q, RandomHadamard):
        return Q.left_t(W)
    return torch.matmul(Q.T, W)


def apply_exact_had_to_linear(module, had_dim=-1, output=False):
    in_features, out_features = module.in_features, module.out_features
    if had_dim != -1:
        assert is_pow2(had_dim), 'Hadamard dimension must be a power of 2!'
    W_ = module.weight.data
    dtype, dev = W_.dtype, W_.device
    W_ = W_.float().cuda().contiguous()
    if had_dim == -1:
        if output:
            had_K, K = get_hadK(out_features)          # along the output axis: [1, out, in]
            W_ = hadamard_transform(W_, out_features, in_features, had_K, K, 1.0 / _fl32_sqrt(out_features))
        else:
            had_K, K = get_hadK(in_features)
            W_ = matmul_hadU_cuda(W_, had_K, K)
    else:
        if not output:
            raise NotImplementedError('Not implemented (or tested) yet!')
        # Sylvester transform of every had_dim chunk of the output axis: [out / had_dim, had_dim, in]
        W_ = hadamard_transform(W_, had_dim, in_features, None, 1, 1 / math.sqrt(had_dim))
    module.weight.data = W_.to(device=dev, dtype=dtype)
