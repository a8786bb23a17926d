"""numpy / fp64 restatement of the Hadamard transforms QuaRot uses (test helper, no GPU):

  T(x) = x . M_n^T / s,   M_n = hadK (x) S_m,   s = fl32(sqrt(n)),   Q = diag(sigma) . M_n^T / s

with S_m = scipy.linalg.hadamard(m) (Sylvester, natural order). `apply_M` uses S_m = S_a (x) S_b so that a 32768-long row needs
no dense matrix; `dense_M` is the literal Kronecker product (the two are compared in tests/test_hadamard_utils.py). `paley` is a
second construction of the factor matrices, independent of llmc_amd's (Euler's criterion instead of a table of squares, explicit
loops instead of index arithmetic). `exact_scaled` is the value a scaled transform of small integers must have bit for bit
(exact sums, one multiplication, one rounding)."""
import numpy as np
from scipy.linalg import hadamard

PALEY_ORDERS = {12: (1, 11), 20: (1, 19), 28: (2, 13), 36: (2, 17), 60: (1, 59)}


def fl32_sqrt(n):
    return float(np.sqrt(np.float32(n)))


def legendre(a, q):
    a %= q
    if a == 0:
        return 0
    return 1 if pow(a, (q - 1) // 2, q) == 1 else -1


def paley(K):
    kind, q = PALEY_ORDERS[K]
    J = np.array([[legendre(j - i, q) for j in range(q)] for i in range(q)], dtype=np.int64)
    if kind == 1:
        H = np.ones((q + 1, q + 1), dtype=np.int64)
        H[0, 1:] = -1
        H[1:, 1:] = np.eye(q, dtype=np.int64) - J
        return H
    S = np.zeros((q + 1, q + 1), dtype=np.int64)
    S[0, 1:] = 1
    S[1:, 0] = 1
    S[1:, 1:] = J
    A = np.array([[1, 1], [1, -1]], dtype=np.int64)
    B = np.array([[1, -1], [-1, -1]], dtype=np.int64)
    return np.kron(A, S) + np.kron(B, np.eye(q + 1, dtype=np.int64))


def is_hadamard(H):
    H = np.asarray(H).astype(np.int64)
    K = H.shape[0]
    return H.shape == (K, K) and bool((np.abs(H) == 1).all()) and bool((H @ H.T == K * np.eye(K, dtype=np.int64)).all())


def dense_M(n, hadK=None):
    K = 1 if hadK is None else np.asarray(hadK).shape[0]
    m = n // K
    S = hadamard(m, dtype=np.int64) if m > 1 else np.ones((1, 1), dtype=np.int64)
    return S if K == 1 else np.kron(np.asarray(hadK).astype(np.int64), S)


def apply_M(x, hadK=None, axis=-1):
    """M_n applied along `axis` of x (int64 stays exact, float64 stays float64)."""
    x = np.moveaxis(np.asarray(x), axis, -1)
    n = x.shape[-1]
    K = 1 if hadK is None else np.asarray(hadK).shape[0]
    m = n // K
    assert K * m == n and m & (m - 1) == 0
    a = 1 << (max(m.bit_length() - 1, 0) // 2)
    b = m // a
    Sa = hadamard(a, dtype=np.int64) if a > 1 else np.ones((1, 1), dtype=np.int64)
    Sb = hadamard(b, dtype=np.int64) if b > 1 else np.ones((1, 1), dtype=np.int64)
    t = x.reshape(x.shape[:-1] + (K, a, b))
    t = np.einsum('...kab,jb->...kaj', t, Sb.astype(x.dtype))
    t = np.einsum('...kaj,ia->...kij', t, Sa.astype(x.dtype))
    if K > 1:
        t = np.einsum('...kij,ck->...cij', t, np.asarray(hadK).astype(x.dtype))
    return np.moveaxis(t.reshape(x.shape), -1, axis)


def transform(x, hadK=None, axis=-1, scale=None):
    """T(x) in float64; scale defaults to 1 / fl32(sqrt(n))."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[axis]
    return apply_M(x, hadK, axis) * (1.0 / fl32_sqrt(n) if scale is None else scale)


def exact_scaled(e, scale, dtype):
    """What llmc_hadamard must return, bit for bit, when e = apply_M(integers) holds integers below 2^24: the sums are exact in
    any order, so the result is one multiplication by the scale cast to the accumulator type and one rounding to `dtype`.
    F32 / F16 / BF16: round_dtype(fl32(fl32(e) * fl32(scale))); F64: fl64(e * scale). Returns a torch tensor of `dtype`."""
    import torch
    e = np.asarray(e)
    assert e.dtype.kind == 'i' and np.abs(e).max(initial=0) < 2 ** 24
    if dtype == torch.float64:
        return torch.from_numpy(np.ascontiguousarray(e.astype(np.float64) * np.float64(scale)))
    return torch.from_numpy(np.ascontiguousarray(e.astype(np.float32) * np.float32(scale))).to(dtype)


def dense_Q(sigma, hadK=None):
    """random_hadamard_matrix: matmul_hadU(diag(sigma)) = diag(sigma) . M_n^T / fl32(sqrt(n)), float64."""
    sigma = np.asarray(sigma, dtype=np.float64)
    n = sigma.size
    return (sigma[:, None] * dense_M(n, hadK).T.astype(np.float64)) / fl32_sqrt(n)


def gamma(r, u):
    return r * u / (1 - r * u)


def bound(x_l1, y, n, K, scale, u_acc, u_out):
    """|yhat - y| <= gamma_r . ||x||_1 . scale + u_out . |y|, r = log2(n / K) + K + 1 roundings of unit roundoff u_acc (every
    |M_n| entry is 1, so (|M_n| |x|)_i = ||x||_1); u_out is half an ulp of the output dtype (0 when it is the accumulator's)."""
    r = int(np.log2(n // K)) + K + 1
    return gamma(r, u_acc) * x_l1 * abs(scale) + u_out * np.abs(y)
