"""Numpy restatement of SparseGPT's blocked column loop as include/llmc_hip.h specifies it (llmc_sparsegpt_prune): the published
`fasterprune` (Frantar & Alistarh 2023) at blocksize 128. Test infrastructure, beside tests/gptq_fp8_oracle.py; the reference
tree has no SparseGPT, so tests/test_sparsegpt_oracle.py pins this file to independent mathematics instead (the paper's
unoptimised column-by-column recursion in float64).

Every step is one numpy vector op over the rows in `dtype` (numpy contracts nothing into an fma, so each rounds once). In
float32 the trailing update `W[:, i2:] -= Err1 @ U[i1:i2, i2:]` is oracle.gptq_ref.mm_chain (one fmaf chain per element from +0
in ascending k, what sgemm.hip computes); in float64 it is numpy's matmul. n:m ranks by np.argsort(kind='stable'): equal scores
by lower column."""
import numpy as np

BLOCKSIZE = 128


def _mm(a, b, dtype):
    if dtype == np.float32:
        from oracle import gptq_ref as G
        return G.mm_chain(a, b)
    return a @ b


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def kth_of(numel, sparsity):
    """Python's int(numel * sparsity): double arithmetic, truncated"""
    return int(float(numel) * float(sparsity))


def prune(W, U, sparsity=None, nm=None, blocksize=BLOCKSIZE, dtype=np.float32):
    """W [R, K] (copied), U [K, K] upper factor with H^-1 = U^T U; exactly one of sparsity and nm = (n, m).
    -> dict(Wout, losses, mask (uint8), W (running weights: a block's own columns keep their block-start values),
            scores [R, K] and thresh [number of blocks] (unstructured only: the block-start scores and each block's threshold))."""
    assert (sparsity is None) != (nm is None)
    F = np.dtype(dtype).type
    W = np.array(W, dtype=F, copy=True, order='C')
    U = np.ascontiguousarray(U, dtype=F)
    R, K = W.shape
    Wout, losses = np.zeros_like(W), np.zeros_like(W)
    mask = np.zeros((R, K), dtype=bool)
    scores, thresh = np.zeros_like(W), []
    if nm is not None:
        n, m = nm
        assert K % m == 0 and blocksize % m == 0
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        for i1 in range(0, K, blocksize):
            i2 = min(i1 + blocksize, K)
            count = i2 - i1
            W1 = W[:, i1:i2].copy()
            Err = np.zeros_like(W1)
            d = np.diagonal(U)[i1:i2].astype(F)
            dd = (d * d).astype(F)
            if nm is None:
                s = ((W1 * W1).astype(F) / dd[None, :]).astype(F)
                t = np.sort(s, axis=None)[kth_of(R * count, sparsity)]
                mask1 = s <= t
                scores[:, i1:i2] = s
                thresh.append(t)
            else:
                mask1 = np.zeros((R, count), dtype=bool)
            for i in range(count):
                c = i1 + i
                w = W1[:, i].copy()
                if nm is not None and i % m == 0:
                    blk = W1[:, i:i + m]
                    s = ((blk * blk).astype(F) / dd[None, i:i + m]).astype(F)
                    lowest = np.argsort(s, axis=1, kind='stable')[:, :n]
                    np.put_along_axis(mask1[:, i:i + m], lowest, True, axis=1)
                cut = mask1[:, i]
                q = np.where(cut, F(0.0), w).astype(F)
                Wout[:, c] = q
                mask[:, c] = cut
                diff = (w - q).astype(F)
                losses[:, c] = ((diff * diff).astype(F) / dd[i]).astype(F)
                err = (diff / d[i]).astype(F)
                if i + 1 < count:
                    W1[:, i + 1:] = (W1[:, i + 1:] - (err[:, None] * U[c, c + 1:i2][None, :]).astype(F)).astype(F)
                Err[:, i] = err
            if i2 < K:
                W[:, i2:] = (W[:, i2:] - _mm(Err, U[i1:i2, i2:], dtype)).astype(F)
    return dict(Wout=Wout, losses=losses, mask=mask.astype(np.uint8), W=W, scores=scores, thresh=thresh)
