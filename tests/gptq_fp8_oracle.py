"""Numpy fp32 restatement of GPTQ.weight_transform (gptq.py:199-244) with a FloatQuantizer weight quantizer (use_qtorch,
quant.py:1061-1081) for any shape. Test infrastructure, beside tests/hqq_oracle.py; tests/test_gptq_fp8_oracle.py pins it to
the reference's own output (tests/golden/gptq_fp8.npz).

Every in-block op is one numpy float32 vector op over the rows (division, product, difference: numpy contracts nothing into
an fma, so each rounds once, like ATen's elementwise kernels); the rounding is oracle.quant_ref.qtorch_float_quantize; the
trailing update `W[:, i2:] -= Err1 @ Hinv[i1:i2, i2:]` is oracle.gptq_ref.mm_chain (one fmaf chain per element from +0 in
ascending k, the order the existing GPTQ goldens pin). Rows are independent given the upper factor, so a row subset of W (and
of the static scales) gives that subset of the full result.
"""
import numpy as np

from oracle import gptq_ref as G
from oracle import quant_ref as Q

F32 = np.float32
FORMATS = {'e4m3': (4, 3, 448.0), 'e5m2': (5, 2, 57344.0)}     # (E, M, finfo(float8 type).max = the quantizer's qmax)


def float_qdq(w, s, E, M):
    """FloatQuantizer.quant_dequant on fp32 columns (sym, zeros = tensor(0.)), op by op. Returns (q, t): the dequantized value
    and the scaled value that was rounded."""
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        s1 = np.where(s == 0, F32(1.0), s).astype(F32)            # scales[scales == 0] = 1
        t = (w / s1).astype(F32)
        t = (t + F32(0.0)).astype(F32)                            # + zeros: -0 becomes +0
        v = Q.qtorch_float_quantize(t, E, M)
        q = ((v - F32(0.0)).astype(F32) * s1).astype(F32)
    return q, t


def weight_transform(W, U, fmt, group_size=0, static_groups=False, col_group=None, scales=None, n_quant=None, blocksize=128):
    """W [R, K] fp32 (copied), U [K, K] fp32 upper factor. group_size 0: per_channel, scales [R] given; static_groups: scales
    [R, K / group_size] given and col_group [K] the group of every processed column; else the scales of every group are taken at
    its start from the running W (search_column_qparams -> get_qparams, quant.py:545-553) and returned [R, ng].
    Returns dict(tmp, losses, W (running), scales, t_absmax (largest |w / s| that was rounded))."""
    E, M, qmax = FORMATS[fmt]
    W = np.array(W, dtype=F32, copy=True, order='C')
    U = np.ascontiguousarray(U, dtype=F32)
    R, K = W.shape
    nq = K if n_quant is None else int(n_quant)
    gs = int(group_size or 0)
    dynamic = bool(gs) and not static_groups
    ng = -(-K // gs) if gs else 1
    if dynamic:
        sc = np.zeros((R, ng), F32) if scales is None else np.array(scales, dtype=F32).reshape(R, ng).copy()
    else:
        sc = np.asarray(scales, dtype=F32).reshape(R, ng)
    tmp, losses = np.zeros_like(W), np.zeros_like(W)
    t_absmax = 0.0
    s = None
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        for i1 in range(0, nq, blocksize):
            i2 = min(i1 + blocksize, nq)
            count = i2 - i1
            W1 = W[:, i1:i2].copy()
            Err = np.zeros_like(W1)
            for i in range(count):
                c = i1 + i
                w = W1[:, i].copy()
                d = U[c, c]
                if dynamic:
                    if c % gs == 0:
                        blk = W[:, c:min(c + gs, nq)]             # W, not W1: the values the block started with
                        s, _ = Q.qparams_from_minmax(blk.min(axis=1), blk.max(axis=1), Q.F32, True, -qmax, qmax)
                        sc[:, c // gs] = s
                elif gs:
                    s = sc[:, int(col_group[c])]
                else:
                    s = sc[:, 0]
                q, t = float_qdq(w, s, E, M)
                fin = np.abs(t[np.isfinite(t)])
                if fin.size:
                    t_absmax = max(t_absmax, float(fin.max()))
                diff = (w - q).astype(F32)
                tmp[:, c] = w
                losses[:, c] = ((diff * diff).astype(F32) / (F32(2.0) * (d * d).astype(F32)).astype(F32)).astype(F32)
                err = (diff / d).astype(F32)
                if i + 1 < count:
                    W1[:, i + 1:] = (W1[:, i + 1:] - (err[:, None] * U[c, c + 1:i2][None, :]).astype(F32)).astype(F32)
                Err[:, i] = err
            if i2 < K:
                W[:, i2:] = (W[:, i2:] - G.mm_chain(Err, U[i1:i2, i2:])).astype(F32)
    return dict(tmp=tmp, losses=losses, W=W, scales=sc, t_absmax=t_absmax)


# ---- the golden file's conventions (tools/make_golden_gptq_fp8.py), shared by the CPU and the GPU tests ----------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def synth_upper(K, seed):
    """tools/make_golden_gptq_mse.py:synth_upper — the upper factor the golden's reference loop ran with"""
    i = np.arange(K, dtype=np.int64)[:, None]
    j = np.arange(K, dtype=np.int64)[None, :]
    h = (i * 2654435761 + j * 40503 + seed * 7919) % 65521
    off = ((h % 257) - 128).astype(np.float32) / np.float32(4096.0)
    diag = np.float32(0.5) + (i % 61).astype(np.float32) / np.float32(64.0)
    return np.where(j > i, off, np.where(j == i, diag, np.float32(0.0))).astype(np.float32)


def from_bits16(b, dt):
    """16-bit patterns of an f16 / bf16 tensor -> its values in fp32"""
    b = np.ascontiguousarray(b, dtype=np.uint16)
    if dt == 'f16':
        return b.view(np.float16).astype(np.float32)
    return (b.astype(np.uint32) << 16).view(np.float32)


def case_inputs(g, case):
    """(Wp fp32, U, fmt, group_size, static_groups, col_group, static scales | None) of a case of tests/golden/gptq_fp8.npz (g: the loaded file)"""
    p = case + '/'
    e_bits, m_bits, gs, actorder, static_groups, R, K, qmin, qmax = g[p + 'meta']
    R, K, gs = int(R), int(K), int(gs)
    seed, csum, amp = g[p + 'U_seed']          # amp: the power of two the off-diagonal entries are multiplied by
    U = synth_upper(K, int(seed))
    U = np.where(np.eye(K, dtype=bool), U, U * np.float32(amp)).astype(np.float32)
    assert int(U.view(np.uint32).astype(np.uint64).sum()) == int(csum), case
    Wp = from_bits16(g[p + 'Wp_bits'], str(g[p + 'dt'])).reshape(R, K)
    perm = g[p + 'perm']
    col_group = scales = None
    if static_groups or not gs:
        scales = g[p + 'rtn_scales'].reshape(R, -1)         # the layer's RTN scales (16-bit values), original group order
        if gs:
            col_group = ((perm if perm.size else np.arange(K)) // gs).astype(np.int32)
    return Wp, U, str(g[p + 'bit']), gs, bool(static_groups), col_group, scales
