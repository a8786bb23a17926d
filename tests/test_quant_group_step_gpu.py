"""The integer quantizer's group step (csrc/quant_group.h) where only its round_zp = False rule decides the result, on every
kernel family that runs it: k_quant_static (vector and scalar kernel), the column kernels (tile, slab and scalar path) and the
mixed int / fp kernels (mask form; index form with a sub-wave team and with the whole workgroup as the team).

round_zp = False divides by s.clamp_min(1e-9) (quant.py:702-707). The inputs are fp32 values in [1, 1 + 5e-6] on an asymmetric
16-bit grid: every group's spread is below get_qparams' 1e-5 floor, so s = 1e-5 / 65535 = 1.5e-10 < 1e-9 and the clamp is what
the fake values depend on. The test first shows on the CPU that the oracle with and without the clamp gives different fake
values in every group (the clamped divisor sends every code to qmin, the unclamped one does not); if that fails the input is
wrong, not a kernel. Then every kernel must equal the clamped oracle bit for bit. The oracle is the numpy restatement that
test_quant_widths_gpu.py uses for k_quant_static (static_reference over oracle/quant_ref.py)."""
import functools

import numpy as np
import pytest
import torch

from oracle import quant_ref as Q
from test_quant_widths_gpu import eq_bits, static_reference

pytestmark = pytest.mark.gpu

QMIN, QMAX = 0.0, 65535.0
PATH_TILE, PATH_SLAB, PATH_SCALAR = 0, 1, 2


def weights(rows, cols, seed):
    """fp32 [rows, cols] in [1, 1 + 5e-6]: about 42 distinct fp32 values, so any group of a few elements has a spread > 0"""
    rng = np.random.default_rng(seed)
    return (np.float32(1.0) + rng.integers(0, 43, size=(rows, cols)).astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)


def unclamped_reference(w2, s, z):
    """static_reference's fractional branch WITHOUT the clamp of the divisor: what a kernel that forgot the rule computes"""
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        t = Q.rnd(w2 / s, 'f32')
        t = Q.rnd(t + z, 'f32')
        codes = np.minimum(np.maximum(np.rint(t), np.float32(QMIN)), np.float32(QMAX))
    return Q.rnd(Q.dequant(codes, s, z, 'f32'), 'f32')


def oracle(w2):
    """[G, g] groups -> (fake values, scales, zeros) of round_zp = False; asserts that the clamp decides every group"""
    assert w2.dtype == np.float32 and float(w2.max() - w2.min()) < 1e-5
    s, z = Q.minmax_qparams(w2, 'f32', False, QMIN, QMAX, round_zp=False)
    assert (s < np.float32(1e-9)).all(), 'the scale must lie below the clamp'
    fake, _ = static_reference(w2, 'f32', s, 'f32', z, 'f32', QMIN, QMAX, fractional=True)
    other = unclamped_reference(w2, s, z)
    differs = (fake.view(np.uint32) != other.view(np.uint32)).any(axis=-1)
    assert differs.all(), f'groups {np.flatnonzero(~differs)[:8]}: clamped and unclamped divisor agree, the input proves nothing'
    return fake, s, z


@functools.lru_cache(maxsize=None)
def case(rows, cols, seed):
    w = weights(rows, cols, seed)
    w.setflags(write=False)
    return w


def gpu(a):
    return torch.tensor(np.asarray(a)).cuda()          # a copy: the cached inputs stay read-only


# ---- k_quant_static with LLMC_FRACTIONAL_ZP and the oracle's qparams ------------------------------------------------------
@pytest.mark.parametrize('kernel', ['vector', 'scalar'])
def test_static(kernel):
    from llmc_amd import _ffi
    G, g = 24, 72
    w2 = case(G, g, 1)
    fake, s, z = oracle(w2)
    buf = torch.zeros(G * g + 1, dtype=torch.float32, device='cuda')
    off = 0 if kernel == 'vector' else 1                       # one element into the storage: no 16-byte alignment
    wd = buf[off:off + G * g]
    wd.copy_(gpu(w2).reshape(-1))
    assert (wd.data_ptr() % 16 == 0) == (kernel == 'vector')
    sd, zd = gpu(s.reshape(-1)), gpu(z.reshape(-1))
    out = torch.empty(G * g, dtype=torch.float32, device='cuda')
    _ffi.check(_ffi.lib().llmc_quant_static(_ffi.ptr(wd), _ffi.dt(wd), G, g, _ffi.ptr(sd), _ffi.dt(sd), _ffi.ptr(zd),
                                            _ffi.dt(zd) | _ffi.FRACTIONAL_ZP, QMIN, QMAX, _ffi.OUT_FAKE, _ffi.ptr(out),
                                            _ffi.stream()), 'llmc_quant_static')
    eq_bits(out.cpu().numpy().reshape(G, g), fake, f'quant_static {kernel}')


# ---- llmc_quant_dynamic_cols: groups of g rows down a column ---------------------------------------------------------------
@pytest.mark.parametrize('name,R,K,g,path', [('tile', 48, 64, 16, PATH_TILE), ('slab', 320, 64, 320, PATH_SLAB),
                                             ('scalar', 48, 66, 16, PATH_SCALAR)])
def test_cols(name, R, K, g, path):
    from llmc_amd.compression.quantization import quant_cols_ops
    w = case(R, K, 2)
    fake, _, _ = oracle(np.ascontiguousarray(w.T).reshape(-1, g))          # group k * (R / g) + r / g
    wd = gpu(w)
    assert quant_cols_ops.path(wd, g) == path
    out = quant_cols_ops.fake_quant_cols(wd, g, False, False, QMIN, QMAX)
    eq_bits(out.cpu().numpy(), fake.reshape(K, R).T, f'quant_dynamic_cols {name}')


# ---- llmc_quant_dynamic_mixed with every column integer --------------------------------------------------------------------
# mixed_t (mixed_quant.hip): no int_idx -> k_mixed_mask, a team of pow2(K / 16) lanes per row, above 64 the workgroup;
# int_idx with g <= 1024 -> k_mixed_idx with sub-wave teams of pow2(g / 8) <= 64 lanes; g > 1024 -> the workgroup is the team
@pytest.mark.parametrize('name,N,K,g,indexed', [('mask', 24, 64, 64, False), ('mask_workgroup', 4, 1088, 1088, False),
                                                ('idx_subwave', 24, 64, 16, True), ('idx_workgroup', 4, 1088, 1088, True)])
def test_mixed(name, N, K, g, indexed):
    from llmc_amd import _ffi
    x = case(N, K, 3)
    idx = np.random.default_rng(4).permutation(K).astype(np.int32) if indexed else np.arange(K, dtype=np.int32)
    fake, _, _ = oracle(np.ascontiguousarray(x[:, idx]).reshape(-1, g))
    want = np.empty_like(x)
    want[:, idx] = fake.reshape(N, K)
    xd, role = gpu(x), torch.ones(K, dtype=torch.uint8, device='cuda')
    idxd = gpu(idx) if indexed else None
    out = torch.empty_like(xd)
    _ffi.check(_ffi.lib().llmc_quant_dynamic_mixed(_ffi.ptr(xd), _ffi.dt(xd), N, K, _ffi.ptr(role), _ffi.ptr(idxd), K, g, 0, 0,
                                                   QMIN, QMAX, _ffi.ptr(out), _ffi.stream()), 'llmc_quant_dynamic_mixed')
    eq_bits(out.cpu().numpy(), want, f'quant_dynamic_mixed {name}')
