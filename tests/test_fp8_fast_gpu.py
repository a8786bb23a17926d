"""The division-free form of the FP8 cast (csrc/fp8_quant.hip:fp8_fast8, its guard in csrc/float_quant_math.h) against the same
kernel with FP8_EXACT_DIV (every element through the IEEE division and the general encoder): identical codes and identical
fake-quantized values, for both semantics, bf16 and fp16, per_tensor and per_channel, on tensors large enough to hit every guard thousands of times."""
import time

import numpy as np
import pytest
import torch

from conftest import report

pytestmark = pytest.mark.gpu
EXACT_DIV = 0x200


def run(w, G, g, mode, sdt):
    from llmc_amd import _ffi
    L = _ffi.lib()
    fake = mode & 1
    out = torch.empty_like(w) if fake else torch.empty(w.shape, dtype=torch.uint8, device=w.device)
    s = torch.empty(G, dtype=sdt, device=w.device)
    ws = _ffi.workspace(L.llmc_fp8_quant_ws_bytes(G, g), w.device)
    _ffi.check(L.llmc_fp8_quant(_ffi.ptr(w), _ffi.dt(w), G, g, mode, _ffi.ptr(out), _ffi.ptr(s), _ffi.dt(sdt), 0, _ffi.ptr(ws),
                                _ffi.stream()), 'llmc_fp8_quant')
    return out, s


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('sem', [0x100, 0])
def test_fast_cast_equals_the_exact_division_path(dt, sem):
    gen = torch.Generator().manual_seed(5 + sem)
    R, K = 4096, 4096
    w = torch.randn(R, K, generator=gen) * 0.03
    w[torch.rand(R, K, generator=gen) < 1e-3] *= 6
    w[:, torch.randperm(K, generator=gen)[:4]] *= 20      # outlier channels: the per-tensor scale pushes ~0.3 % of the elements below 2^-6
    w[0, :64] = 0.0
    w[1, :64] = -0.0
    w[2, :64] = 1e-7                      # the 8-bit format's subnormal range after scaling
    w[3, :64] = 6e-8 if dt == torch.float16 else 1e-30
    w = w.to(dt).cuda()
    for gran, G, g, sdt in (('per_tensor', 1, R * K, torch.float32), ('per_channel', R, K, dt)):
        for fake in (0, 1):
            mode = fake | sem
            a, sa = run(w, G, g, mode, sdt)
            b, sb = run(w, G, g, mode | EXACT_DIV, sdt)
            assert torch.equal(sa, sb)
            if fake:
                assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (gran, fake, float((a != b).float().mean()))
            else:
                assert torch.equal(a, b), (gran, fake, float((a != b).float().mean()))


def run_static(w, G, g, mode, scales):
    from llmc_amd import _ffi
    L = _ffi.lib()
    out = torch.empty_like(w) if mode & 1 else torch.empty(w.shape, dtype=torch.uint8, device=w.device)
    _ffi.check(L.llmc_fp8_quant(_ffi.ptr(w), _ffi.dt(w), G, g, mode, _ffi.ptr(out), _ffi.ptr(scales), _ffi.dt(scales.dtype), 1, None,
                                _ffi.stream()), 'llmc_fp8_quant')
    return out


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
def test_every_bit_pattern_equals_the_exact_division_path(dt):
    """The guard of the division-free form (csrc/float_quant_math.h:DivFreeGuard) on ALL 65536 patterns of the dtype — NaN, +-inf,
    +-0 and subnormals included — per row, under static scales that exercise the zero -> 1 rule (0) and push quotients into the
    8-bit subnormal range (3e4); as one per_tensor row with an fp32 scale; and with [5] fp32 scales, which promote the quotient to
    fp32 (the fast form must not be taken). Each call equals the same call with FP8_EXACT_DIV, bit for bit.

    The bf16 row with scale 3e4 holds the case this test found: negative patterns 0x8001..0x83e7 have a quotient below half of
    bf16's smallest subnormal, rnd_bf16(w / s) is -0 and the reference's `+ zeros` makes it +0 (code 0x00); a division-free form
    that adds its zero before the rounding returns -0 (code 0x80) under the dtype-cast semantics."""
    from llmc_amd import _ffi
    R, K = 5, 65536
    row = torch.from_numpy(np.arange(K, dtype=np.uint16).view(np.int16)).view(dt)
    w = row.repeat(R, 1).contiguous().cuda()
    vals = [1.0, 0.0123, 2.0 ** -14, 0.0, 3e4]
    layouts = (('rows, scales in dt', R, K, torch.tensor(vals, dtype=dt).cuda()),
               ('one row, fp32 scale', 1, R * K, torch.tensor([0.0123], dtype=torch.float32).cuda()),
               ('rows, fp32 scales', R, K, torch.tensor(vals, dtype=torch.float32).cuda()))
    for fmt in (0, 0x10):                       # e4m3; e5m2 as the control (never on the fast form)
        for sem in (0x100, 0):
            for fake in (0, 1):
                for no_packed16 in (0, 1):
                    for name, G, g, s in layouts:
                        mode = fake | fmt | sem
                        with _ffi.option(fp8_no_packed16=no_packed16):
                            a = run_static(w, G, g, mode, s)
                            b = run_static(w, G, g, mode | EXACT_DIV, s)
                        where = (fmt, sem, fake, no_packed16, name)
                        if fake:
                            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), where
                        else:
                            assert torch.equal(a, b), where


def test_cast_rate_at_the_mixtral_expert_shape():
    """14336 x 4096 bf16 per_tensor (BASELINE configs[4]): absmax + cast, codes; reported, with a loose floor."""
    from llmc_amd.compression.quantization import FloatQuantizer
    w = (torch.randn(14336, 4096, device='cuda') * 0.02).to(torch.bfloat16)
    for sem in ('qtorch', 'cast'):
        q = FloatQuantizer('e4m3', True, 'per_tensor', use_qtorch=True, fp8_semantics=sem)
        for _ in range(3):
            q.real_quant_weight_dynamic(w)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 20
        for _ in range(n):
            q.real_quant_weight_dynamic(w)
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) / n * 1e6
        report('fp8_per_tensor_14336x4096/' + sem, us=us, tb_per_s_at_3B_per_element=3 * w.numel() / us / 1e6)
        assert us < 150
