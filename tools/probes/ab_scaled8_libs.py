"""A/B of the FP8 and int8 scaled GEMMs (csrc/fp8_linear.hip, csrc/i8_linear.hip) between two builds of the library in ONE process:
    python tools/probes/ab_scaled8_libs.py parent.so parent_copy.so new.so out.txt [f16 | bf16 | f32]
parent.so is another commit's libllmc_hip.so, parent_copy.so a second copy of that file (its own inode, so it is loaded again), new.so
this tree's. Calls llmc_fp8_scaled_gemm_on_rung / llmc_i8_scaled_gemm_on_rung on preallocated buffers (the output dtype named last, bf16 if none; per-token and
per-channel scales) on the four Llama-3-8B shapes: tile128 at 4096 and 256 tokens, decode at 64, 16 and 1, int8 decode_split at 64 and
32 on 1024 x 4096. 9 interleaved rounds (parent, new, parent copy) of equal batches of about 20 ms under device events, medians per
call; below 1024 tokens the weight comes from rotating copies of 320 MiB in all (more than the Infinity Cache). The three outputs are
compared bit for bit. A shape's noise is the largest relative difference between the two parent copies' medians over the rows of
that format and N x K; a row passes when new <= parent * (1 + noise)."""
import ctypes as C
import sys

import torch

ROTATE_BYTES = 320 << 20
SHAPES = ((4096, 4096), (1024, 4096), (14336, 4096), (4096, 14336))        # N x K
OUT_DTYPES = {'f16': (0, torch.float16), 'bf16': (1, torch.bfloat16), 'f32': (2, torch.float32)}      # LLMC_F16 / BF16 / F32
I64, VP, SZ = C.c_int64, C.c_void_p, C.c_size_t


def load(path):
    L = C.CDLL(path)
    L.llmc_fp8_scaled_gemm_on_rung.restype = C.c_int
    L.llmc_fp8_scaled_gemm_on_rung.argtypes = [VP, VP, I64, VP, VP, I64, I64, I64, I64, C.c_int, VP, VP, C.c_int, VP]
    L.llmc_i8_scaled_gemm_on_rung.restype = C.c_int
    L.llmc_i8_scaled_gemm_on_rung.argtypes = [VP, VP, I64, VP, VP, I64, I64, I64, I64, C.c_int, VP, VP, VP, SZ, C.c_int, VP]
    L.llmc_i8_scaled_gemm_ws_bytes.restype = SZ
    L.llmc_i8_scaled_gemm_ws_bytes.argtypes = [I64, I64, I64]
    return L


def batch_time(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls


def interleaved(arms, rounds):
    calls = {}
    for k, fn in arms.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[k] = max(10, min(4000, int(0.02 / batch_time(fn, 10))))
    n = max(calls.values())                 # the same batch for every arm of a row
    ts = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ts[k].append(batch_time(fn, n))
    return {k: sorted(v)[len(v) // 2] for k, v in ts.items()}


def main():
    paths, out = sys.argv[1:4], sys.argv[4]
    out_name = sys.argv[5] if len(sys.argv) > 5 else 'bf16'
    out_dt, out_torch = OUT_DTYPES[out_name]
    bits = torch.int32 if out_name == 'f32' else torch.int16
    libs = dict(zip(('parent', 'parent copy', 'new'), (load(p) for p in paths)))
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device='cuda').manual_seed(0)
    lines, failed = [], 0

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'output dtype {out_name}')
    say(f'{"format rung":22s} {"tokens":>6s} {"N":>6s} {"K":>6s} {"parent us":>10s} {"copy us":>10s} {"new us":>10s} {"|p-c|":>7s} {"new/parent":>10s}  verdict, bits')
    for fmt in ('fp8', 'i8'):
        for N, K in SHAPES:
            if fmt == 'fp8':
                w8 = (torch.randn(N, K, generator=g, device='cuda') * 0.5).to(torch.float8_e4m3fn)
            else:
                w8 = torch.randint(-127, 128, (N, K), generator=g, device='cuda', dtype=torch.int8)
            w_s = (torch.rand(N, generator=g, device='cuda') * 0.01 + 0.001).float()
            nrot = -(-ROTATE_BYTES // (N * K))
            rot = [w8] + [w8.clone() for _ in range(nrot - 1)]
            rows = [(4096, 1, 'tile128'), (256, 1, 'tile128'), (64, 0, 'decode'), (16, 0, 'decode'), (1, 0, 'decode')]
            if fmt == 'i8' and N == 1024:
                rows += [(64, 2, 'decode_split'), (32, 2, 'decode_split')]
            shape_rows = []
            for M, rung, rname in rows:
                if fmt == 'fp8':
                    a8 = torch.randn(M, K, generator=g, device='cuda').to(torch.float8_e4m3fn)
                else:
                    a8 = torch.randint(-127, 128, (M, K), generator=g, device='cuda', dtype=torch.int8)
                a_s = (torch.rand(M, generator=g, device='cuda') * 0.01 + 0.001).float()
                cs = {k: torch.zeros(M, N, dtype=out_torch, device='cuda') for k in libs}
                nb = libs['parent'].llmc_i8_scaled_gemm_ws_bytes(M, N, K) if rung == 2 else 0
                assert nb == (libs['new'].llmc_i8_scaled_gemm_ws_bytes(M, N, K) if rung == 2 else 0)
                ws = torch.empty(max(nb, 4), dtype=torch.uint8, device='cuda')
                turn = {k: 0 for k in libs}

                def call(k, rotate=True):
                    w = w8
                    if rotate and M < 1024:
                        turn[k] = (turn[k] + 1) % nrot
                        w = rot[turn[k]]
                    L = libs[k]
                    if fmt == 'fp8':
                        rc = L.llmc_fp8_scaled_gemm_on_rung(a8.data_ptr(), a_s.data_ptr(), M, w.data_ptr(), w_s.data_ptr(), N, M, N, K, out_dt,
                                                            None, cs[k].data_ptr(), rung, st)
                    else:
                        rc = L.llmc_i8_scaled_gemm_on_rung(a8.data_ptr(), a_s.data_ptr(), M, w.data_ptr(), w_s.data_ptr(), N, M, N, K, out_dt,
                                                           None, cs[k].data_ptr(), ws.data_ptr() if nb else None, nb, rung, st)
                    assert rc == 0, (k, fmt, rname, M, N, K, rc)

                for k in libs:
                    call(k, rotate=False)
                torch.cuda.synchronize()
                same = all(torch.equal(cs['parent'].view(bits), cs[k].view(bits)) for k in libs)
                assert bool(cs['new'].float().abs().sum() > 0)
                t = interleaved({k: (lambda k=k: call(k)) for k in ('parent', 'new', 'parent copy')}, rounds=9)
                p, pc, nw = t['parent'], t['parent copy'], t['new']
                shape_rows.append((fmt + ' ' + rname, M, p, pc, nw, same))
            noise = max(abs(p - pc) / min(p, pc) for _, _, p, pc, _, _ in shape_rows)
            for name, M, p, pc, nw, same in shape_rows:
                ok = nw <= p * (1 + noise)
                failed += not ok
                say(f'{name:22s} {M:6d} {N:6d} {K:6d} {p * 1e6:10.2f} {pc * 1e6:10.2f} {nw * 1e6:10.2f} {abs(p - pc) / min(p, pc) * 100:6.2f}% {nw / p:10.4f}  '
                    f'{"within" if ok else "SLOWER than parent +"} the noise of the shape {noise * 100:.2f}%, {"same bits" if same else "BITS DIFFER"}')
            del rot
    say(f'{failed} rows slower than the parent by more than their shape\'s noise')
    with open(out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
