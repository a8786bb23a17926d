// Host side of csrc/fp4_quant.hip under AddressSanitizer / UBSan, without a GPU: argument checks, the kernel choice (lane count
// and shift of k_fpx_seg, the LDS size of k_fpx_row) and the workspace split of the two-read path, for every dtype / format /
// geometry class. Kernel launches fail for want of a device (LLMC_EIO) or succeed; either way the host code has run.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         llmc_amd/csrc/fp4_quant.hip tools/probes/fpx_host_check.cpp -o fpx_host_check -Lllmc_amd/csrc -lllmc_hip \
//         -Wl,-rpath,$PWD/llmc_amd/csrc && ./fpx_host_check
// (the library supplies llmc_minmax_qparams and the error plumbing; fp4_quant.hip's own entries come from the sanitized object)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../include/llmc_hip.h"

int main() {
    std::vector<char> w(1 << 16), out(1 << 16), sc(1 << 12), ws(1 << 16), cols(1 << 12);
    int calls = 0, refused = 0;
    const int64_t geoms[][2] = {{4, 128}, {3, 320}, {5, 33}, {2, 16384}, {1, 16392}, {1, 960}, {7, 8}, {1, 512}, {2, 4}};
    for (int dt = 0; dt < 3; ++dt)
        for (int fmt = 0; fmt < 4; ++fmt)
            for (int flags : {0, 0x100, 0x300, 0x200, 0x800, 0x1000})
                for (auto& g : geoms)
                    for (int st = 0; st < 2; ++st)
                        for (int off = 0; off < 2; ++off)
                            for (int wc = 0; wc < 2; ++wc) {
                                if (g[0] * g[1] * 4 + 16 > (int64_t)w.size()) continue;
                                const int rc = llmc_fpx_quant(w.data() + 2 * off, dt, g[0], g[1], wc ? cols.data() : nullptr, wc ? g[1] : 0,
                                                              1 | (fmt << 4) | flags, out.data(), sc.data(), dt, st, ws.data(), nullptr);
                                ++calls;
                                refused += rc == LLMC_EINVAL || rc == LLMC_ENOTSUP;
                            }
    if (llmc_fpx_quant_ws_bytes(4, 128) > ws.size() || llmc_fpx_quant_ws_bytes(1, 16392) > ws.size()) return 2;
    refused += llmc_fp4_pack(w.data(), 4, 127, out.data(), nullptr) != 0;
    llmc_fp4_pack(w.data(), 4, 128, out.data(), nullptr);
    for (int fmt = 1; fmt < 4; ++fmt)
        for (int packed = 0; packed < 2; ++packed)
            for (int sdt = -1; sdt < 4; ++sdt) refused += llmc_fpx_dequant(w.data(), fmt, packed, sc.data(), sdt, 4, 128, out.data(), 1, nullptr) != 0;
    printf("fpx host check: %d quant calls, %d refusals, no sanitizer report\n", calls, refused);
    return 0;
}
