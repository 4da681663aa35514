// The weight packers of roomnet_amd/csrc/rn_pack.h as a host program (tests/test_pack_host.py):
//
//     pack_main k32 NCHUNKS COUT DTYPE in.bin out.bin      in.bin: float32 [32 NCHUNKS][COUT], out.bin: the uint16 fragments
//     pack_main k48 COUT DTYPE in.bin out.bin              in.bin: float32 [9 x 64][COUT]
//
// DTYPE: 1 = bf16, 2 = f16 (RN_DTYPE_*).  c++ -std=c++17 -I include -I roomnet_amd/csrc tools/pack_main.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rn_pack.h"

int main(int argc, char** argv) {
    const bool k48 = argc == 6 && !std::strcmp(argv[1], "k48");
    if (!k48 && !(argc == 7 && !std::strcmp(argv[1], "k32"))) {
        std::fprintf(stderr, "usage: pack_main k32 NCHUNKS COUT DTYPE in out | pack_main k48 COUT DTYPE in out\n");
        return 2;
    }
    const int nchunks = k48 ? 18 : std::atoi(argv[2]);
    const int cout = std::atoi(argv[argc - 4]), dtype = std::atoi(argv[argc - 3]);
    if (nchunks <= 0 || cout <= 0 || cout % 16 || (dtype != RN_DTYPE_BF16 && dtype != RN_DTYPE_F16)) return 2;
    std::vector<float> w(static_cast<size_t>(32) * nchunks * cout);
    FILE* in = std::fopen(argv[argc - 2], "rb");
    if (!in || std::fread(w.data(), sizeof(float), w.size(), in) != w.size()) {
        std::fprintf(stderr, "pack_main: %s does not hold %zu floats\n", argv[argc - 2], w.size());
        return 1;
    }
    std::fclose(in);
    std::vector<unsigned short> frag;
    if (k48)
        rn_pack_k48(w.data(), cout, dtype, &frag);
    else
        rn_pack_k32(w.data(), nchunks, cout, dtype, &frag);
    FILE* out = std::fopen(argv[argc - 1], "wb");
    if (!out || std::fwrite(frag.data(), sizeof(unsigned short), frag.size(), out) != frag.size()) return 1;
    std::fclose(out);
    return 0;
}
