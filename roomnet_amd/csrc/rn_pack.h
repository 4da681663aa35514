// Weight fragments of the kernels on 16x16x32 matrix tiles (rn_stage4x / 5x / 6x.hip, rn_conv16.hip, rn_backend.hip): one lane of an
// MFMA operand holds 8 consecutive K elements of one cout.  Plain C++ (no HIP): tools/pack_main.cpp and tests/test_pack_host.py hold
// the two layouts to their formulas on the host.
// w_hwio is the checkpoint's HWIO kernel read as [k = tap * cin + channel][cout] (tap = ky * 3 + kx); dtype = RN_DTYPE_BF16 / RN_DTYPE_F16.
#pragma once
#include <cstddef>
#include <vector>

#include "rn_host16.h"

// K in chunks of 32:  frag[chunk c][cout tile t][lane][j] = W[k = 32 c + 8 (lane / 16) + j][cout = 16 t + lane % 16]
// for c < nchunks = 9 cin / 32 and t < cout / 16.  With cin = 32 chunk c is tap c (rn_stage4x.hip: 9 chunks, 64 couts); with cin = 64 it
// is (tap c / 2, channel half c % 2) (rn_stage5x.hip: 18, 64; rn_stage6x.hip and conv16_kernel: 18, 128); conv16p_kernel: 36, 16.
inline void rn_pack_k32(const float* w_hwio, int nchunks, int cout, int dtype, std::vector<unsigned short>* out) {
    const int ntiles = cout / 16;
    out->assign(static_cast<size_t>(nchunks) * ntiles * 64 * 8, 0);
    for (int c = 0; c < nchunks; ++c)
        for (int t = 0; t < ntiles; ++t)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int k = 32 * c + 8 * (l >> 4) + j, co = 16 * t + (l & 15);
                    (*out)[((static_cast<size_t>(c) * ntiles + t) * 64 + l) * 8 + j] = rn_to16(w_hwio[static_cast<size_t>(k) * cout + co], dtype);
                }
}

// K48: a 64-channel stage without its input channels 48..63 (constants on the handle; StageArgs::cstart carries their sum): five
// fragments per kernel row instead of six.  frag[f = ky * 5 + j][cout tile t][lane][e] with g = lane / 16, cout = 16 t + lane % 16:
//   j < 3:  W[tap (ky, kx = j)][channel 8 g + e]
//   j = 3:  lane groups 0, 1 = W[tap (ky, 0)][channel 32 + 8 g + e], groups 2, 3 = W[tap (ky, 1)][channel 32 + 8 (g - 2) + e]
//   j = 4:  groups 0, 1 = W[tap (ky, 2)][channel 32 + 8 g + e], groups 2, 3 = 0
// (rn_stage5x.hip: 64 couts, rn_stage6x.hip: 128)
inline void rn_pack_k48(const float* w_hwio, int cout, int dtype, std::vector<unsigned short>* out) {
    const int ntiles = cout / 16;
    out->assign(static_cast<size_t>(15) * ntiles * 64 * 8, 0);
    for (int ky = 0; ky < 3; ++ky)
        for (int j = 0; j < 5; ++j)
            for (int t = 0; t < ntiles; ++t)
                for (int l = 0; l < 64; ++l)
                    for (int e = 0; e < 8; ++e) {
                        const int g = l >> 4, co = 16 * t + (l & 15);
                        if (j == 4 && g >= 2) continue;
                        const int kx = j < 3 ? j : j == 3 ? g >> 1 : 2;
                        const int ch = j < 3 ? 8 * g + e : 32 + 8 * (g & 1) + e;
                        const float v = w_hwio[(static_cast<size_t>(ky * 3 + kx) * 64 + ch) * cout + co];
                        (*out)[((static_cast<size_t>(ky * 5 + j) * ntiles + t) * 64 + l) * 8 + e] = rn_to16(v, dtype);
                    }
}
