// The ranking of a heat map for the deletion / insertion curves (rn_faith.hip): a stable least-significant-
// digit radix sort of one (key, raster index) pair per pixel, 8-bit digits, four passes, ending in rank[sorted_index[r]] = r.
//   order   map value descending; equal values by raster index ascending; -0.0 equals +0.0; NaN behind everything else, NaNs among
//           themselves by index: np.argsort(-m.ravel(), kind="stable").
//   key     0 for NaN; otherwise u = bits(v + 0.0f), key = u ^ 0xFFFFFFFF when the sign bit of u is set, else u ^ 0x80000000 -- the
//           usual order-preserving map of a float onto an unsigned integer.  Sorted by 0xFFFFFFFF - key ascending, stably.
// One workgroup of kWaves waves ranks one image.  The npix pixels are cut into tiles of 64; wave w owns the contiguous tiles
// [t0, t1) of tile_range and walks them in order, so "earlier in the buffer" is "earlier wave, then earlier tile, then lower lane".
// Per pass:
//   count    per tile, lanes with the same digit find each other (peer_mask from the eight ballots of the digit's bits); the lowest
//            lane of a peer group adds the group's size to cnt[w][digit] -- no atomic, a wave's tiles come one after the other;
//   scan     scan_digit turns cnt[.][d] into each wave's exclusive prefix within digit d and leaves the digit's total, scan_totals
//            turns the 256 totals into exclusive prefixes: element (d, w) starts at total[d] + cnt[w][d], the (digit, wave) order;
//   scatter  the second walk: a lane's position is total[d] + cnt[w][d] + (its peers in lower lanes), then the group's lowest
//            lane advances cnt[w][d] by the group's size.
// No atomic decides a position: the same map gives the same ranks on every run.
// Everything above the model is __host__ __device__; compiled as plain C++ the file includes no HIP header, and rank_model runs
// the same steps lane after lane (tools/faith_rank_main.cpp, tests/test_faithfulness_host.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define RN_HD __host__ __device__
#else
#ifndef RN_HD
#define RN_HD
#endif
#endif

namespace rn_faith {

constexpr int kWaves = 16;              // waves of the ranking workgroup
constexpr int kDigits = 256;            // 8-bit digits
constexpr int kPasses = 4;

// the ascending sort key of a map value given as its bits: 0xFFFFFFFF - key
RN_HD inline uint32_t sort_key(uint32_t bits) {
    if ((bits & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;         // NaN: key 0
    const uint32_t u = bits == 0x80000000u ? 0u : bits;                 // v + 0.0f: -0.0 becomes +0.0, nothing else changes
    const uint32_t key = (u & 0x80000000u) ? u ^ 0xFFFFFFFFu : u ^ 0x80000000u;
    return 0xFFFFFFFFu - key;
}

RN_HD inline uint32_t digit_of(uint32_t key, int pass) { return (key >> (8 * pass)) & 0xFFu; }

// wave w's tiles [t0, t1) of the npix pixels: contiguous, ceil(tiles / kWaves) each
RN_HD inline void tile_range(int npix, int w, int* t0, int* t1) {
    const int tiles = (npix + 63) / 64, per = (tiles + kWaves - 1) / kWaves;
    const int a = w * per, b = a + per;
    *t0 = a < tiles ? a : tiles;
    *t1 = b < tiles ? b : tiles;
}

// The lanes of a tile that hold `digit`: `bit[b]` is the ballot of "valid and bit b of the digit set", `valid` the ballot of the
// lanes inside the image (the tail tile).
RN_HD inline uint64_t peer_mask(const uint64_t (&bit)[8], uint64_t valid, uint32_t digit) {
    uint64_t peers = valid;
#pragma unroll
    for (int b = 0; b < 8; ++b) peers &= ((digit >> b) & 1u) ? bit[b] : ~bit[b];
    return peers;
}

RN_HD inline int peers_below(uint64_t peers, int lane) { return __builtin_popcountll(peers & ((1ull << lane) - 1ull)); }
RN_HD inline int peers_all(uint64_t peers) { return __builtin_popcountll(peers); }
RN_HD inline bool peers_lowest(uint64_t peers, int lane) { return (peers & ((1ull << lane) - 1ull)) == 0; }

// cnt[w * kDigits + d] over the waves -> each wave's exclusive prefix within digit d; total[d] = the digit's count
RN_HD inline void scan_digit(uint32_t* cnt, uint32_t* total, int d) {
    uint32_t run = 0;
    for (int w = 0; w < kWaves; ++w) {
        const uint32_t c = cnt[w * kDigits + d];
        cnt[w * kDigits + d] = run;
        run += c;
    }
    total[d] = run;
}

// the 256 totals -> exclusive prefixes
RN_HD inline void scan_totals(uint32_t* total) {
    uint32_t run = 0;
    for (int d = 0; d < kDigits; ++d) {
        const uint32_t c = total[d];
        total[d] = run;
        run += c;
    }
}

// ---- the host model: the kernel's passes with the waves, tiles and lanes run one after another
inline void rank_model_image(const float* map, int npix, uint32_t* rank) {
    std::vector<uint32_t> key[2], idx[2];
    for (int s = 0; s < 2; ++s) {
        key[s].resize(static_cast<size_t>(npix));
        idx[s].resize(static_cast<size_t>(npix));
    }
    std::vector<uint32_t> cnt(static_cast<size_t>(kWaves) * kDigits), total(kDigits);
    for (int pass = 0; pass < kPasses; ++pass) {
        const uint32_t* kin = key[(pass + 1) & 1].data();         // (pass 0 reads the map itself)
        const uint32_t* iin = idx[(pass + 1) & 1].data();
        uint32_t* kout = key[pass & 1].data();
        uint32_t* iout = idx[pass & 1].data();
        std::fill(cnt.begin(), cnt.end(), 0u);
        for (int phase = 0; phase < 2; ++phase) {                 // 0: count, 1: scatter
            for (int w = 0; w < kWaves; ++w) {
                int t0, t1;
                tile_range(npix, w, &t0, &t1);
                for (int t = t0; t < t1; ++t) {
                    uint32_t k[64] = {}, ix[64] = {}, dg[64] = {};
                    uint64_t bit[8] = {}, valid = 0;
                    for (int lane = 0; lane < 64; ++lane) {
                        const int e = t * 64 + lane;
                        if (e >= npix) continue;
                        valid |= 1ull << lane;
                        if (pass == 0) {
                            uint32_t bits;
                            std::memcpy(&bits, map + e, 4);
                            k[lane] = sort_key(bits);
                            ix[lane] = static_cast<uint32_t>(e);
                        } else {
                            k[lane] = kin[e];
                            ix[lane] = iin[e];
                        }
                        dg[lane] = digit_of(k[lane], pass);
                        for (int b = 0; b < 8; ++b)
                            if ((dg[lane] >> b) & 1u) bit[b] |= 1ull << lane;
                    }
                    // (every lane reads its counter before any lane of the tile advances one: the kernel's instruction order)
                    uint32_t pos[64] = {};
                    uint64_t peers[64] = {};
                    for (int lane = 0; lane < 64; ++lane) {
                        if (!((valid >> lane) & 1ull)) continue;
                        peers[lane] = peer_mask(bit, valid, dg[lane]);
                        if (phase == 1) pos[lane] = total[dg[lane]] + cnt[static_cast<size_t>(w) * kDigits + dg[lane]] + peers_below(peers[lane], lane);
                    }
                    for (int lane = 0; lane < 64; ++lane) {
                        if (!((valid >> lane) & 1ull)) continue;
                        if (peers_lowest(peers[lane], lane)) cnt[static_cast<size_t>(w) * kDigits + dg[lane]] += peers_all(peers[lane]);
                        if (phase == 0) continue;
                        if (pass == kPasses - 1) {
                            rank[ix[lane]] = pos[lane];
                        } else {
                            kout[pos[lane]] = k[lane];
                            iout[pos[lane]] = ix[lane];
                        }
                    }
                }
            }
            if (phase == 0) {
                for (int d = 0; d < kDigits; ++d) scan_digit(cnt.data(), total.data(), d);
                scan_totals(total.data());
            }
        }
    }
}

}  // namespace rn_faith
