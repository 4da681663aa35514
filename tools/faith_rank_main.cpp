// Host-sanitizer run of the heat-map ranking's host model (roomnet_amd/csrc/rn_faith_rank.h): a stand-alone program, no GPU, no HIP.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iroomnet_amd/csrc \
//       tools/faith_rank_main.cpp -o build/faith_rank && build/faith_rank
//
// For the pixel counts 1, 63, 64, 65, 4095, 4096, 4097, 33 489 (side 183), 50 176 (224) and 481 636 (694) -- below, at and above a
// tile, around 64 tiles, tails of 17 and 36 mod 64, 19-bit indices -- seeded maps go through rank_model_image (the kernel's count,
// scan and scatter, wave after wave, tile after tile, lane after lane) into heap blocks of EXACTLY npix entries, so
// AddressSanitizer sees any access past them: random values, tie-heavy maps (8 distinct values), all-equal maps, a map with one
// large zero plateau, and maps strewn with +-0, +-inf, NaNs of both signs and denormals.  Every result is compared with
// std::stable_sort under the order the library defines (value descending, -0 equal to +0, NaN last, ties by index) and checked to
// be a permutation.  Prints one summary line; exit status 0 unless something differed (sanitizer findings abort the run).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <numeric>

#include "rn_faith_rank.h"

namespace {

uint64_t g_seed = 0x9e3779b97f4a7c15ull;
uint64_t next() {
    g_seed ^= g_seed << 13;
    g_seed ^= g_seed >> 7;
    g_seed ^= g_seed << 17;
    return g_seed;
}
float uniform() { return static_cast<float>(next() >> 40) / static_cast<float>(1 << 24) * 2.0f - 1.0f; }

float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

const char* kKinds[] = {"random", "ties", "equal", "plateau", "special"};

void fill(std::vector<float>& m, int kind) {
    const float inf = std::numeric_limits<float>::infinity();
    const float special[] = {0.0f, -0.0f, inf, -inf, from_bits(0x7FC00000u), from_bits(0xFFC00001u), from_bits(0x7F800001u),
                             from_bits(0x00000001u), from_bits(0x80000001u), 1.0f, -1.0f, std::numeric_limits<float>::max(),
                             std::numeric_limits<float>::lowest()};
    for (size_t e = 0; e < m.size(); ++e) {
        switch (kind) {
            case 0: m[e] = uniform(); break;
            case 1: m[e] = static_cast<float>(static_cast<int>(next() % 8)) * 0.25f - 1.0f; break;
            case 2: m[e] = 0.375f; break;
            case 3: m[e] = (e % 7 == 3) ? uniform() * uniform() : 0.0f; m[e] = m[e] < 0.0f ? 0.0f : m[e]; break;
            default: m[e] = next() % 3 ? special[next() % (sizeof(special) / sizeof(special[0]))] : uniform(); break;
        }
    }
}

// the order the library defines, stated without the key
bool before(float a, float b) {
    const bool na = std::isnan(a), nb = std::isnan(b);
    if (na || nb) return !na && nb;
    return a > b;                         // (-0.0f > +0.0f is false both ways: equal)
}

int check(int npix, int kind) {
    std::vector<float> m(static_cast<size_t>(npix));
    fill(m, kind);
    // exactly npix entries each, on the heap
    float* map = static_cast<float*>(std::malloc(sizeof(float) * npix));
    uint32_t* rank = static_cast<uint32_t*>(std::malloc(sizeof(uint32_t) * npix));
    std::memcpy(map, m.data(), sizeof(float) * npix);
    std::memset(rank, 0xFF, sizeof(uint32_t) * npix);
    rn_faith::rank_model_image(map, npix, rank);
    std::vector<uint32_t> order(static_cast<size_t>(npix));
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return before(m[a], m[b]); });
    int bad = 0;
    for (int r = 0; r < npix; ++r)
        if (rank[order[r]] != static_cast<uint32_t>(r)) {
            if (!bad) std::printf("npix %d, %s: pixel %u has rank %u, expected %d\n", npix, kKinds[kind], order[r], rank[order[r]], r);
            ++bad;
        }
    std::free(map);
    std::free(rank);
    return bad;
}

}  // namespace

int main() {
    const int sizes[] = {1, 63, 64, 65, 4095, 4096, 4097, 33489, 50176, 481636};
    int cases = 0, bad = 0;
    // the key alone on a few values: descending order of the value is ascending order of the key
    const float ladder[] = {std::numeric_limits<float>::infinity(), 3.0f, from_bits(0x00000001u), 0.0f, from_bits(0x80000001u), -3.0f,
                            -std::numeric_limits<float>::infinity()};
    for (size_t k = 0; k + 1 < sizeof(ladder) / sizeof(ladder[0]); ++k) {
        uint32_t a, b;
        std::memcpy(&a, &ladder[k], 4);
        std::memcpy(&b, &ladder[k + 1], 4);
        if (!(rn_faith::sort_key(a) < rn_faith::sort_key(b))) {
            std::printf("sort_key: %g is not in front of %g\n", ladder[k], ladder[k + 1]);
            ++bad;
        }
    }
    if (rn_faith::sort_key(0x80000000u) != rn_faith::sort_key(0u) || rn_faith::sort_key(0x7FC00000u) != 0xFFFFFFFFu ||
        rn_faith::sort_key(0xFFC00001u) != 0xFFFFFFFFu) {
        std::printf("sort_key: -0.0 / NaN\n");
        ++bad;
    }
    for (int npix : sizes)
        for (int kind = 0; kind < 5; ++kind) {
            bad += check(npix, kind) != 0;
            ++cases;
        }
    std::printf("faith_rank_main: %d maps over %zu pixel counts ranked by the host model, %d differ from std::stable_sort\n", cases,
                sizeof(sizes) / sizeof(sizes[0]), bad);
    return bad ? 1 : 0;
}
